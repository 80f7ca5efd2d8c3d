#!/usr/bin/env python
"""What composed prompts cost per step: the README cascade (unet1 + unet2, 64 -> 256, batch 8, one request at a time, CFG 7.5) under
sampler='dpmpp_2m' at 32 + 32 steps with plain guidance (2 B denoiser rows), K = 2 (3 B rows) and K = 3 (4 B rows, half-image masks),
ALTERNATING in one process on one box (the box-to-box spread is 17 %: only a same-call A/B counts):

    python tools/compose_step_bench.py [--out profiles/compose_step_mi355x.json] [--reps 5]

After a warm-up call of each leg (stages built, weights packed, graphs captured), `reps` rounds of one whole call per leg, in turn; the
median per leg, and the difference to plain guidance per step pair (one step of each stage).  The cost is the denoiser's further B rows per
prompt; COMPOSE_X0 itself is one launch, as CFG_X0 is."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

STEPS = 32


def legs(dev):
    p = lambda seed: torch.randn(1, 256, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    left = torch.zeros(1, 64, 64)
    left[..., :32] = 1.0
    return {"plain": {}, "k2": dict(compose=[dict(text_embeds=p(1), weight=3.0)]),
            "k3_masks": dict(compose=[dict(text_embeds=p(1), weight=3.0, mask=left), dict(text_embeds=p(2), weight=3.0, mask=1.0 - left)])}


def main():
    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_step_mi355x.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    te = torch.randn(8, 256, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    model = bench.build_imagen(1000, dev)
    LEGS = legs(dev)
    kw = dict(text_embeds=te, cond_scale=7.5, use_tqdm=False, sampler="dpmpp_2m", sample_steps=STEPS)
    for extra in LEGS.values():
        model.sample(seed=1, **kw, **extra)
    torch.cuda.synchronize()
    times = {name: [] for name in LEGS}
    for r in range(args.reps):
        for name, extra in LEGS.items():
            t0 = time.perf_counter()
            img = model.sample(seed=2 + r, **kw, **extra)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            assert bool(torch.isfinite(img).all())
    med = {name: statistics.median(t) for name, t in times.items()}
    res = dict(config=f"README unet1 + unet2, 64 -> 256, batch 8, CFG 7.5, dpmpp_2m {STEPS} + {STEPS} steps, one request at a time, legs alternating",
               device=torch.cuda.get_device_name(0), reps=args.reps, legs={"plain": "2 B rows, CFG_X0", "k2": "K = 2: one further prompt at weight 3, 3 B rows", "k3_masks": "K = 3: two further prompts at weight 3 under half-image masks, 4 B rows"},
               call_s=times, call_median_s=med,
               extra_us_per_step_pair={name: (med[name] - med["plain"]) / STEPS * 1e6 for name in LEGS if name != "plain"},
               spread_of_plain_us_per_step_pair=(max(times["plain"]) - min(times["plain"])) / STEPS * 1e6)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
