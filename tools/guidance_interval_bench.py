#!/usr/bin/env python
"""Time per call of the README cascade (unet1 + unet2, 64 -> 256, batch 8, one request at a time, CFG 3) with full guidance against
`guidance_interval=(0.2, 0.8)` on both stages, in ONE process on one box (the box-to-box spread is 17 %: only a same-call A/B counts):

    python tools/guidance_interval_bench.py [--out profiles/guidance_interval_mi355x.json] [--skip-ancestral]

Five whole calls each after a warm-up call, the median taken: under sampler='dpmpp_2m' at 32 + 32 steps, and under the ancestral sampler at
1000 + 1000.  Writes the four times, the guided / unguided steps per stage and the derived time per guided and per unguided step pair (one
step of each stage).  Per leg, from t_full = n g, t_interval = n_g g + n_u u: these two figures INCLUDE the per-call fixed costs (initial
noise, conditioning, the time-table pass, low-res prep) spread over the leg's steps, which 32 steps dilute far less than 1000.  Free of them
are `saved_ms_per_unguided_step_pair` = (t_full - t_interval) / n_u of each leg, and the `across_legs` block: g from the difference of the
two full-guidance times over the difference of their step counts (the two samplers' update launches differ by microseconds), the fixed cost
per call that leaves, and u = g - the saving.

    python tools/guidance_interval_bench.py --rederive FILE      # recompute the derived figures of a written file from its recorded times"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

INTERVAL = (0.2, 0.8)


def timed(model, reps, **kw):
    model.sample(seed=1, **kw)                              # builds the stages, packs the weights, captures the graphs
    torch.cuda.synchronize()
    out = []
    for i in range(reps):
        t0 = time.perf_counter()
        img = model.sample(seed=2 + i, **kw)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    assert bool(torch.isfinite(img).all())
    return out


def leg(name, timesteps, solver, reps, te):
    import bench
    from imagen_pytorch_amd.schedules import guidance_scales

    model = bench.build_imagen(timesteps, te.device)
    steps = solver.get("sample_steps", timesteps)
    kw = dict(text_embeds=te, cond_scale=3.0, use_tqdm=False, **solver)
    full = timed(model, reps, **kw)
    part = timed(model, reps, guidance_interval=INTERVAL, **kw)
    n_g = int((guidance_scales(steps, 3.0, None, INTERVAL) != 1.0).sum())
    n_u = steps - n_g
    t_full, t_part = statistics.median(full), statistics.median(part)
    g = t_full / steps
    u = (t_part - n_g * g) / n_u
    rec = dict(sampler=solver.get("sampler", "ddpm"), steps_per_stage=steps, guided_steps_per_stage=n_g, unguided_steps_per_stage=n_u,
               full_guidance_s=full, interval_s=part, full_guidance_median_s=t_full, interval_median_s=t_part,
               ms_per_guided_step_pair=g * 1e3, ms_per_unguided_step_pair=u * 1e3, unguided_over_guided=u / g, interval_over_full=t_part / t_full)
    print(f"{name}: full guidance {t_full:.3f} s, interval {INTERVAL} {t_part:.3f} s ({n_g} guided + {n_u} unguided steps per stage): "
          f"{g * 1e3:.2f} ms per guided step pair, {u * 1e3:.2f} ms per unguided one", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_interval_mi355x.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-ancestral", action="store_true")
    ap.add_argument("--rederive", metavar="FILE", default=None)
    args = ap.parse_args()
    if args.rederive:
        with open(args.rederive) as f:
            res = derive(json.load(f))
        with open(args.rederive, "w") as f:
            json.dump(res, f, indent=1)
        return
    dev = torch.device("cuda:0")
    te = torch.randn(8, 256, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    res = dict(config="README unet1 + unet2, 64 -> 256, batch 8, CFG 3, one request at a time", interval=list(INTERVAL), reps=args.reps,
               device=torch.cuda.get_device_name(0), legs={})
    res["legs"]["dpmpp_2m_32"] = leg("dpmpp_2m 32 + 32", 1000, dict(sampler="dpmpp_2m", sample_steps=32), args.reps, te)
    if not args.skip_ancestral:
        res["legs"]["ddpm_1000"] = leg("ddpm 1000 + 1000", 1000, {}, args.reps, te)
    derive(res)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


def derive(res):
    """The figures that do not carry the per-call fixed costs (see the module docstring), written into `res`."""
    legs = res["legs"]
    for rec in legs.values():
        rec["saved_ms_per_unguided_step_pair"] = (rec["full_guidance_median_s"] - rec["interval_median_s"]) / rec["unguided_steps_per_stage"] * 1e3
        rec["per_step_figures_include_call_overhead"] = True
    if len(legs) == 2:
        a, b = sorted(legs.values(), key=lambda r: r["steps_per_stage"])
        g = (b["full_guidance_median_s"] - a["full_guidance_median_s"]) / (b["steps_per_stage"] - a["steps_per_stage"]) * 1e3
        saved = statistics.mean(r["saved_ms_per_unguided_step_pair"] for r in (a, b))
        res["across_legs"] = dict(ms_per_guided_step_pair=g, ms_per_unguided_step_pair=g - saved, unguided_over_guided=(g - saved) / g,
                                  fixed_ms_per_call=a["full_guidance_median_s"] * 1e3 - a["steps_per_stage"] * g)
        print("across the legs (call overhead removed): " + ", ".join(f"{k} {v:.3f}" for k, v in res["across_legs"].items()))
    return res


if __name__ == "__main__":
    main()
