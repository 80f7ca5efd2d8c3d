#!/usr/bin/env python
"""What tiled sampling costs per step: the README cascade (unet1 + unet2, batch 2, one request at a time, CFG 7.5) under sampler='dpmpp_2m' at
32 + 32 steps with the second stage at 256 x 1024 (the first at 64 x 256, untiled in both legs),

    untiled   image_shapes alone: 2 B denoiser rows at 256 x 1024
    tiled     tile_shapes=(None, (256, 256)), tile_overlap=64: T = 5, 2 T B rows at 256 x 256, two TILES launches per step

ALTERNATING in one process on one box (the box-to-box spread is 17 %: only a same-call A/B counts):

    python tools/tile_step_bench.py [--out profiles/tile_step_mi355x.json] [--reps 5]

After a warm-up call of each leg (stages built, weights packed, graphs captured), `reps` rounds of one whole call per leg, in turn; the median
per leg and the difference per step pair (one step of each stage).  Beside it the two TILES launches of a stage-2 step on their own (gather of
the canvas into T B tile rows, blend of T B tile rows into x0 and |x0|), timed with events over `--launches` replays, and a device copy of the
tile rows' bytes (T B C h w floats) as the yardstick of a streaming launch of that size."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

STEPS, B = 32, 2
SHAPES, TILE, OVERLAP = ((64, 256), (256, 1024)), (256, 256), 64


def event_us(fn, n):
    """Mean microseconds of fn() over n calls on the current stream (after 3 warm-up calls)."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def tiles_alone(dev, n):
    from imagen_pytorch_amd import ops
    from imagen_pytorch_amd.sample_call import tile_geometry

    (H, W), (h, w) = SHAPES[1], TILE
    geo = tile_geometry(H, W, h, w, OVERLAP, OVERLAP)
    T, C = geo["T"], 3
    canvas, x0, ab = (torch.randn(B, C, H, W, device=dev) for _ in range(3))
    rows, rows2 = torch.randn(T * B, C, h, w, device=dev), torch.empty(T * B, C, h, w, device=dev)
    origins, nw = geo["origins"].to(dev), geo["nw"].to(dev)
    dims = dict(B=B, C=C, H=H, W=W, h=h, w=w)
    gather, blend = ops.Plan("gather"), ops.Plan("blend")
    ops.tiles(gather, canvas, rows2, origins, mode="gather", **dims)
    ops.tiles(blend, rows, x0, origins, mode="blend", nw=nw, absdst=ab, **dims)
    return dict(T=T, tile_rows_bytes=rows.numel() * 4, canvas_bytes=canvas.numel() * 4,
                gather_us=event_us(gather.run, n), blend_us=event_us(blend.run, n), copy_of_tile_rows_us=event_us(lambda: rows2.copy_(rows), n))


def main():
    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_step_mi355x.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    te = torch.randn(B, 256, 768, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    model = bench.build_imagen(1000, dev)
    LEGS = {"untiled": {}, "tiled": dict(tile_shapes=(None, TILE), tile_overlap=OVERLAP)}
    kw = dict(text_embeds=te, cond_scale=7.5, use_tqdm=False, sampler="dpmpp_2m", sample_steps=STEPS, image_shapes=SHAPES)
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
            assert bool(torch.isfinite(img).all()) and tuple(img.shape) == (B, 3, *SHAPES[1])
    med = {name: statistics.median(t) for name, t in times.items()}
    alone = tiles_alone(dev, args.launches)
    T = alone["T"]
    res = dict(config=f"README unet1 + unet2, {SHAPES[0]} -> {SHAPES[1]}, batch {B}, CFG 7.5, dpmpp_2m {STEPS} + {STEPS} steps, one request at a time, legs alternating",
               device=torch.cuda.get_device_name(0), reps=args.reps,
               legs={"untiled": f"2 B = {2 * B} rows at 256 x 1024", "tiled": f"T = {T}: 2 T B = {2 * T * B} rows at 256 x 256, overlap {OVERLAP}, two TILES launches per step"},
               rows_ratio=T, pixels_per_row_ratio=TILE[0] * TILE[1] / (SHAPES[1][0] * SHAPES[1][1]), denoiser_pixels_ratio=T * TILE[0] * TILE[1] / (SHAPES[1][0] * SHAPES[1][1]),
               call_s=times, call_median_s=med, ms_per_step_pair={name: med[name] / STEPS * 1e3 for name in LEGS},
               tiled_over_untiled=med["tiled"] / med["untiled"],
               spread_of_untiled_ms_per_step_pair=(max(times["untiled"]) - min(times["untiled"])) / STEPS * 1e3,
               tiles_launches_alone=alone)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
