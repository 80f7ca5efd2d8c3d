#!/usr/bin/env python
"""Kernel-level timing of TEMPORAL_ATTENTION (csrc/temporal.hip) at the C5 shape — B = 2 rows x F = 16 frames x P = 64^2 pixels, inner width
512 — three ways: 16 heads x 32 on the MFMA kernel, the same shape on the vector kernel (an o row stride of 514 halfs is no multiple of 4, which
keeps a launch off the MFMA route), and 8 heads x 64 on the MFMA kernel.  Events on the launch stream over four rotating qkv / o buffer sets
(as tools/attn_bench.py).

    python tools/temporal_attn_bench.py [--iters 30] [--out file.jsonl]
    python tools/temporal_attn_bench.py --long     # the long-clip pair instead: 2 x 64 frames x 32^2, 8 heads x 64 on the tiled kernel
                                                   # (ABI 15), and 2 x 32 frames x 32^2 on the route of before (F = 32: the vector kernel)

One JSON line per case: us per launch, the bytes a launch has to move (qkv rows in, o rows out) and the GB/s that makes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from imagen_pytorch_amd import ops  # noqa: E402
from imagen_pytorch_amd.ops import Act  # noqa: E402

CASES = [("d32_mfma", 16, 32, 0), ("d32_vector", 16, 32, 2), ("d64_mfma", 8, 64, 0)]   # (name, heads, head dim, pad columns of an o row)
LONG_CASES = [("d64_long_f64", 8, 64, 0, 64), ("d64_short_f32", 8, 64, 0, 32)]          # (..., frames) at P = 32^2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--long", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P = 2, (32 * 32 if args.long else 64 * 64)
    g = torch.Generator().manual_seed(0)
    lines, first = [], {}
    for name, heads, D, pad, Fr in (LONG_CASES if args.long else [c + (16,) for c in CASES]):
        C = heads * D
        rows = B * Fr * P
        null_kv, qs, ks = torch.randn(2, D, generator=g).to(dev), (torch.rand(D, generator=g) + 0.5).to(dev), (torch.rand(D, generator=g) + 0.5).to(dev)
        bias = torch.randn(heads, Fr, Fr + 1, generator=g).to(dev)
        src = torch.Generator().manual_seed(1)
        plan = ops.Plan("bench")
        sets = []
        for i in range(4):
            qkv = ops.new_act(1, 1, rows, C + 2 * D, dev)
            if i == 0:
                qkv.t.copy_(torch.randn(rows, C + 2 * D, generator=src).half().reshape(qkv.t.shape))
            else:
                qkv.t.copy_(sets[0][0].t)
            ot = torch.zeros(rows, C + pad, dtype=torch.float16, device=dev)
            ops.temporal_attention(plan, qkv, null_kv, qs, ks, bias, Act(ot, 1, 1, rows, C, C + pad, rows * (C + pad)), B=B, F=Fr, P=P, heads=heads,
                                   causal=True, scale=8.0, head_dim=D)
            sets.append((qkv, ot))
        plan.run()
        torch.cuda.synchronize()
        out = sets[0][1][:, :C].float()
        dist = None
        if (D, Fr) in first:                            # the two D = 32 routes compute the same thing
            dist = float(((out - first[D, Fr]).norm() / first[D, Fr].norm()).item())
        first.setdefault((D, Fr), out.clone())
        for _ in range(3):
            plan.run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            plan.run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (4 * args.iters)
        nbytes = rows * (C + 2 * D + C) * 2
        lines.append(dict(case=name, heads=heads, head_dim=D, B=B, F=Fr, P=P, us=round(us, 2), mbytes=round(nbytes / 1e6, 1),
                          gbps=round(nbytes / us / 1e3, 1), dist_to_first_of_head_dim=dist))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
