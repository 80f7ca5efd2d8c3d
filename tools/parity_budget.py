"""CPU experiment (test infrastructure): where does the whole-Unet distance to the fp32 oracle come from?

Runs the Unet planner's launch list through the plan interpreter (tests/plan_interp.py: every op kind of include/imagen_hip.h restated
from its contract, fp16 storage, fp32 arithmetic — the rounding points of the HIP path without its kernels; so any plan the planners
emit can be replayed, head-dim-32 temporal attention included; a linear cross-attention unet still has no oracle to be priced against)
against the oracle, with switches that keep chosen tensors at higher precision:

  --exact-weights REGEX   the conv / GEMM launches whose label matches read the UNROUNDED fp32 weight (what a split-precision weight gives a
                          launch: ops.pack_weight(split=True)) — prices a planner policy before it is written.  Round 5, BASELINE C5:
                          '^(final_conv$|final_res_block\.block1$)' 1.008e-3 -> 0.970e-3 (cond), then engine3d.SPLIT_OUTPUT_STAGE; '.' (every
                          launch) 0.863e-3; '^(to_time|time_mlps)' nothing.  Deltas under ~3 % are inside what another realisation of the
                          rounding noise does to the figure.

    python tools/parity_budget.py [--config u1|u2|hd32|memeff|c5|c5hd32] [--size 64] [--seeds 0 1 2] [--exact-weights REGEX]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

README_U1 = dict(dim=32, cond_dim=512, dim_mults=(1, 2, 4, 8), num_resnet_blocks=3, layer_attns=(False, True, True, True),
                 layer_cross_attns=(False, True, True, True))
README_U2 = dict(dim=32, cond_dim=512, dim_mults=(1, 2, 4, 8), num_resnet_blocks=(2, 4, 8, 8), layer_attns=(False, False, False, True),
                 layer_cross_attns=(False, False, False, True), lowres_cond=True)
MEMEFF = dict(dim=32, cond_dim=64, dim_mults=(1, 2, 4), num_resnet_blocks=(1, 2, 2), layer_attns=(False, False, True),
              layer_cross_attns=(False, True, True), memory_efficient=True, lowres_cond=True, attn_heads=4)
HD32 = dict(README_U1, attn_dim_head=32, attn_heads=16)
CONFIGS = dict(u1=README_U1, u2=README_U2, memeff=MEMEFF, hd32=HD32)
C5_HEADS = dict(c5={}, c5hd32=dict(attn_dim_head=32, attn_heads=16))      # (c5hd32: the config-default heads of Unet3DConfig)


def nerr(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def case(kw, S, B, seed=0):
    from imagen_pytorch_amd import Unet
    torch.manual_seed(seed)
    u = Unet(**kw).eval()
    torch.nn.init.normal_(u.final_conv.weight, std=0.05)
    torch.nn.init.normal_(u.final_conv.bias, std=0.05)
    sd = {k: v.clone() for k, v in u.state_dict().items()}
    x, t = torch.randn(B, 3, S, S), torch.tensor([0.3, -1.2, 0.9, 2.0][:B])
    te = torch.randn(B, 24, kw.get("text_embed_dim", 768))
    mask = torch.ones(B, 24, dtype=torch.bool)
    mask[1, 18:] = False
    extra = dict(lowres_cond_img=torch.randn(B, 3, S, S), lowres_noise_times=torch.full((B,), 0.5)) if kw.get("lowres_cond") else {}
    return u, sd, x, t, te, mask, extra


def run_interp(u, x, t, te, mask, extra, S, B, interp_cls):
    from imagen_pytorch_amd.engine import UnetEngine
    from plan_interp import run_engine
    out_c, out_n, eng, _ = run_engine(UnetEngine(u, 2 * B, B, S, "cpu", dry=True), x, t, te, mask, it=interp_cls(), **extra)
    return torch.cat((out_c, out_n)), eng


def exact_weight_interpreter(regex: str):
    """An Interpreter whose IGEMM launches with a label matching `regex` use the fp32 weight as given to ops.pack_weight (a split-precision
    weight [hi | lo] read against the input twice is the same product to ~2^-22); ops.pack_weight is wrapped to remember it."""
    import re
    from imagen_pytorch_amd import ops
    from plan_interp import Interpreter

    exact = {}
    pack = ops.pack_weight

    def pack_weight(w, bias, device, in_scale=None, G=None, split=False):
        pw = pack(w, bias, device, in_scale=in_scale, G=G, split=split)
        ww = w.detach().float().cpu()
        if ww.ndim == 2:
            ww = ww[:, :, None, None]
        if in_scale is not None:
            ww = ww * in_scale.detach().float().cpu()[None, : ww.shape[1], None, None]
        exact[pw.w.data_ptr()] = torch.cat((ww, torch.zeros_like(ww)), 1) if split else ww    # (split: the input comes twice, [W | 0] . [x | x] = W . x)
        return pw
    ops.pack_weight = pack_weight
    pat = re.compile(regex)

    class Exact(Interpreter):
        def run(self, plan):
            self.mem.register_plan(plan)
            for kind, p, label in plan.ops:
                fn = self.DISPATCH[kind]
                if fn is Interpreter.igemm and pat.search(label):
                    saved = ops.REFERENCE_WEIGHTS[p.w]
                    ops.REFERENCE_WEIGHTS[p.w] = (exact[p.w], saved[1])
                    try:
                        fn(self, p)
                    finally:
                        ops.REFERENCE_WEIGHTS[p.w] = saved
                else:
                    fn(self, p)
                self.trace.append(label)
    return Exact


def c5_case(interp_cls, name="c5"):
    """BASELINE C5's denoiser (Unet3D(dim 64), one 16 x 64 x 64 clip, the sampler's 2-row plan) through the interpreter, against the oracle: the
    case of tests/test_video_gpu.py::test_unet3d_forward_vs_oracle_c5 (c5hd32: ..._c5_head_dim_32)."""
    from imagen_pytorch_amd import Unet3D
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from oracle import unet3d_oracle as u3
    from plan_interp import run_engine
    from test_video_gpu import _derandomise_unet3d as derandomise_unet3d   # (the C5 test's own weights: dirac + dense temporal convs)

    kw = dict(dim=64, dim_mults=(1, 2, 4, 8), **C5_HEADS[name])
    torch.manual_seed(0)
    u = Unet3D(**kw).eval()
    derandomise_unet3d(u)
    sd = {k: v.clone() for k, v in u.state_dict().items()}
    x, t = torch.randn(1, 3, 16, 64, 64), torch.tensor([0.3])
    te = torch.randn(1, 24, 768)
    mask = torch.ones(1, 24, dtype=torch.bool)
    mask[0, 19:] = False
    with torch.no_grad():
        ref = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, text_mask=mask)
        ref_null = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, text_mask=mask, cond_drop_prob=1.0)
    out_c, out_n, eng, _ = run_engine(UnetEngine3D(u, 2, 1, 16, 64, "cpu", dry=True), x, t, te, mask, it=interp_cls())
    print(f"{name} Unet3D(dim 64) 16x64x64, plan through the interpreter: cond {nerr(out_c, ref):.3e} null {nerr(out_n, ref_null):.3e}  ({len(eng.step_plan.ops)} launches)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="u1")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seeds", type=int, nargs="*", default=[0], help="weight / input seeds (0 = the GPU test's case)")
    ap.add_argument("--exact-weights", default=None, metavar="REGEX", help="launch labels that read the unrounded fp32 weight")
    args = ap.parse_args()
    from imagen_pytorch_amd import ops
    from oracle import unet_oracle as uo
    from plan_interp import Interpreter
    ops.KEEP_REFERENCE_WEIGHTS = True
    if args.exact_weights:
        Interpreter = exact_weight_interpreter(args.exact_weights)
    if args.config in C5_HEADS:
        c5_case(Interpreter, args.config)
        return
    kw, S, B = CONFIGS[args.config], args.size, args.batch
    for seed in args.seeds:
        u, sd, x, t, te, mask, extra = case(kw, S, B, seed)
        with torch.no_grad():
            ref = uo.unet_forward(sd, kw, x, t, text_embeds=te, text_mask=mask, **extra)
            ref_null = uo.unet_forward(sd, kw, x, t, text_embeds=te, text_mask=mask, cond_drop_prob=1.0, **extra)
            r16 = lambda v: v.half().float() if torch.is_tensor(v) and v.is_floating_point() else v
            sd16 = {k: r16(v) for k, v in sd.items()}
            ex16 = {k: r16(v) for k, v in extra.items()}
            calib = nerr(uo.unet_forward(sd16, kw, r16(x), t, text_embeds=r16(te), text_mask=mask, cond_drop_prob=1.0, **ex16), ref_null)
        out, eng = run_interp(u, x, t, te, mask, extra, S, B, Interpreter)
        print(f"{args.config}@{S} B{B} seed {seed}: fp16 params + inputs only (null) {calib:.3e};  plan through the interpreter: cond {nerr(out[:B], ref):.3e} "
              f"null {nerr(out[B:], ref_null):.3e}", flush=True)
        ops.REFERENCE_WEIGHTS.clear()


if __name__ == "__main__":
    main()
