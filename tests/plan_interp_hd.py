"""The plan interpreter with TEMPORAL_ATTENTION restated for a head dim D (ABI 12: ImagenTemporalAttentionParams.head_dim, 0 means 64).

tests/plan_interp.py states the contract of before ABI 12 (64-wide heads); this subclass states the contract of include/imagen_hip.h as it
is now — qkv rows hold q (heads*D) | k (D) | v (D), null_kv is [2][D], q_scale / k_scale are [D] — and is the same function at D = 64
(tests/test_video_headdim32.py runs an existing head-dim-64 video plan through both and compares the outputs bit for bit).
TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from plan_interp import Interpreter, K, f16, f32


class InterpreterHD(Interpreter):
    def temporal_attention(self, p):
        m = self.mem
        D = p.head_dim or 64
        assert D in (32, 64), D
        Fr, P, H = p.F, p.P, p.heads
        rows = m.strided(p.qkv, f16, (p.B, Fr, P, H * D + 2 * D), (Fr * P * p.ld, P * p.ld, p.ld, 1)).float()
        q = rows[..., :H * D].reshape(p.B, Fr, P, H, D).permute(0, 2, 3, 1, 4)          # b p h i d
        k, v = rows[..., H * D:H * D + D].permute(0, 2, 1, 3), rows[..., H * D + D:].permute(0, 2, 1, 3)   # b p j d
        nkv = m.view(p.null_kv, f32)[:2 * D].reshape(2, D)
        k = torch.cat((nkv[0].expand(p.B, P, 1, D), k), dim=2)
        v = torch.cat((nkv[1].expand(p.B, P, 1, D), v), dim=2)
        qh = F.normalize(q, dim=-1, eps=1e-12) * m.view(p.q_scale, f32)[:D] * p.scale
        kh = F.normalize(k, dim=-1, eps=1e-12) * m.view(p.k_scale, f32)[:D]
        sim = torch.einsum("bphid,bpjd->bphij", qh, kh) + m.view(p.bias, f32)[:H * Fr * (Fr + 1)].reshape(H, Fr, Fr + 1)
        if p.causal:
            sim = sim.masked_fill(torch.ones(Fr, Fr + 1, dtype=torch.bool).triu(2), -torch.finfo(sim.dtype).max)
        o = torch.einsum("bphij,bpjd->bphid", sim.softmax(-1), v)                       # b p h i d
        o = o.permute(0, 3, 1, 2, 4).reshape(p.B, Fr, P, H * D)
        m.strided(p.o, f16, (p.B, Fr, P, H * D), (Fr * P * p.ld_o, P * p.ld_o, p.ld_o, 1)).copy_(o.half())


InterpreterHD.DISPATCH = {**Interpreter.DISPATCH, K["IMAGEN_OP_TEMPORAL_ATTENTION"]: InterpreterHD.temporal_attention}


def run_unet3d(unet, x, t, text_embeds, text_mask=None, interp=InterpreterHD):
    """One CFG pair (cond rows, then null rows) of `unet` on the clip batch x (B, C, F, S, S) at times t: the dry-run launch lists of
    engine3d.UnetEngine3D executed by `interp`.  Returns (out_cond, out_null) as (B, C, F, S, S) fp32, and the engine."""
    from imagen_pytorch_amd.engine3d import UnetEngine3D

    B, _, Fr, S, _ = x.shape
    eng = UnetEngine3D(unet, 2 * B, B, Fr, S, "cpu", dry=True)
    keep = torch.tensor([True] * B + [False] * B)
    eng.set_conditioning(text_embeds=text_embeds, text_mask=text_mask, keep=keep, lowres_noise_times=None)
    it = interp()
    for buf in (eng.x_in, eng.times, eng.lowres_times, eng.out, eng.keep_u8, eng.src_idx, eng.arange_idx, eng.t_const.t):
        it.mem.register(buf)
    it.run(eng._static_plans[text_embeds.shape[1]][0])
    eng.x_in.copy_(x.permute(0, 2, 1, 3, 4))
    eng.times.copy_(t.repeat(2))
    it.run(eng.step_plan)
    out = eng.out.permute(0, 2, 1, 3, 4).float().clone()
    return out[:B], out[B:], eng
