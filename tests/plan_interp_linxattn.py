"""The plan interpreter with the two op kinds of ABI 14 (LINCTX, LINEAR_XATTN: LinearCrossAttention, Unet(use_linear_cross_attn=...)), the
fp32 / fp64 restatements of LinearCrossAttention.forward (ip.py:836-874) and the loaders of tests/golden/linxattn_*.pt
(tools/make_linear_xattn_golden.py).

tests/plan_interp.py and tests/plan_interp_selfcond.py state the contracts of before ABI 14; this subclass adds the two new ones as
include/imagen_hip.h states them (fp16 storage, fp32 arithmetic) and changes nothing else.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import ctypes
import os

import torch

from plan_interp import K, f16, f32
from plan_interp_selfcond import GOLDEN, InterpreterSC, nerr, unpack_state_dict  # noqa: F401

from imagen_pytorch_amd import _abi


class InterpreterLX(InterpreterSC):
    def linctx(self, p):
        m = self.mem
        st = _abi.STRUCTS["ImagenLinCtxJob"]
        for i in range(p.n):
            j = st.from_address(p.jobs + i * ctypes.sizeof(st))
            D, H = j.head_dim, j.heads
            assert D in (32, 64) and j.R * H <= p.max_bh
            rows = m.strided(j.kv, f16, (j.R, j.J, 2 * H * D), (j.kv_bs, j.kv_rs, 1)).float()
            k = rows[..., :H * D].reshape(j.R, j.J, H, D)
            v = rows[..., H * D:].reshape(j.R, j.J, H, D)
            M = torch.einsum("rjha,rjhb->rhab", k.softmax(dim=1), v)
            m.view(j.M, f32)[:M.numel()].copy_(M.reshape(-1))

    def linear_xattn(self, p):
        m = self.mem
        D, H, N = p.head_dim, p.heads, p.rows
        assert D in (32, 64)
        q = m.strided(p.q, f16, (p.R, N, H, D), (N * p.ld_q, p.ld_q, D, 1)).float()
        M = m.view(p.M, f32)[:p.R * H * D * D].reshape(p.R, H, D, D)
        o = 8.0 * torch.einsum("rnha,rhab->rnhb", q.softmax(dim=-1), M)
        m.strided(p.o, f16, (p.R, N, H, D), (N * p.ld_o, p.ld_o, D, 1)).copy_(o.half())


InterpreterLX.DISPATCH = {**InterpreterSC.DISPATCH, K["IMAGEN_OP_LINCTX"]: InterpreterLX.linctx, K["IMAGEN_OP_LINEAR_XATTN"]: InterpreterLX.linear_xattn}


# ------------------------------------------------------------------------------------------------ restatements

def linear_cross_attention(sd, prefix, x, context, heads, dtype=torch.float32):
    """LinearCrossAttention.forward (ip.py:836-874) without a mask, from the state_dict entries under `prefix`; x (b, n, dim),
    context (b, j, cond_dim)."""
    w = lambda k: sd[prefix + k].to(dtype)
    x, context = x.to(dtype), context.to(dtype)

    def ln(t, g):     # ip.py:331-349 LayerNorm: gain only, eps 1e-5 (1e-3 for fp16), biased variance
        var = t.var(dim=-1, unbiased=False, keepdim=True)
        return (t - t.mean(dim=-1, keepdim=True)) * (var + 1e-5).rsqrt() * g

    b, n, _ = x.shape
    q = ln(x, w("norm.g")) @ w("to_q.weight").t()
    k, v = (context @ w("to_kv.weight").t()).chunk(2, dim=-1)
    split = lambda t: t.reshape(b, t.shape[1], heads, -1).permute(0, 2, 1, 3)          # b h n d
    q, k, v = split(q), split(k), split(v)
    nk, nv = w("null_kv")[0], w("null_kv")[1]
    k = torch.cat((nk.expand(b, heads, 1, -1), k), dim=2)
    v = torch.cat((nv.expand(b, heads, 1, -1), v), dim=2)
    q = q.softmax(dim=-1) * 8.0
    k = k.softmax(dim=-2)
    M = torch.einsum("bhnd,bhne->bhde", k, v)
    out = torch.einsum("bhnd,bhde->bhne", q, M).permute(0, 2, 1, 3).reshape(b, n, -1)
    return ln(out @ w("to_out.0.weight").t(), w("to_out.1.g"))


def linctx_fp64(kv, heads, D):
    """M of LINCTX in fp64 from fp16 rows kv [R, J, 2 * heads * D]."""
    R, J, _ = kv.shape
    k = kv[..., :heads * D].double().reshape(R, J, heads, D)
    v = kv[..., heads * D:].double().reshape(R, J, heads, D)
    return torch.einsum("rjha,rjhb->rhab", k.softmax(dim=1), v)


def linear_xattn_fp64(q, M, heads, D):
    """o of LINEAR_XATTN in fp64 from fp16 q [R, N, heads * D] and M [R, heads, D, D]."""
    R, N, _ = q.shape
    return (8.0 * torch.einsum("rnha,rhab->rnhb", q.double().reshape(R, N, heads, D).softmax(dim=-1), M.double())).reshape(R, N, heads * D)


# ------------------------------------------------------------------------------------------------ fixtures

_cache = {}


def _load(name):
    if name not in _cache:
        _cache[name] = torch.load(os.path.join(GOLDEN, name), weights_only=False)
    return _cache[name]


def unet_record(name):
    """The record of `lin64` | `lin32` | `twin`: kwargs, forward inputs and outputs; and its state_dict (the twin's is lin64's)."""
    rec = _load("linxattn_unet_hd32.pt" if name == "lin32" else "linxattn_unet.pt")["models"][name]
    src = _load("linxattn_unet.pt")["models"][rec["weights_of"]] if "weights_of" in rec else rec
    return rec, unpack_state_dict(src)


def unet(name, device="cpu"):
    from imagen_pytorch_amd import Unet

    rec, sd = unet_record(name)
    u = Unet(**rec["kwargs"]).eval()
    u.load_state_dict(sd)
    return u.to(device) if str(device) != "cpu" else u


def sample_fixture():
    return _load("linxattn_sample.pt")


def sample_model(kind, name="lin64", device="cpu"):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the one unet `name`."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen

    g = sample_fixture()
    u = unet(name)
    if kind == "ddpm":
        model = Imagen((u,), image_sizes=g["image_sizes"], timesteps=g["timesteps"], text_embed_dim=32, cond_drop_prob=0.1)
    else:
        model = ElucidatedImagen((u,), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["hparams"])
    if str(device) != "cpu":
        model = model.to(device)
    model.unets[0].load_state_dict(unet_record(name)[1])
    return model.eval()


def run_unet(u, f, interp=InterpreterLX):
    """One CFG pair (cond rows, then null rows) of `u` on the forward record f: the dry-run launch lists of engine.UnetEngine executed by
    `interp`.  Returns (out_cond, out_null) and the engine."""
    from imagen_pytorch_amd.engine import UnetEngine

    B, S = f["x"].shape[0], f["x"].shape[-1]
    eng = UnetEngine(u, 2 * B, B, S, "cpu", dry=True)
    keep = torch.tensor([True] * B + [False] * B)
    eng.set_conditioning(text_embeds=f["text_embeds"], text_mask=f["text_mask"], keep=keep, lowres_noise_times=None)
    it = interp()
    for buf in (eng.x_in, eng.times, eng.lowres_times, eng.out, eng.keep_u8, eng.src_idx, eng.arange_idx, eng.t_const.t):
        it.mem.register(buf)
    it.run(eng._static_plans[f["text_embeds"].shape[1]][0])
    eng.x_in.copy_(f["x"])
    eng.times.copy_(f["time"].repeat(2))
    it.run(eng.step_plan)
    out = eng.out.float().clone()
    return out[:B], out[B:], eng
