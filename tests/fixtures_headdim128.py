"""Attention head dim 128 (Unet(attn_dim_head=128)): the loaders of tests/golden/headdim128_*.pt (tools/make_headdim128_golden.py), the
plan interpreter restated for a head dim the params carry (tests/plan_interp.py reads `head_dim` as 32-or-else-64 in five contracts), and
the fp64 contracts of the attention-side kernels over plain tensors.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn.functional as F

from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401

f16, f32 = torch.float16, torch.float32


# ------------------------------------------------------------------------------------------------ fixtures

def unet_record(name):
    """(kwargs, state_dict) of `hd128` | `hd128_lin` | `sr`: the flat fp16 parameters lie in two files."""
    a, b = load(f"headdim128_w_{name}_0.pt"), load(f"headdim128_w_{name}_1.pt")
    return a["kwargs"], unpack_state_dict(dict(index=a["index"], flat=torch.cat((a["flat"], b["flat"]))))


def forward_record(name):
    return load("headdim128_forward.pt")["models"][name]


def unet(name, device="cpu"):
    from imagen_pytorch_amd import Unet

    kw, sd = unet_record(name)
    u = Unet(**kw).eval()
    u.load_state_dict(sd)
    return u.to(device) if str(device) != "cpu" else u


def sample_fixture():
    return load("headdim128_sample.pt")


def sample_model(kind, device="cpu"):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the two stages of the fixture."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen

    g = sample_fixture()
    us = [unet(n) for n in g["unets"]]
    if kind == "ddpm":
        model = Imagen(us, image_sizes=g["image_sizes"], timesteps=g["timesteps"], text_embed_dim=32, cond_drop_prob=0.1)
    else:
        model = ElucidatedImagen(us, image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["hparams"])
    if str(device) != "cpu":
        model = model.to(device)
    for u, n in zip(model.unets, g["unets"]):
        u.load_state_dict(unet_record(n)[1])
    return model.eval()


# ------------------------------------------------------------------------------------------------ contracts (plain tensors, any dtype)

def attention_contract(q, k, v, q_scale=None, q_mult=1.0, dtype=torch.float64):
    """ATTENTION: q [B, H, N, D], k / v [B, H, J, D] (k already K^: l2-normalised * k_scale, fp16).  With q_scale the q rows are raw and the
    kernel's fused QNORM applies (l2norm * q_scale * q_mult, rounded to fp16); the logits are in log2 units."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    if q_scale is not None:
        q = (F.normalize(q, dim=-1, eps=1e-12) * q_scale.to(dtype) * q_mult).half().to(dtype)
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * math.log(2.0)
    return torch.einsum("bhij,bhjd->bhid", sim.softmax(-1), v)


def l2norm_scale_contract(x, scale, mult=1.0, dtype=torch.float64):
    """QNORM / the K^ half of KV_PREP: x [..., D] -> x / max(|x|, 1e-12) * scale * mult."""
    return F.normalize(x.to(dtype), dim=-1, eps=1e-12) * scale.to(dtype) * mult


# ------------------------------------------------------------------------------------------------ interpreter

def interpreter_class():
    """plan_interp.Interpreter with the five contracts that read a head dim restated for the value the params carry (0: 64)."""
    import plan_interp as pi
    from imagen_pytorch_amd import _abi

    K = _abi.ENUMS

    class InterpreterHD(pi.Interpreter):
        def kv_prep(self, p):
            m = self.mem
            dt = f32 if p.src_is_f32 else f16
            D = p.head_dim or 64
            sz = (p.B, p.heads, p.rows, D)
            st = (p.src_bs, p.src_hs, p.src_rs, 1)
            k = m.strided(p.k_src, dt, sz, st).float()
            v = m.strided(p.v_src, dt, sz, st).float()
            khat = F.normalize(k, dim=-1, eps=1e-12) * m.view(p.k_scale, f32)[:D]
            m.strided(p.khat + 2 * p.r0 * p.k_rs, f16, sz, (p.k_bs, p.k_hs, p.k_rs, 1)).copy_(khat.half())
            m.strided(p.vt + 2 * p.r0, f16, sz, (p.vt_bs, p.vt_hs, 1, p.vt_ds)).copy_(v.half())

        def kv_prep_multi(self, p):
            st = _abi.STRUCTS["ImagenKvPrepParams"]
            for i in range(p.n):
                self.kv_prep(st.from_address(p.jobs + i * ctypes.sizeof(st)))

        def qnorm(self, p):
            m = self.mem
            D = p.head_dim or 64
            q = m.strided(p.q, f16, (p.rows, p.heads, D), (p.ld, D, 1))
            q.copy_((F.normalize(q.float(), dim=-1, eps=1e-12) * m.view(p.q_scale, f32)[:D] * p.mult).half())

        def attention(self, p):
            m = self.mem
            D = p.head_dim or 64
            q = m.strided(p.q, f16, (p.B, p.heads, p.rows, D), (p.q_bs, p.q_hs, p.q_rs, 1))
            k = m.strided(p.k, f16, (p.B, p.heads, p.J, D), (p.k_bs, p.k_hs, p.k_rs, 1))
            v = m.strided(p.vt, f16, (p.B, p.heads, p.J, D), (p.vt_bs, p.vt_hs, 1, p.vt_ds))
            o = attention_contract(q, k, v, m.view(p.q_scale, f32)[:D] if p.q_scale else None, p.q_mult, dtype=f32)
            m.strided(p.o, f16, (p.B, p.heads, p.rows, D), (p.o_bs, p.o_hs, p.o_rs, 1)).copy_(o.half())

        def linctx(self, p):
            m = self.mem
            st = _abi.STRUCTS["ImagenLinCtxJob"]
            for i in range(p.n):
                j = st.from_address(p.jobs + i * ctypes.sizeof(st))
                D, H = j.head_dim, j.heads
                assert D in (32, 64, 128) and j.R * H <= p.max_bh
                M = pi.linctx_contract(m.strided(j.kv, f16, (j.R, j.J, 2 * H * D), (j.kv_bs, j.kv_rs, 1)), H, D)
                m.view(j.M, f32)[:M.numel()].copy_(M.reshape(-1))

        def linear_xattn(self, p):
            m = self.mem
            D, H, N = p.head_dim, p.heads, p.rows
            assert D in (32, 64, 128)
            q = m.strided(p.q, f16, (p.R, N, H * D), (N * p.ld_q, p.ld_q, 1))
            o = pi.linear_xattn_contract(q, m.view(p.M, f32)[:p.R * H * D * D].reshape(p.R, H, D, D), H, D)
            m.strided(p.o, f16, (p.R, N, H * D), (N * p.ld_o, p.ld_o, 1)).copy_(o.half())

    InterpreterHD.DISPATCH = {**pi.Interpreter.DISPATCH, K["IMAGEN_OP_KV_PREP"]: InterpreterHD.kv_prep,
                              K["IMAGEN_OP_KV_PREP_MULTI"]: InterpreterHD.kv_prep_multi, K["IMAGEN_OP_QNORM"]: InterpreterHD.qnorm,
                              K["IMAGEN_OP_ATTENTION"]: InterpreterHD.attention, K["IMAGEN_OP_LINCTX"]: InterpreterHD.linctx,
                              K["IMAGEN_OP_LINEAR_XATTN"]: InterpreterHD.linear_xattn}
    return InterpreterHD
