"""Clips of 33 .. 128 frames (ABI 15: TEMPORAL_ATTENTION takes F <= 128): the contract restated in fp64 for the kernel tests, the plan
interpreter for such plans, and the loaders of the long-clip fixtures (tests/golden/longclip_*.pt, tools/make_longclip_golden.py).

The TEMPORAL_ATTENTION contracts of tests/plan_interp.py (64-wide heads) and tests/plan_interp_hd.py (head dim D) are written over the
whole key axis and hold no frame bound, so the interpreter of long-clip plans is InterpreterHD as it stands; `temporal_attention_fp64` is
the same statement of include/imagen_hip.h on plain tensors, in fp64, which is what the kernel is measured against.
TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from plan_interp_hd import InterpreterHD, run_unet3d  # noqa: F401
from plan_interp_selfcond import nerr, unpack_state_dict  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class InterpreterLong(InterpreterHD):
    """(nothing to restate: the contract of InterpreterHD.temporal_attention is generic in F)"""


def temporal_attention_fp64(qkv, null_kv, q_scale, k_scale, bias, *, heads, D, causal, scale):
    """o [B, F, P, heads * D] in fp64 from fp16 rows qkv [B, F, P, heads * D + 2 D] (q | k | v), fp32 null_kv [2, D], q_scale / k_scale
    [D] and bias [heads, F, F + 1] (column 0 = the null key): include/imagen_hip.h, TEMPORAL_ATTENTION."""
    B, Fr, P, _ = qkv.shape
    rows = qkv.double()
    q = rows[..., :heads * D].reshape(B, Fr, P, heads, D).permute(0, 2, 3, 1, 4)                       # b p h i d
    k, v = rows[..., heads * D:heads * D + D].permute(0, 2, 1, 3), rows[..., heads * D + D:].permute(0, 2, 1, 3)   # b p j d
    nkv = null_kv.double().reshape(2, D)
    k = torch.cat((nkv[0].expand(B, P, 1, D), k), dim=2)
    v = torch.cat((nkv[1].expand(B, P, 1, D), v), dim=2)
    qh = F.normalize(q, dim=-1, eps=1e-12) * q_scale.double() * scale
    kh = F.normalize(k, dim=-1, eps=1e-12) * k_scale.double()
    sim = torch.einsum("bphid,bpjd->bphij", qh, kh) + bias.double()
    if causal:
        sim = sim.masked_fill(torch.ones(Fr, Fr + 1, dtype=torch.bool).triu(2), -torch.finfo(sim.dtype).max)
    o = torch.einsum("bphij,bpjd->bphid", sim.softmax(-1), v)
    return o.permute(0, 3, 1, 2, 4).reshape(B, Fr, P, heads * D)


# ------------------------------------------------------------------------------------------------ fixtures

_cache = {}


def _load(name):
    if name not in _cache:
        _cache[name] = torch.load(os.path.join(GOLDEN, name), weights_only=False)
    return _cache[name]


def unet_record(name):
    """(forward record, kwargs, state_dict) of `long` | `long32` | `twin` (long's weights on the first 16 frames of long's input)."""
    rec = _load({"long": "longclip_long.pt", "long32": "longclip_long32.pt", "twin": "longclip_twin.pt"}[name])
    first, second = (_load(n) for n in rec["weights_from"])          # the flat fp16 tensor in two files (each under 1 MiB)
    spec = dict(first, flat=torch.cat((first["flat"], second["flat"])))
    f = dict(rec["forward"])
    x = _load("longclip_long.pt")["forward"]["x"].float()               # one input for all three (stored once, fp16-exact)
    f["x"] = x[:, :, :f["frames"]].contiguous()
    return f, spec["kwargs"], unpack_state_dict(spec)


def unet(name, device="cpu"):
    from imagen_pytorch_amd import Unet3D

    _, kwargs, sd = unet_record(name)
    u = Unet3D(**kwargs).eval()
    u.load_state_dict(sd)
    return u.to(device) if str(device) != "cpu" else u


def sample_fixture():
    return _load("longclip_sample.pt")


def sample_model(kind, device="cpu"):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the one `long` unet."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen

    g = sample_fixture()
    u = unet("long")
    kw = g["model_kwargs"][kind]          # centred outputs, the clip-wide threshold at the median (tools/make_longclip_golden.py)
    if kind == "ddpm":
        model = Imagen((u,), image_sizes=g["image_sizes"], timesteps=g["ddpm"]["timesteps"], text_embed_dim=32, cond_drop_prob=0.1, **kw)
    else:
        model = ElucidatedImagen((u,), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["edm"]["hparams"], **kw)
    if str(device) != "cpu":
        model = model.to(device)
    model.unets[0].load_state_dict(unet_record("long")[2])
    return model.eval()


def launch_list(eng, text_len):
    """[[kind, label], ...] of the static and the step plan of an engine (the form of tests/golden/*_launch_list_*.json)."""
    return {"static": [[int(k), l] for k, _, l in eng._static_plans[text_len][0].ops], "step": [[int(k), l] for k, _, l in eng.step_plan.ops]}
