"""Linear cross-attention (Unet(use_linear_cross_attn=...)): the fp32 / fp64 restatement of LinearCrossAttention.forward (ip.py:836-874)
and the loaders of tests/golden/linxattn_*.pt (tools/make_linear_xattn_golden.py).  The contracts of the two op kinds, LINCTX and
LINEAR_XATTN, are in tests/plan_interp.py.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import torch

from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401


# ------------------------------------------------------------------------------------------------ restatement

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


# ------------------------------------------------------------------------------------------------ fixtures

def unet_record(name):
    """The record of `lin64` | `lin32` | `twin`: kwargs, forward inputs and outputs; and its state_dict (the twin's is lin64's)."""
    rec = load("linxattn_unet_hd32.pt" if name == "lin32" else "linxattn_unet.pt")["models"][name]
    src = load("linxattn_unet.pt")["models"][rec["weights_of"]] if "weights_of" in rec else rec
    return rec, unpack_state_dict(src)


def unet(name, device="cpu"):
    from imagen_pytorch_amd import Unet

    rec, sd = unet_record(name)
    u = Unet(**rec["kwargs"]).eval()
    u.load_state_dict(sd)
    return u.to(device) if str(device) != "cpu" else u


def sample_fixture():
    return load("linxattn_sample.pt")


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

