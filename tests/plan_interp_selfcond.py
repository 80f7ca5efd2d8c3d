"""The plan interpreter with LINCOMB restated for ABI 13 (ImagenLincombParams.thr1_out / thr3_out), and the loaders of the self-conditioning
fixtures (tests/golden/selfcond_*.pt, tools/make_selfcond_golden.py).

tests/plan_interp.py states the contract of before ABI 13; this subclass adds the two optional outputs as include/imagen_hip.h states them —
each receives thr(t1, q1) / thr(t3, q3), the value that enters the sum, whatever its weight and whatever the mask — and is the same function
when both are NULL.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import os

import torch

from plan_interp import Interpreter, K, f32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class InterpreterSC(Interpreter):
    def lincomb(self, p):
        m = self.mem
        n = p.B * p.n_per_sample

        def thr(t, q):
            if p.thr_mode == 1:
                s = (m.view(q, f32)[: p.B].clamp(min=1.0) if q else torch.ones(p.B)).reshape(p.B, 1)
                return (t.reshape(p.B, -1).clamp(-s, s) / s).reshape(-1)
            return t.clamp(-1.0, 1.0) if p.thr_mode == 2 else t.clone()

        outs = []
        for dst, src, q in ((p.thr1_out, p.t1, p.q1), (p.thr3_out, p.t3, p.q3)):
            if dst:
                assert src, "thr1_out needs t1, thr3_out needs t3"
                outs.append((dst, thr(m.view(src, f32)[:n], q)))     # formed from the inputs BEFORE anything is written
        super().lincomb(p)
        for dst, v in outs:
            m.view(dst, f32)[:n].copy_(v)


InterpreterSC.DISPATCH = {**Interpreter.DISPATCH, K["IMAGEN_OP_LINCOMB"]: InterpreterSC.lincomb}


# ------------------------------------------------------------------------------------------------ fixtures

def unpack_state_dict(spec):
    """{key: fp32 tensor} in state_dict order from a unet record (one flat fp16 tensor + the ordered (key, shape) index)."""
    sd, at = {}, 0
    for key, shape in spec["index"]:
        n = 1
        for d in shape:
            n *= d
        sd[key] = spec["flat"][at:at + n].float().reshape(shape)
        at += n
    assert at == spec["flat"].numel()
    return sd


def _load(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


_cache = {}


def image_fixture():
    """(runs record, [unet record per stage]) of fixture (b): ElucidatedImagen over two Unet(self_cond=True) stages."""
    if "image" not in _cache:
        g = _load("selfcond_image_runs.pt")
        _cache["image"] = (g, [_load(n) for n in g["weights_from"]])
    return _cache["image"]


def video_fixture():
    """(record, unet record) of fixtures (a) and (c): one Unet3D(self_cond=True)."""
    if "video" not in _cache:
        g = _load("selfcond_video.pt")
        _cache["video"] = (g, _load(g["weights_from"]))
    return _cache["video"]


def image_model(device="cpu", **over):
    from imagen_pytorch_amd import ElucidatedImagen, Unet

    g, specs = image_fixture()
    unets = [Unet(**{**s["kwargs"], **over}).eval() for s in specs]
    model = ElucidatedImagen(tuple(unets), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["hparams"])
    if str(device) != "cpu":
        model = model.to(device)
    for u, s in zip(model.unets, specs):
        u.load_state_dict(unpack_state_dict(s))
    return model.eval()


def video_unet():
    from imagen_pytorch_amd import Unet3D

    _, spec = video_fixture()
    u = Unet3D(**spec["kwargs"]).eval()
    u.load_state_dict(unpack_state_dict(spec))
    return u


def video_model(kind, device="cpu"):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the one video unet."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen

    g, spec = video_fixture()
    if kind == "ddpm":
        model = Imagen((video_unet(),), image_sizes=g["image_sizes"], timesteps=g["ddpm"]["timesteps"], text_embed_dim=32, cond_drop_prob=0.1)
    else:
        model = ElucidatedImagen((video_unet(),), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["edm"]["hparams"])
    if str(device) != "cpu":
        model = model.to(device)
    model.unets[0].load_state_dict(unpack_state_dict(spec))
    return model.eval()


def nerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm())
