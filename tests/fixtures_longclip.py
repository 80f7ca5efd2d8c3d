"""Clips of 33 .. 128 frames: the loaders of the long-clip fixtures (tests/golden/longclip_*.pt, tools/make_longclip_golden.py).  The
TEMPORAL_ATTENTION contract, which holds no frame bound, is in tests/plan_interp.py.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import torch

from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401


def unet_record(name):
    """(forward record, kwargs, state_dict) of `long` | `long32` | `twin` (long's weights on the first 16 frames of long's input)."""
    rec = load({"long": "longclip_long.pt", "long32": "longclip_long32.pt", "twin": "longclip_twin.pt"}[name])
    first, second = (load(n) for n in rec["weights_from"])          # the flat fp16 tensor in two files (each under 1 MiB)
    spec = dict(first, flat=torch.cat((first["flat"], second["flat"])))
    f = dict(rec["forward"])
    x = load("longclip_long.pt")["forward"]["x"].float()               # one input for all three (stored once, fp16-exact)
    f["x"] = x[:, :, :f["frames"]].contiguous()
    return f, spec["kwargs"], unpack_state_dict(spec)


def unet(name, device="cpu"):
    from imagen_pytorch_amd import Unet3D

    _, kwargs, sd = unet_record(name)
    u = Unet3D(**kwargs).eval()
    u.load_state_dict(sd)
    return u.to(device) if str(device) != "cpu" else u


def sample_fixture():
    return load("longclip_sample.pt")


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
