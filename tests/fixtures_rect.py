"""Rectangular images (H != W): the loaders of tests/golden/rect_*.pt (tools/make_rect_golden.py).  TEST INFRASTRUCTURE, never imported by
the product."""
from __future__ import annotations

import torch

from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401

FORWARD_UNETS = ("tiny", "memeff", "comb", "linx", "four", "four_sr")
RUNS = ("ddpm", "ddpm_tall", "neg", "init_skip", "inpaint", "edm")
FORWARD_BAR = 1e-2                               # tests/test_plan_interp.py
SAMPLE_BAR = {"ddpm": 2e-2, "edm": 3e-2}         # tests/test_sample_cpu_replay.py, tests/test_model_gpu.py


def crop(t):
    """The centre square of the last two axes."""
    H, W = t.shape[-2:]
    s = min(H, W)
    y0, x0 = (H - s) // 2, (W - s) // 2
    return t[..., y0:y0 + s, x0:x0 + s]


def unet_record(name):
    """(kwargs, state_dict): the flat fp16 parameters lie in `parts` files."""
    head = load(f"rect_w_{name}_0.pt")
    flat = torch.cat([load(f"rect_w_{name}_{k}.pt")["flat"] for k in range(head["parts"])])
    return head["kwargs"], unpack_state_dict(dict(index=head["index"], flat=flat))


def unet(name, device="cpu"):
    from imagen_pytorch_amd import Unet

    kw, sd = unet_record(name)
    u = Unet(**kw).eval()
    u.load_state_dict(sd)
    return u.to(device) if str(device) != "cpu" else u


def forward_records(name):
    """{"HxW": record} of one unet."""
    return load(f"rect_forward_{name}.pt")["records"]


def forward_cases():
    return [(n, k) for n in FORWARD_UNETS for k in forward_records(n)]


def low_kw(f, device="cpu"):
    return {k: f[k].to(device) for k in ("lowres_cond_img", "lowres_noise_times") if k in f}


def sample_fixture(run):
    return load(f"rect_sample_{run}.pt")


def sample_model(kind, device="cpu"):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the two stages of the fixtures, built at the SQUARE image_sizes (16, 32): the
    rectangular shapes come in per call (image_shapes)."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen

    g = sample_fixture("ddpm")
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


def run_kwargs(run, device="cpu"):
    """(fixture, the sample() keywords of the recorded run with its draws injected)."""
    g = sample_fixture(run)
    r = g["run"]
    kw = dict(text_embeds=g["text_embeds"].to(device), cond_scale=r.get("cond_scale", g["cond_scale"]), use_tqdm=False, image_shapes=r["image_shapes"],
              noise_fn=lambda t, shape: r["noise"][t].to(device), return_all_unet_outputs=True)
    for k in ("negative_text_embeds", "negative_text_masks", "init_images", "inpaint_images", "inpaint_masks"):
        if k in r:
            kw[k] = r[k].to(device)
    for k in ("skip_steps", "inpaint_resample_times"):
        if k in r:
            kw[k] = r[k]
    return g, kw
