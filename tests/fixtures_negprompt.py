"""Negative prompts (a second text prompt on the null rows of guidance): the loaders of tests/golden/negprompt_*.pt
(tools/make_negprompt_golden.py), the fixture models, and the launch lists of the fixture stages in the form of tests/golden/negprompt_parent_launch_list_abi<N>.json.

The models: an image cascade 16^2 -> 32^2 of two dim-16 unets, dim_mults (1, 2) — stage 1 is the flag-off `twin` of
tests/golden/linxattn_unet.pt (weights stored there), stage 2 its low-res-conditioned sibling (negprompt_unet_sr.pt) — under Imagen (DDPM)
and ElucidatedImagen (Karras), and the tiny Unet3D of tests/golden/sample_tiny_video.pt as a one-stage video DDPM model at 16^2.
TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import torch

import fixtures_linxattn as lx
from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401

KW_SR = dict(dim=16, cond_dim=16, text_embed_dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True),
             layer_cross_attns=(False, True), max_text_len=16, attn_pool_num_latents=8, attn_heads=2, attn_dim_head=64, lowres_cond=True)
IMAGE_SIZES = (16, 32)
VIDEO_SIZE, VIDEO_FRAMES = 16, 4
T = 4

def forward_fixture():
    return load("negprompt_forward.pt")


def runs_fixture():
    return load("negprompt_runs.pt")


def base_kwargs():
    return dict(lx.unet_record("twin")[0]["kwargs"])


def base_unet(device="cpu"):
    return lx.unet("twin", device)


def video_kwargs():
    return dict(load("sample_tiny_video.pt")["unets"][0]["kwargs"])


def image_model(kind, device="cpu", weights=True):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the two-stage image cascade."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen, Unet

    unets = (Unet(**base_kwargs()).eval(), Unet(**KW_SR).eval())
    if kind == "ddpm":
        model = Imagen(unets, image_sizes=IMAGE_SIZES, timesteps=T, text_embed_dim=32, cond_drop_prob=0.1)
    else:
        model = ElucidatedImagen(unets, image_sizes=IMAGE_SIZES, text_embed_dim=32, cond_drop_prob=0.1, **runs_hparams())
    if str(device) != "cpu":
        model = model.to(device)
    if weights:
        model.unets[0].load_state_dict(lx.unet_record("twin")[1])
        model.unets[1].load_state_dict(unpack_state_dict(load("negprompt_unet_sr.pt")))
    return model.eval()


def runs_hparams():
    from oracle.make_golden import ELUCIDATED_HP

    return dict(ELUCIDATED_HP, num_sample_steps=T)


def video_model(device="cpu", weights=True):
    from imagen_pytorch_amd import Imagen, Unet3D

    model = Imagen((Unet3D(**video_kwargs()).eval(),), image_sizes=(VIDEO_SIZE,), timesteps=T, text_embed_dim=32, cond_drop_prob=0.1)
    if str(device) != "cpu":
        model = model.to(device)
    if weights:
        model.unets[0].load_state_dict(load("sample_tiny_video.pt")["unets"][0]["state_dict"])
    return model.eval()


def _ops(plan):
    return [[int(k), l] for k, _, l in plan.ops]


def launch_lists():
    """{name: [[kind, label], ...]} of the static plan, the per-step plan(s) and the engine's step plan of every fixture stage, built dry
    (no negative prompt anywhere): image DDPM and Karras cascades (both stages), the video DDPM stage.  Call with engine.UnetEngine and
    engine3d.UnetEngine3D patched to dry=True (tests: monkeypatch; the tool: directly)."""
    out = {}
    te = torch.zeros(2, 9, 32)
    dev = torch.device("cpu")
    for kind in ("ddpm", "edm"):
        model = image_model(kind, weights=False)
        for idx in range(2):
            st = model._stage(idx, 2, dev, cond_scale=3.0, with_text=True, inject_noise=True, sample_offset=0)
            eng = st["eng"]
            eng.set_conditioning(text_embeds=te, text_mask=None, keep=torch.tensor([True, True, False, False]),
                                 lowres_noise_times=torch.full((2,), 0.2) if idx else None)
            out[f"{kind}.{idx}.static"] = _ops(eng._static_plans[9][0])
            out[f"{kind}.{idx}.step"] = _ops(eng.step_plan)
            out[f"{kind}.{idx}.plan"] = _ops(st["plan"])
            if "last" in st:
                out[f"{kind}.{idx}.last"] = _ops(st["last"])
    model = video_model(weights=False)
    st = model._stage(0, 2, dev, cond_scale=3.0, with_text=True, inject_noise=True, sample_offset=0, frames=VIDEO_FRAMES)
    eng = st["eng"]
    eng.set_conditioning(text_embeds=te, text_mask=None, keep=torch.tensor([True, True, False, False]), lowres_noise_times=None)
    out["video.0.static"] = _ops(eng._static_plans[9][0])
    out["video.0.step"] = _ops(eng.step_plan)
    out["video.0.plan"] = _ops(st["plan"])
    return out
