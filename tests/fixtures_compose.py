"""Composed prompts of Imagen.sample (compose=[...], compose_mask=): a plain fp32 sampling loop over the oracle's K + 1 forwards per step — one
per prompt and the null (or negative-prompt) one — combined as include/imagen_hip.h states for COMPOSE_X0,

    out = nul + sum_k  w_k * m_k(pixel) * (cond_k - nul)          k = 0 .. K - 1, ascending

followed by the x0 expression, the dynamic threshold and the restated solver row of tests/fixtures_solver.py; the settings of the recorded runs
and the loader of tests/golden/compose_runs.pt (tools/make_compose_golden.py).  The same tiny cascade as tests/fixtures_guide.py (16^2 -> 32^2,
dim 8, text width 32), the same STEPS.  TEST INFRASTRUCTURE, never imported by the product.

The weights that were used: the main prompt at COND_SCALE = 7.5 (the twin's); the further prompts of the cascade runs at 15 .. 60 with their
embeddings scaled by 4 (k2: 40; k3_masks: (30, 60) per unet and [60, 50] per sample; main_masked: (15, 30)); the negated one at -6.  The tiny
untrained models respond weakly to the text, the dynamic threshold saturates and the cascade's second stage dilutes what the first one
moved: at a further weight of 6 the cascade runs lie 5.5 .. 6.3 bars from their plain-CFG twin, at 15 still 6.9 .. 7.3 (measured);
tools/make_compose_golden.py wants 10 and prints what each run reaches (10.4 .. 33 bars)."""
from __future__ import annotations

from typing import Callable

import torch
import torch.nn.functional as F

import fixtures_guidance as fg
import fixtures_solver as fs
from fixtures_common import GOLDEN, load, nerr  # noqa: F401

COND_SCALE, STEPS, SAMPLERS = fg.COND_SCALE, fg.STEPS, fg.SAMPLERS
WIDTH = 32


def prompt(seed: int, batch: int = 2, tokens: int = 7, scale: float = 1.0):
    """A further prompt: [batch, tokens, 32] embeddings, every position attended."""
    return torch.randn(batch, tokens, WIDTH, generator=torch.Generator().manual_seed(seed)) * scale


def half_mask(side: str, size: int = 16, batch: int = 1):
    """1 on one half of a size x size image, 0 on the other: 'left' | 'right' | 'top' | 'bottom'."""
    m = torch.zeros(batch, size, size)
    if side == "left":
        m[..., : size // 2] = 1.0
    elif side == "right":
        m[..., size // 2:] = 1.0
    elif side == "top":
        m[:, : size // 2] = 1.0
    else:
        m[:, size // 2:] = 1.0
    return m


def settings():
    """name -> dict(compose=[...], compose_mask=...): the keywords of a recorded run, as Imagen.sample takes them."""
    return {
        # K = 2, weights: a batch-1 prompt at one weight for both unets
        "k2": dict(compose=[dict(text_embeds=prompt(41, batch=1, scale=4.0), weight=40.0)]),
        # K = 3 with half-image masks: the main prompt everywhere, one further prompt per half (a per-unet weight tuple, a [B] weight tensor)
        "k3_masks": dict(compose=[dict(text_embeds=prompt(42, scale=4.0), weight=(30.0, 60.0), mask=half_mask("left")),
                                  dict(text_embeds=prompt(43, tokens=11, scale=4.0), weight=torch.tensor([60.0, 50.0]), mask=half_mask("right", batch=2))]),
        # negation
        "negative_weight": dict(compose=[dict(text_embeds=prompt(44), weight=-6.0)]),
        # the main prompt masked too (top half), fractional mask on the further one
        "main_masked": dict(compose=[dict(text_embeds=prompt(45), weight=(15.0, 30.0), mask=half_mask("bottom") * 0.75)], compose_mask=half_mask("top")),
    }


def resized(mask, hw):
    """A [b, H, W] mask at `hw` with the nearest rule of the cascade (F.interpolate(mode='nearest') = imagen.nearest_indices)."""
    return mask if tuple(mask.shape[-2:]) == tuple(hw) else F.interpolate(mask[:, None], tuple(hw), mode="nearest")[:, 0]


def compose_sample(unets, sizes, text_embeds, *, sampler: str, steps, cond_scale, compose, compose_mask=None, noise_fn: Callable, negative=None,
                   return_all: bool = False):
    """The restatement.  compose / compose_mask as Imagen.sample takes them (text_embeds only); compose=None is plain guidance (the twin)."""
    from oracle import sampler_oracle as so
    from oracle.unet_oracle import unet_forward

    n = len(unets)
    per = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v,) * n
    steps, cond_scale = per(steps), per(cond_scale)
    kind, eta = SAMPLERS[sampler]
    schedules = so.default_noise_schedules(n)
    b = text_embeds.shape[0]
    prompts = [(text_embeds, torch.any(text_embeds != 0.0, dim=-1))]
    weights, masks = [[torch.full((b,), float(cs)) for cs in cond_scale]], [compose_mask]
    for e in compose or ():
        emb = e["text_embeds"].expand(b, -1, -1)
        prompts.append((emb, torch.any(emb != 0.0, dim=-1)))
        w = e.get("weight", 1.0)
        weights.append([w.float() if isinstance(w, torch.Tensor) else torch.full((b,), float(per(w)[stage])) for stage in range(n)])
        masks.append(e.get("mask"))
    outs, img = [], None
    for stage in range(n):
        sd, kw = unets[stage]
        hw = (sizes[stage],) * 2 if isinstance(sizes[stage], int) else tuple(sizes[stage])
        shape = (b, 3, *hw)
        common = {}
        if kw.get("lowres_cond", False):
            up = img if tuple(img.shape[2:]) == tuple(shape[2:]) else F.interpolate(img, tuple(shape[2:]), mode="nearest")
            up = up * 2 - 1
            lowres_logsnr = so.SCHEDULES["linear"](torch.full((b,), 0.2, dtype=torch.float32))
            a, s = so.alpha_sigma(lowres_logsnr.reshape(-1, 1, 1, 1))
            common = dict(lowres_cond_img=a * up + s * noise_fn(("lowres", stage), tuple(up.shape)), lowres_noise_times=lowres_logsnr)
        rows = fs.restated_rows(schedules[stage], kind, steps[stage], eta)
        # t_k = w_k * m_k per pixel, fp32, as the kernel forms it
        t = []
        for k in range(len(prompts)):
            tk = weights[k][stage].reshape(b, 1, 1, 1)
            if masks[k] is not None:
                m = masks[k] if masks[k].ndim == 3 else masks[k][None]
                tk = tk * resized(m.float(), hw).expand(b, -1, -1)[:, None]
            t.append(tk)
        with torch.no_grad():
            x = noise_fn(("init", stage), tuple(shape))
            x0_prev = None
            for i, r in enumerate(rows):
                log_snr = torch.full((b,), r.log_snr, dtype=torch.float32)
                alpha, sigma = torch.tensor(r.alpha, dtype=torch.float32), torch.tensor(r.sigma, dtype=torch.float32)
                if negative is None:
                    nul = unet_forward(sd, kw, x, log_snr, text_embeds=prompts[0][0], text_mask=prompts[0][1], cond_drop_prob=1.0, **common)
                else:
                    nul = unet_forward(sd, kw, x, log_snr, text_embeds=negative[0].expand(b, -1, -1), text_mask=negative[1].expand(b, -1), **common)
                out = nul
                for k, (emb, tm) in enumerate(prompts):
                    cond = unet_forward(sd, kw, x, log_snr, text_embeds=emb, text_mask=tm, **common)
                    out = out + (cond - nul) * t[k]
                est = so.dynamic_threshold(so.predict_x0(x, out, alpha, sigma, "noise"), 0.95)
                nxt = r.on_x * x + r.on_x0 * est
                if r.on_prev != 0.0:
                    nxt = nxt + r.on_prev * x0_prev
                if eta > 0.0:
                    nxt = nxt + r.on_noise * noise_fn(("step", stage, i), tuple(shape))
                x, x0_prev = nxt, est
            img = (x.clamp(-1.0, 1.0) + 1) * 0.5
        outs.append(img)
    return outs if return_all else outs[-1]


NEGATIVE = (torch.randn(1, 6, WIDTH, generator=torch.Generator().manual_seed(5)), torch.ones(1, 6, dtype=torch.bool))


def groups():
    """The recorded groups: name -> dict(setting names, sampler, stages (None: the cascade; else the cascade's first unet alone), sizes, and what
    the product call / the restatement take beside them)."""
    return {
        "cascade.ddpm": dict(which=("k2", "negative_weight"), sampler="ddpm", stages=2),
        "cascade.dpmpp_2m": dict(which=("k3_masks", "main_masked"), sampler="dpmpp_2m", stages=2),
        "negative_prompt.ddpm": dict(which=("k2",), sampler="ddpm", stages=1, sample=dict(negative_text_embeds=NEGATIVE[0], negative_text_masks=NEGATIVE[1]),
                                     restate=dict(negative=NEGATIVE)),
        "rect.dpmpp_2m": dict(which=("k3_masks",), sampler="dpmpp_2m", stages=1, sizes=((16, 24),), sample=dict(image_shapes=((16, 24),))),
    }


def group_model(grp, device, steps):
    """The Imagen of a group at `steps` training timesteps (the ancestral sampler takes one step per timestep)."""
    if grp["stages"] == 2:
        return fs.cascade_model(device, timesteps=steps) if grp["sampler"] == "ddpm" else fs.cascade_model(device)
    return fs.single_stage_model(fs.cascade_specs()[0], 16, device, timesteps=steps if grp["sampler"] == "ddpm" else 4)


def to_device(kw, dev):
    """The compose keywords with every tensor moved to `dev`."""
    mv = lambda v: v.to(dev) if isinstance(v, torch.Tensor) else v
    out = {k: mv(v) for k, v in kw.items() if k != "compose"}
    if "compose" in kw:
        out["compose"] = [{k: mv(v) for k, v in e.items()} for e in kw["compose"]]
    return out


def keywords(which: str, stages: int, dev="cpu"):
    """settings()[which] for a model of `stages` unets on `dev`: a per-unet weight tuple keeps its first `stages` entries (the restatement
    reads entry [stage] of the same tuple)."""
    kw = to_device(settings()[which], dev)
    for e in kw["compose"]:
        if isinstance(e.get("weight"), tuple):
            e["weight"] = e["weight"][:stages] if stages > 1 else e["weight"][0]
    return kw


def runs_fixture():
    return load("compose_runs.pt")
