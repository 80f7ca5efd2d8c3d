"""Tiled sampling of Imagen.sample (tile_shapes=, tile_overlap=, tile_blend=): a plain fp32 sampling loop that, per step and tile, calls the
oracle's guided forward on the crop of the canvas (with the crop of the low-res image), applies CFG_X0's x0 expression to the tile, blends the
tiles' x0 in fp64 with the window weights of the issue (restated here with plain Python loops, not imported from the product), and then runs
the dynamic threshold and the restated solver row of tests/fixtures_solver.py on the canvas; the settings of the recorded runs and the loader of
tests/golden/tile_runs.pt (tools/make_tile_golden.py).  The tiny cascade of tests/fixtures_guide.py (dim 8, text width 32) at 16 x 48 then
32 x 96, tiles 16 x 16 on both stages at overlap 4: T = 4, then T = 3 x 8 = 24.  TEST INFRASTRUCTURE, never imported by the product.

The twin of every run is the same canvas through image_shapes alone (tile=None below): one forward on the whole canvas per step.  Every stage
of every run lies >= 10 bars from its twin's (tools/make_tile_golden.py asserts it and prints the figures).  The canvas and the second stage's
tiles are not the 16 x 24 -> 32 x 48 with 32 x 32 tiles one would pick first: there the base stage lay 5.5 .. 11 bars from its twin, and with
32 x 32 tiles the tiny super-resolution unet, which follows its low-res image, stayed 2.5 .. 7 bars from its twin on every canvas and overlap."""
from __future__ import annotations

from typing import Callable

import torch
import torch.nn.functional as F

import fixtures_guidance as fg
import fixtures_solver as fs
from fixtures_common import GOLDEN, load, nerr  # noqa: F401

COND_SCALE, STEPS, SAMPLERS = fg.COND_SCALE, fg.STEPS, fg.SAMPLERS
WIDTH = 32
SHAPES = ((16, 48), (32, 96))            # the canvas of every stage (image_shapes)
TILES = ((16, 16), (16, 16))             # tile_shapes
OVERLAPS = ((4, 4), (4, 4))              # tile_overlap: x origins 0, 12, 24, 32, then y 0, 12, 16 and x 0, 12, ..., 72, 80
NEGATIVE = (torch.randn(1, 6, WIDTH, generator=torch.Generator().manual_seed(5)), torch.ones(1, 6, dtype=torch.bool))


def restated_origins(N: int, L: int, o: int):
    """0, s, 2 s, ... while < N - L, then N - L (s = L - o)."""
    assert N >= L and 0 <= o < L
    out, v = [], 0
    while v < N - L:
        out.append(v)
        v += L - o
    return out + [N - L]


def restated_weights(H: int, W: int, h: int, w: int, oy: int, ox: int, blend: str):
    """(origins [(y0, x0)] row-major with y outer, nw fp64 [T, h, w]): the window min(i + 1, L - i, o + 1) / (o + 1) per axis ('uniform': 1),
    normalised by its sum over the tiles at every canvas pixel."""
    axis = lambda L, o: [1.0 if blend == "uniform" else min(i + 1, L - i, o + 1) / (o + 1) for i in range(L)]
    wy, wx = axis(h, oy), axis(w, ox)
    origins = [(y0, x0) for y0 in restated_origins(H, h, oy) for x0 in restated_origins(W, w, ox)]
    total = [[0.0] * W for _ in range(H)]
    for y0, x0 in origins:
        for i in range(h):
            for j in range(w):
                total[y0 + i][x0 + j] += wy[i] * wx[j]
    nw = torch.tensor([[[wy[i] * wx[j] / total[y0 + i][x0 + j] for j in range(w)] for i in range(h)] for y0, x0 in origins], dtype=torch.float64)
    return origins, nw


def tile_sample(unets, sizes, text_embeds, *, sampler: str, steps, cond_scale, tiles, overlaps=None, blend: str = "ramp", noise_fn: Callable,
                negative=None, lowres_level: float = 0.2, return_all: bool = False):
    """The restatement.  tiles: per stage None (untiled: the twin's stage) or (h, w); overlaps: per stage (oy, ox)."""
    from oracle import sampler_oracle as so
    from oracle.unet_oracle import unet_forward, unet_forward_with_cond_scale

    n = len(unets)
    per = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v,) * n
    steps, cond_scale = per(steps), per(cond_scale)
    kind, eta = SAMPLERS[sampler]
    schedules = so.default_noise_schedules(n)
    b = text_embeds.shape[0]
    masks = torch.any(text_embeds != 0.0, dim=-1)
    outs, img = [], None
    for stage in range(n):
        sd, kw = unets[stage]
        H, W = (sizes[stage],) * 2 if isinstance(sizes[stage], int) else tuple(sizes[stage])
        shape = (b, 3, H, W)
        lowres_img = lowres_logsnr = None
        if kw.get("lowres_cond", False):
            up = img if tuple(img.shape[2:]) == (H, W) else F.interpolate(img, (H, W), mode="nearest")
            up = up * 2 - 1
            lowres_logsnr = so.SCHEDULES["linear"](torch.full((b,), lowres_level, dtype=torch.float32))
            a, s = so.alpha_sigma(lowres_logsnr.reshape(-1, 1, 1, 1))
            lowres_img = a * up + s * noise_fn(("lowres", stage), tuple(up.shape))          # augmented once, on the canvas

        def guided(x, log_snr, lowres, _sd=sd, _kw=kw, _cs=cond_scale[stage], _lt=lowres_logsnr):
            common = dict(lowres_cond_img=lowres, lowres_noise_times=_lt)
            if negative is None or _cs == 1.0:
                return unet_forward_with_cond_scale(_sd, _kw, x, log_snr, cond_scale=_cs, text_embeds=text_embeds, text_mask=masks, **common)
            cond = unet_forward(_sd, _kw, x, log_snr, text_embeds=text_embeds, text_mask=masks, **common)
            nul = unet_forward(_sd, _kw, x, log_snr, text_embeds=negative[0].expand(b, -1, -1), text_mask=negative[1].expand(b, -1), **common)
            return nul + (cond - nul) * _cs

        if tiles[stage] is None:
            h, w, origins, nw = H, W, [(0, 0)], torch.ones(1, H, W, dtype=torch.float64)
        else:
            h, w = tiles[stage]
            origins, nw = restated_weights(H, W, h, w, *overlaps[stage], blend)
        rows = fs.restated_rows(schedules[stage], kind, steps[stage], eta)
        with torch.no_grad():
            x = noise_fn(("init", stage), shape)
            x0_prev = None
            for i, r in enumerate(rows):
                log_snr = torch.full((b,), r.log_snr, dtype=torch.float32)
                alpha, sigma = torch.tensor(r.alpha, dtype=torch.float32), torch.tensor(r.sigma, dtype=torch.float32)
                acc = torch.zeros(shape, dtype=torch.float64)
                for t, (y0, x0) in enumerate(origins):
                    crop = x[:, :, y0:y0 + h, x0:x0 + w].contiguous()
                    low = None if lowres_img is None else lowres_img[:, :, y0:y0 + h, x0:x0 + w].contiguous()
                    est_t = so.predict_x0(crop, guided(crop, log_snr, low), alpha, sigma, "noise")
                    acc[:, :, y0:y0 + h, x0:x0 + w] += nw[t] * est_t.double()
                est = so.dynamic_threshold(acc.float(), 0.95)
                nxt = r.on_x * x + r.on_x0 * est
                if r.on_prev != 0.0:
                    nxt = nxt + r.on_prev * x0_prev
                if eta > 0.0:
                    nxt = nxt + r.on_noise * noise_fn(("step", stage, i), shape)
                x, x0_prev = nxt, est
            img = (x.clamp(-1.0, 1.0) + 1) * 0.5
        outs.append(img)
    return outs if return_all else outs[-1]


def groups():
    """The recorded runs: name -> dict(sampler, blend, and what the product call / the restatement take beside the tile keywords)."""
    neg = dict(sample=dict(negative_text_embeds=NEGATIVE[0], negative_text_masks=NEGATIVE[1]), restate=dict(negative=NEGATIVE))
    return {
        "ddpm.ramp": dict(sampler="ddpm", blend="ramp"),
        "ddpm.uniform": dict(sampler="ddpm", blend="uniform"),
        "dpmpp_2m.ramp": dict(sampler="dpmpp_2m", blend="ramp"),
        "dpmpp_2m.uniform": dict(sampler="dpmpp_2m", blend="uniform"),
        "dpmpp_2m.ramp.negative": dict(sampler="dpmpp_2m", blend="ramp", **neg),
    }


def group_model(grp, device, steps):
    return fs.cascade_model(device, timesteps=steps) if grp["sampler"] == "ddpm" else fs.cascade_model(device)


def keywords(grp, steps, dev="cpu", tiled: bool = True):
    """The Imagen.sample keywords of a recorded run (tiled) or of its twin."""
    kw = dict(image_shapes=SHAPES, **{k: v.to(dev) for k, v in grp.get("sample", {}).items()})
    if grp["sampler"] != "ddpm":
        kw.update(sampler=grp["sampler"], sample_steps=steps)
    if tiled:
        kw.update(tile_shapes=TILES, tile_overlap=OVERLAPS, tile_blend=grp["blend"])
    return kw


def restate(grp, steps, noise_fn, tiled: bool = True):
    g = fs.cascade_fixture()
    return tile_sample(fs.cascade_specs(), SHAPES, g["text_embeds"], sampler=grp["sampler"], steps=steps, cond_scale=COND_SCALE,
                       tiles=TILES if tiled else (None, None), overlaps=OVERLAPS, blend=grp["blend"], noise_fn=noise_fn, return_all=True,
                       **grp.get("restate", {}))


def runs_fixture():
    return load("tile_runs.pt")


def twins_fixture():
    """{run name: [the untiled twin's output per stage]}."""
    return load("tile_twins.pt")["twins"]


def noise_fixture():
    """{tag: draw}: the Gaussian draws every recorded run and twin read."""
    return load("tile_noise.pt")["noise"]
