"""Guidance rescale and adaptive projected guidance of Imagen.sample (guidance_rescale= / guidance_apg=): a plain fp32 sampling loop over the
oracle's conditional and null forwards that applies the formulas of include/imagen_hip.h (GUIDE_X0) per guided step, the per-sample sums in
fp64, the momentum's running average carried across the steps of a stage; the settings of the recorded runs and the loader of
tests/golden/guide_runs.pt (tools/make_guide_golden.py).  It extends tests/fixtures_guidance.py: the same tiny cascades, STEPS, COND_SCALE = 7.5,
the same restated solver rows (the ancestral sampler as the ddim row at eta = 1).  A step whose scale is 1 (outside a guidance interval) is the
conditional forward alone and leaves the running average as it is.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn.functional as F

import fixtures_guidance as fg
import fixtures_solver as fs
from fixtures_common import GOLDEN, load, nerr  # noqa: F401

COND_SCALE, STEPS, SAMPLERS = fg.COND_SCALE, fg.STEPS, fg.SAMPLERS
# phi: at 0.7 the tiny cascades move only 5 .. 7 bars from their plain-CFG twin (tools/make_guide_golden.py wants 10), at 1.0 they move 10 .. 16;
# the blend itself (phi = 0.7) is checked per element by tests/test_guide_kernel_gpu.py
RESCALE = ("rescale", 1.0)
# eta, norm_threshold, momentum.  These untrained models predict x0 of the order 1e8 at the first step (alpha ~ 0 at t = 1, before the dynamic
# threshold), so |D| starts near 8e8 and, with momentum -0.5, about halves every step: the cap at 2e8 binds on the first steps of a stage
# and is slack on the later ones (tools/make_guide_golden.py prints |D| per step)
APG = ("apg", 0.0, 2e8, -0.5)
KEYWORDS = {"rescale": dict(guidance_rescale=RESCALE[1]), "apg": dict(guidance_apg=dict(eta=APG[1], norm_threshold=APG[2], momentum=APG[3]))}
SETTINGS = {"rescale": RESCALE, "apg": APG}


def guided_x0(x, cond, nul, alpha, sigma, s: float, objective: str, guide, avg):
    """One guided step's x0 estimate (before thresholding) and the new running average.  fp32 elementwise, fp64 per-sample sums."""
    from oracle import sampler_oracle as so

    x0 = lambda e: so.predict_x0(x, e, alpha, sigma, objective)
    flat = lambda t: t.reshape(t.shape[0], -1).double()
    per = lambda v: v.float().reshape(-1, *([1] * (x.ndim - 1)))
    s = torch.tensor(s, dtype=torch.float32)
    if guide is None:
        return x0(nul + (cond - nul) * s), avg
    if guide[0] == "rescale":
        g = nul + (cond - nul) * s
        f = per(flat(cond).std(1, unbiased=False) / flat(g).std(1, unbiased=False))
        return x0(guide[1] * (g * f) + (1 - guide[1]) * g), avg
    _, eta, thr, mom = guide
    dc, du = x0(cond), x0(nul)
    d = dc - du
    if mom != 0.0:
        d = d + mom * avg
        avg = d
    r = torch.ones(x.shape[0], dtype=torch.float64)
    if thr > 0.0:
        r = (thr / flat(d).norm(dim=1)).clamp(max=1.0)
    k = r * (flat(d) * flat(dc)).sum(1) / (flat(dc) ** 2).sum(1)
    dp, par = per(r) * d, per(k) * dc
    return dc + (s - 1) * ((dp - par) + eta * par), avg


def guide_sample(unets, sizes, text_embeds, *, sampler: str, steps, scales, guides, noise_fn: Callable, video_frames: Optional[int] = None,
                 negative=None, objectives=None, return_all: bool = False, caps: Optional[list] = None):
    """fixtures_guidance.guided_sample with `guides[stage]` (None | RESCALE-like | APG-like) applied on the guided steps of the stage."""
    from oracle import sampler_oracle as so
    from oracle.unet3d_oracle import unet3d_forward
    from oracle.unet_oracle import unet_forward

    n = len(unets)
    per = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v,) * n
    steps, objectives = per(steps), per(objectives or "noise")
    kind, eta = SAMPLERS[sampler]
    schedules = so.default_noise_schedules(n)
    masks = torch.any(text_embeds != 0.0, dim=-1)
    b = text_embeds.shape[0]
    video = video_frames is not None
    plain = unet3d_forward if video else unet_forward
    outs, img = [], None
    for stage in range(n):
        sd, kw = unets[stage]
        hw = (sizes[stage],) * 2 if isinstance(sizes[stage], int) else tuple(sizes[stage])
        shape = (b, 3, video_frames, *hw) if video else (b, 3, *hw)
        common = {}
        if kw.get("lowres_cond", False):
            up = img if tuple(img.shape[2:]) == tuple(shape[2:]) else F.interpolate(img, tuple(shape[2:]), mode="nearest")
            up = up * 2 - 1
            lowres_logsnr = so.SCHEDULES["linear"](torch.full((b,), 0.2, dtype=torch.float32))
            a, s = so.alpha_sigma(lowres_logsnr.reshape(-1, *([1] * (up.ndim - 1))))
            common = dict(lowres_cond_img=a * up + s * noise_fn(("lowres", stage), tuple(up.shape)), lowres_noise_times=lowres_logsnr)
        rows = fs.restated_rows(schedules[stage], kind, steps[stage], eta)
        assert len(scales[stage]) == len(rows)
        self_cond = bool(kw.get("self_cond", False))
        with torch.no_grad():
            x = noise_fn(("init", stage), tuple(shape))
            x0_prev, avg = None, torch.zeros(shape)
            for i, r in enumerate(rows):
                log_snr = torch.full((b,), r.log_snr, dtype=torch.float32)
                extra = dict(self_cond=x0_prev, **common) if self_cond else common
                alpha, sigma = torch.tensor(r.alpha, dtype=torch.float32), torch.tensor(r.sigma, dtype=torch.float32)
                cond = plain(sd, kw, x, log_snr, text_embeds=text_embeds, text_mask=masks, **extra)
                if scales[stage][i] == 1.0:
                    est = so.predict_x0(x, cond, alpha, sigma, objectives[stage])
                else:
                    if negative is None:
                        nul = plain(sd, kw, x, log_snr, text_embeds=text_embeds, text_mask=masks, cond_drop_prob=1.0, **extra)
                    else:
                        nul = plain(sd, kw, x, log_snr, text_embeds=negative[0].expand(b, -1, -1), text_mask=negative[1].expand(b, -1), **extra)
                    est, avg = guided_x0(x, cond, nul, alpha, sigma, scales[stage][i], objectives[stage], guides[stage], avg)
                    if caps is not None and guides[stage] is not None and guides[stage][0] == "apg" and guides[stage][2] > 0:
                        caps.append(float(avg.reshape(b, -1).norm(dim=1).max()))
                est = so.dynamic_threshold(est, 0.95)
                nxt = r.on_x * x + r.on_x0 * est
                if r.on_prev != 0.0:
                    nxt = nxt + r.on_prev * x0_prev
                if eta > 0.0:
                    nxt = nxt + r.on_noise * noise_fn(("step", stage, i), tuple(shape))
                x, x0_prev = nxt, est
            img = (x.clamp(-1.0, 1.0) + 1) * 0.5
        outs.append(img)
    return outs if return_all else outs[-1]


def v_model(device="cpu", timesteps=4):
    """The cascade's first unet as a one-stage Imagen with the v objective."""
    from imagen_pytorch_amd import Imagen, Unet

    sd, kw = fs.cascade_specs()[0]
    model = Imagen((Unet(**kw).eval(),), image_sizes=(16,), timesteps=timesteps, text_embed_dim=32, cond_drop_prob=0.1, pred_objectives="v")
    if str(device) != "cpu":
        model = model.to(device)
    model.unets[0].load_state_dict(sd)
    return model.eval()


# the recorded variants: name -> (model builder(device, steps), specs, sizes, steps, sampler, which setting, sample() keywords, restatement keywords)
def variants():
    g = fs.cascade_fixture()
    v = fs.load("sample_tiny_video.pt")
    specs = fs.cascade_specs()
    neg = (torch.randn(1, 6, 32, generator=torch.Generator().manual_seed(5)), torch.ones(1, 6, dtype=torch.bool))
    te = g["text_embeds"]
    return {
        "v.rescale": dict(model=lambda dev, T: v_model(dev, T), unets=specs[:1], sizes=(16,), steps=4, sampler="ddpm", which="rescale", te=te,
                          restate=dict(objectives="v")),
        "selfcond.apg": dict(model=lambda dev, T: fs.single_stage_model(fs.selfcond_spec(), 16, dev, timesteps=T), unets=[fs.selfcond_spec()], sizes=(16,),
                             steps=4, sampler="ddpm", which="apg", te=te),
        "video.apg": dict(model=lambda dev, T: fs.video_model(dev, timesteps=T), unets=[fs.video_spec()], sizes=(v["image_sizes"][0],), steps=4,
                              sampler="ddpm", which="apg", te=v["text_embeds"], sample=dict(video_frames=v["frames"]),
                              restate=dict(video_frames=v["frames"])),
        "rect.rescale": dict(model=lambda dev, T: fs.single_stage_model(specs[0], 16, dev, timesteps=T), unets=specs[:1], sizes=((16, 24),), steps=4,
                         sampler="dpmpp_2m", which="rescale", te=te, sample=dict(image_shapes=((16, 24),))),
        "negative_interval.apg": dict(model=lambda dev, T: fs.single_stage_model(specs[0], 16, dev, timesteps=T), unets=specs[:1], sizes=(16,), steps=4,
                                      sampler="ddpm", which="apg", te=te, interval=True,
                                      sample=dict(negative_text_embeds=neg[0], negative_text_masks=neg[1], guidance_interval=fg.INTERVAL),
                                      restate=dict(negative=neg)),
    }


def runs_fixture():
    return load("guide_runs.pt")
