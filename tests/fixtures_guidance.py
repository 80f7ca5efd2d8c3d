"""Guidance schedules of Imagen.sample (guidance_schedule= / guidance_interval=): a restatement of how the two keywords resolve to one scale
per step, a plain fp32 sampling loop over the oracle's guided forward that hands step i its own scale s_i (scale 1: the conditional forward
alone, as oracle.*_forward_with_cond_scale does it), the schedules of the recorded runs and the loader of tests/golden/guidance_runs.pt
(tools/make_guidance_golden.py).  The steps themselves are those of tests/fixtures_solver.py: its decimal restatement of the solver rows,
and for the ancestral sampler the same restatement's ddim row at eta = 1 on the training grid, which is the reference's posterior step
(tests/test_solver_cpu.py anchors it to the reference's recorded DDPM run).  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

from fractions import Fraction
from typing import Callable, Optional

import torch
import torch.nn.functional as F

import fixtures_solver as fs
from fixtures_common import GOLDEN, load, nerr  # noqa: F401

COND_SCALE = 7.5            # the constant-scale twin of every recorded run
STEPS = {"ddpm": 4, "dpmpp_2m": 6, "ddim": 6}      # steps per stage of the recorded cascade runs (ddpm: Imagen(timesteps=4))
RAMP = lambda t: 12.0 * t - 2.5                    # high guidance early, low late: 9.5 at t = 1, 0.5 at t = 1 / 4 (-0.5 at 1 / 6)
INTERVAL = (0.3, 0.8)                              # of 4 steps (t = 1, .75, .5, .25) the middle two are guided, of 6 steps t = .667, .5, .333
STEEP = lambda t: 40.0 * t - 20.0                  # the ramp enlarged for the self_cond unet, which answers guidance weakly: 20, 10, 0, -10 at 4 steps
SWITCH = [20.0, 1.0, 0.0, -10.0]                   # guided -> unguided -> guided -> guided, as a sequence (a 4-step stage)
SAMPLERS = {"ddpm": ("ddim", 1.0), "dpmpp_2m": ("dpmpp_2m", 0.0), "ddim": ("ddim", 0.0)}      # sampler= -> (restated row kind, eta)


def restated_times(steps: int):
    """t of row i on the grid linspace(1, 0, steps + 1), exactly: (steps - i) / steps."""
    return [Fraction(steps - i, steps) for i in range(steps)]


def restated_scales(steps: int, cond_scale: float, schedule=None, interval=None):
    """The issue's rules, literally: a callable is evaluated at t, a sequence is taken as it is, None is cond_scale; then every step whose t
    lies outside the closed interval runs at scale 1.  The interval is compared in exact rational arithmetic on the decimal the caller wrote."""
    ts = restated_times(steps)
    if schedule is None:
        vals = [float(cond_scale)] * steps
    elif callable(schedule):
        vals = [float(schedule(float(t))) for t in ts]
    else:
        vals = [float(v) for v in schedule]
        assert len(vals) == steps
    if interval is not None:
        lo, hi = (Fraction(str(v)) for v in interval)
        vals = [v if lo <= t <= hi else 1.0 for v, t in zip(vals, ts)]
    return [float(torch.tensor(v, dtype=torch.float32)) for v in vals]


def guided_loop(denoise: Callable, shape, rows, scales, *, noise_fn: Callable, stage: int, self_cond: bool = False,
                init_images: Optional[torch.Tensor] = None, skip_steps: int = 0, stochastic: bool = False) -> torch.Tensor:
    """fixtures_solver.solver_loop with the step's own guidance scale handed to the denoiser: denoise(x, log_snr, scale, x0_prev).
    stochastic: every step draws ("step", stage, i), the last one too, whose weight is 0 (the ancestral sampler asks for it all the same)."""
    from oracle import sampler_oracle as so

    b = shape[0]
    img = noise_fn(("init", stage), tuple(shape))
    if init_images is not None:
        img = img + init_images
    x0 = None
    for i in range(skip_steps, len(rows)):
        r = rows[i]
        log_snr = torch.full((b,), r.log_snr, dtype=torch.float32)
        pred = denoise(img, log_snr, scales[i], x0 if self_cond else None)
        est = so.predict_x0(img, pred, torch.tensor(r.alpha, dtype=torch.float32), torch.tensor(r.sigma, dtype=torch.float32), "noise")
        est = so.dynamic_threshold(est, 0.95)
        nxt = r.on_x * img + r.on_x0 * est
        if r.on_prev != 0.0:
            nxt = nxt + r.on_prev * x0
        if stochastic:
            nxt = nxt + r.on_noise * noise_fn(("step", stage, i), tuple(shape))
        img, x0 = nxt, est
    return (img.clamp(-1.0, 1.0) + 1) * 0.5


def guided_sample(unets, sizes, text_embeds, *, sampler: str, steps, scales, noise_fn: Callable, video_frames: Optional[int] = None,
                  skip_steps=None, init_images=None, negative=None, return_all: bool = False):
    """The cascade of fixtures_solver.solver_sample with `scales[stage][i]` as the guidance scale of step i of stage `stage`.
    sampler: 'ddpm' | 'dpmpp_2m' | 'ddim' (eta 0).  negative = (embeds, mask): the prompt of the null branch (guided steps only: an
    unguided step has no null branch)."""
    from oracle import sampler_oracle as so
    from oracle.unet3d_oracle import unet3d_forward, unet3d_forward_with_cond_scale
    from oracle.unet_oracle import unet_forward, unet_forward_with_cond_scale

    n = len(unets)
    per = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v,) * n
    steps, skips, inits = per(steps), per(skip_steps), per(init_images)
    kind, eta = SAMPLERS[sampler]
    schedules = so.default_noise_schedules(n)
    masks = torch.any(text_embeds != 0.0, dim=-1)
    b = text_embeds.shape[0]
    video = video_frames is not None
    fwd, plain = (unet3d_forward_with_cond_scale, unet3d_forward) if video else (unet_forward_with_cond_scale, unet_forward)
    outs, img = [], None
    for stage in range(n):
        sd, kw = unets[stage]
        hw = (sizes[stage],) * 2 if isinstance(sizes[stage], int) else tuple(sizes[stage])
        shape = (b, 3, video_frames, *hw) if video else (b, 3, *hw)
        lowres_img = lowres_logsnr = None
        if kw.get("lowres_cond", False):
            up = img if tuple(img.shape[2:]) == tuple(shape[2:]) else F.interpolate(img, tuple(shape[2:]), mode="nearest")
            up = up * 2 - 1
            lowres_logsnr = so.SCHEDULES["linear"](torch.full((b,), 0.2, dtype=torch.float32))
            a, s = so.alpha_sigma(lowres_logsnr.reshape(-1, *([1] * (up.ndim - 1))))
            lowres_img = a * up + s * noise_fn(("lowres", stage), tuple(up.shape))

        def denoise(x, log_snr, scale, x0_prev, _sd=sd, _kw=kw, _li=lowres_img, _lt=lowres_logsnr):
            extra = dict(self_cond=x0_prev) if _kw.get("self_cond", False) else {}
            common = dict(lowres_cond_img=_li, lowres_noise_times=_lt, **extra)
            if negative is None or scale == 1.0:
                return fwd(_sd, _kw, x, log_snr, cond_scale=scale, text_embeds=text_embeds, text_mask=masks, **common)
            cond = plain(_sd, _kw, x, log_snr, text_embeds=text_embeds, text_mask=masks, **common)
            nul = plain(_sd, _kw, x, log_snr, text_embeds=negative[0].expand(b, -1, -1), text_mask=negative[1].expand(b, -1), **common)
            return nul + (cond - nul) * scale

        skip = skips[stage] or 0
        init = inits[stage]
        if init is not None:
            init = init * 2 - 1
            init = init if tuple(init.shape[2:]) == tuple(shape[2:]) else F.interpolate(init, tuple(shape[2:]), mode="nearest")
        rows = fs.restated_rows(schedules[stage], kind, steps[stage], eta, start=skip)
        assert len(scales[stage]) == len(rows)
        with torch.no_grad():
            img = guided_loop(denoise, shape, rows, scales[stage], noise_fn=noise_fn, stage=stage, self_cond=bool(kw.get("self_cond", False)),
                              init_images=init, skip_steps=skip, stochastic=eta > 0.0)
        outs.append(img)
    return outs if return_all else outs[-1]


def schedule_kwargs(which: str):
    """The sample() keywords of the recorded schedule `which`, and the same as (schedule, interval) for restated_scales."""
    return {"ramp": dict(guidance_schedule=RAMP), "steep": dict(guidance_schedule=STEEP), "interval": dict(guidance_interval=INTERVAL), "switch": dict(guidance_schedule=SWITCH)}[which]


def scales_of(which: str, steps: int):
    kw = schedule_kwargs(which)
    return restated_scales(steps, COND_SCALE, kw.get("guidance_schedule"), kw.get("guidance_interval"))


def runs_fixture():
    return load("guidance_runs.pt")
