"""Few-step solvers of Imagen.sample (sampler='ddim' | 'dpmpp_2m'): an independent restatement of the coefficient formulas
 in 60-digit decimal arithmetic, a plain fp32 sampling loop over the oracle's guided forward that applies them, the
fixture models (all from weights already under tests/golden/), the launch lists of the default call in the form of
tests/golden/solver_parent_launch_list_abi<N>.json and the loader of tests/golden/solver_runs.pt (tools/make_solver_golden.py).
TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

from decimal import Decimal, getcontext
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn.functional as F

from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401

getcontext().prec = 60

STEPS = 6            # solver steps of the recorded runs
COND_SCALE = 3.0


class Row(NamedTuple):
    """One solver step: the log-SNR the denoiser is conditioned on, (alpha, sigma) of the x0 estimate, and the update
    x_next = on_x * x + on_x0 * x0 + on_prev * x0_prev + on_noise * z."""
    log_snr: float
    alpha: float
    sigma: float
    alpha_next: float
    sigma_next: float
    c: float
    nonzero: float
    on_x: float
    on_x0: float
    on_prev: float
    on_noise: float


def grid_log_snr(schedule: str, steps: int):
    """log_snr on linspace(1, 0, steps + 1) as the reference's scheduler evaluates it (fp32; ip.py:212-218, 245-250) — the values a
    checkpoint's denoiser was conditioned on.  Everything below is derived from them exactly."""
    from oracle import sampler_oracle as so

    t = torch.linspace(1.0, 0.0, steps + 1)
    return [float(v) for v in so.SCHEDULES[schedule](t)], [float(v) for v in t]


def restated_rows(schedule: str, sampler: str, steps: int, eta: float = 0.0, start: int = 0):
    """The formulas of the issue, literally, per step and in decimal arithmetic:
      l = log_snr(t), alpha^2 = sigmoid(l), sigma^2 = sigmoid(-l), lambda = l / 2, h = lambda_next - lambda, c = -expm1(l - l_next)
      ddim:      s = eta sigma_n sqrt(c);  x_next = alpha_n x0 + sqrt(sigma_n^2 - s^2) (x - alpha x0) / sigma + nonzero s z
      dpmpp_2m:  x_next = (sigma_n / sigma) x - alpha_n expm1(-h) D,  D = (1 + 1/(2r)) x0 - (1/(2r)) x0_prev,  r = h_prev / h;
                 D = x0 on the first step of the run (`start`) and on the last."""
    ls, ts = grid_log_snr(schedule, steps)
    one = Decimal(1)
    sig = lambda v: one / (one + (-v).exp())
    L = [Decimal(v) for v in ls]
    rows = []
    for i in range(steps):
        l, ln = L[i], L[i + 1]
        a, s, an, sn = sig(l).sqrt(), sig(-l).sqrt(), sig(ln).sqrt(), sig(-ln).sqrt()
        c = one - (l - ln).exp()
        nonzero = Decimal(0 if ts[i + 1] == 0.0 else 1)
        on_prev = on_noise = Decimal(0)
        if sampler == "ddim":
            sd = Decimal(eta) * sn * c.sqrt()
            on_x = (sn * sn - sd * sd).sqrt() / s
            on_x0 = an - a * on_x
            on_noise = nonzero * sd
        elif sampler == "dpmpp_2m":
            h = (ln - l) / 2
            g = -an * ((-h).exp() - one)
            on_x = sn / s
            if i in (start, steps - 1) or i == 0:
                on_x0 = g
            else:
                r = ((l - L[i - 1]) / 2) / h
                on_x0, on_prev = g * (one + one / (2 * r)), -g / (2 * r)
        else:
            raise ValueError(sampler)
        rows.append(Row(*(float(v) for v in (l, a, s, an, sn, c, nonzero, on_x, on_x0, on_prev, on_noise))))
    return rows


# ------------------------------------------------------------------------------------------------ the fp32 loop over the oracle

def solver_loop(denoise: Callable, shape, rows, *, noise_fn: Callable, stage: int, dynamic_thresholding: bool = True, percentile: float = 0.95,
                self_cond: bool = False, pred_objective: str = "noise", init_images: Optional[torch.Tensor] = None, skip_steps: int = 0,
                max_steps: Optional[int] = None, trace: Optional[list] = None) -> torch.Tensor:
    """One stage: x ~ noise_fn(("init", stage)) (+ init_images, normalised, at this size), then for every row the guided denoiser at the
    row's log-SNR -> x0 (oracle.predict_x0) -> threshold (ip.py:2094-2107) -> the row's update; the draw of a stochastic row is
    noise_fn(("step", stage, i)).  Returns the [0, 1] image (ip.py:2281-2288)."""
    from oracle import sampler_oracle as so

    b = shape[0]
    img = noise_fn(("init", stage), tuple(shape))
    if init_images is not None:
        img = img + init_images
    x0 = None
    last = len(rows) if max_steps is None else min(len(rows), skip_steps + max_steps)
    for i in range(skip_steps, last):
        r = rows[i]
        log_snr = torch.full((b,), r.log_snr, dtype=torch.float32)
        pred = denoise(img, log_snr, x0) if self_cond else denoise(img, log_snr)
        est = so.predict_x0(img, pred, torch.tensor(r.alpha, dtype=torch.float32), torch.tensor(r.sigma, dtype=torch.float32), pred_objective)
        est = so.dynamic_threshold(est, percentile) if dynamic_thresholding else est.clamp(-1.0, 1.0)
        nxt = r.on_x * img + r.on_x0 * est
        if r.on_prev != 0.0:
            nxt = nxt + r.on_prev * x0
        if r.on_noise != 0.0:
            nxt = nxt + r.on_noise * noise_fn(("step", stage, i), tuple(shape))
        img, x0 = nxt, est
        if trace is not None:
            trace.append(img.clone())
    return (img.clamp(-1.0, 1.0) + 1) * 0.5


def solver_sample(unets, sizes, text_embeds, *, sampler: str, steps, eta: float = 0.0, cond_scale=COND_SCALE, noise_fn: Callable,
                  video_frames: Optional[int] = None, skip_steps=None, init_images=None, lowres_sample_noise_level: float = 0.2,
                  start_image=None, start_at: int = 0, return_all: bool = False):
    """The cascade of oracle.sampler_oracle.imagen_sample (text conditioning, CFG, low-res noise augmentation, the default schedules
    'cosine', 'cosine', 'linear'...) with `solver_loop` in place of the ancestral loop.  unets: [(state_dict, ctor kwargs)]; sizes: an
    int or (H, W) per stage; steps: an int or one per stage."""
    from oracle import sampler_oracle as so
    from oracle.unet3d_oracle import unet3d_forward_with_cond_scale
    from oracle.unet_oracle import unet_forward_with_cond_scale

    n = len(unets)
    per = lambda v: tuple(v) if isinstance(v, (list, tuple)) else (v,) * n
    steps, skips, inits, scales = per(steps), per(skip_steps), per(init_images), per(cond_scale)
    schedules = so.default_noise_schedules(n)
    masks = torch.any(text_embeds != 0.0, dim=-1)
    b = text_embeds.shape[0]
    video = video_frames is not None
    fwd = unet3d_forward_with_cond_scale if video else unet_forward_with_cond_scale
    outs, img = [], start_image
    for stage in range(start_at, n):
        sd, kw = unets[stage]
        hw = (sizes[stage],) * 2 if isinstance(sizes[stage], int) else tuple(sizes[stage])
        shape = (b, 3, video_frames, *hw) if video else (b, 3, *hw)
        lowres_img = lowres_logsnr = None
        if kw.get("lowres_cond", False):
            target = shape[2:]
            up = img if tuple(img.shape[2:]) == tuple(target) else F.interpolate(img, tuple(target), mode="nearest")
            up = up * 2 - 1
            times = torch.full((b,), lowres_sample_noise_level, dtype=torch.float32)
            lowres_logsnr = so.SCHEDULES["linear"](times)
            a, s = so.alpha_sigma(lowres_logsnr.reshape(-1, *([1] * (up.ndim - 1))))
            lowres_img = a * up + s * noise_fn(("lowres", stage), tuple(up.shape))

        def denoise(x, log_snr, x0_prev=None, _sd=sd, _kw=kw, _cs=scales[stage], _li=lowres_img, _lt=lowres_logsnr):
            extra = dict(self_cond=x0_prev) if _kw.get("self_cond", False) else {}
            return fwd(_sd, _kw, x, log_snr, cond_scale=_cs, text_embeds=text_embeds, text_mask=masks, lowres_cond_img=_li,
                       lowres_noise_times=_lt, **extra)

        skip = skips[stage] or 0
        init = inits[stage]
        if init is not None:
            init = init * 2 - 1
            init = init if tuple(init.shape[2:]) == tuple(shape[2:]) else F.interpolate(init, tuple(shape[2:]), mode="nearest")
        rows = restated_rows(schedules[stage], sampler, steps[stage], eta, start=skip)
        with torch.no_grad():
            img = solver_loop(denoise, shape, rows, noise_fn=noise_fn, stage=stage, self_cond=bool(kw.get("self_cond", False)),
                              init_images=init, skip_steps=skip)
        outs.append(img)
    return outs if return_all else outs[-1]


# ------------------------------------------------------------------------------------------------ fixture models and draws

def memo_noise(seed: int, device="cpu"):
    """noise_fn(tag, shape): one standard normal draw per tag from a CPU generator, kept, so that the product and the restatement
    (and every repetition of a call) read the same tensors."""
    gen, draws = torch.Generator().manual_seed(seed), {}

    def fn(tag, shape):
        if tag not in draws:
            draws[tag] = torch.randn(tuple(shape), generator=gen)
        assert tuple(draws[tag].shape) == tuple(shape), (tag, shape)
        return draws[tag].to(device)
    fn.draws = draws
    return fn


def fixed_noise(draws: dict, device="cpu"):
    return lambda tag, shape: draws[tag].to(device)


def cascade_fixture():
    return load("sample_tiny_cascade.pt")


def cascade_specs():
    return [(u["state_dict"], u["kwargs"]) for u in cascade_fixture()["unets"]]


def cascade_model(device="cpu", weights=True, **kw):
    """The two-stage image cascade 16^2 -> 32^2 of tests/golden/sample_tiny_cascade.pt (dim 8; stage 2 low-res conditioned) as Imagen."""
    from imagen_pytorch_amd import Imagen, Unet

    g = cascade_fixture()
    kw.setdefault("timesteps", g["timesteps"])
    model = Imagen([Unet(**u["kwargs"]).eval() for u in g["unets"]], image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **kw)
    if str(device) != "cpu":
        model = model.to(device)
    if weights:
        for m, u in zip(model.unets, g["unets"]):
            m.load_state_dict(u["state_dict"])
    return model.eval()


def selfcond_spec():
    """(state_dict, kwargs) of the first Unet(self_cond=True) of tests/golden/selfcond_image_runs.pt (dim 16, 16^2)."""
    spec = load(load("selfcond_image_runs.pt")["weights_from"][0])
    return unpack_state_dict(spec), dict(spec["kwargs"])


def video_spec():
    """(state_dict, kwargs) of the first Unet3D of tests/golden/sample_tiny_video.pt."""
    u = load("sample_tiny_video.pt")["unets"][0]
    return u["state_dict"], dict(u["kwargs"])


def single_stage_model(spec, size, device="cpu", timesteps=4, video=False):
    """Imagen over one unet — a Unet, or with `video` a Unet3D — at `size`."""
    from imagen_pytorch_amd import Imagen, Unet, Unet3D

    sd, kw = spec
    model = Imagen(((Unet3D if video else Unet)(**kw).eval(),), image_sizes=(size,), timesteps=timesteps, text_embed_dim=32, cond_drop_prob=0.1)
    if str(device) != "cpu":
        model = model.to(device)
    model.unets[0].load_state_dict(sd)
    return model.eval()


def video_model(device="cpu", timesteps=4):
    return single_stage_model(video_spec(), load("sample_tiny_video.pt")["image_sizes"][0], device, timesteps, video=True)


def runs_fixture():
    return load("solver_runs.pt")


# ------------------------------------------------------------------------------------------------ launch lists of the default call

def _ops(plan):
    return [[int(k), l] for k, _, l in plan.ops]


def launch_lists():
    """{name: [[kind, label], ...]} of the per-step plan of both stages of the tiny cascade as a default sample() call builds them
    (sampler='ddpm'; Philox noise and injected noise), built dry.  Call with engine.UnetEngine patched to dry=True."""
    out = {}
    model = cascade_model(weights=False)
    dev = torch.device("cpu")
    for inject in (False, True):
        for idx in range(2):
            st = model._stage(idx, 2, dev, cond_scale=COND_SCALE, with_text=True, inject_noise=inject, sample_offset=0)
            out[f"stage{idx}.{'injected' if inject else 'philox'}.plan"] = _ops(st["plan"])
            out[f"stage{idx}.{'injected' if inject else 'philox'}.step"] = _ops(st["step_plan"])
    return out
