"""Continuous-time Gaussian diffusion schedules (host side).

Mirror of the reference's `GaussianDiffusionContinuousTimes` (ip.py:212-318) for the sampling path: the
log-SNR schedules and the per-step scalar coefficients of the DDPM posterior.  These are O(T) scalars per
stage — they are evaluated once on the host (fp32 torch on CPU, exactly the reference's formulas) and
uploaded as a `[T, 8]` table that the sampler kernels index with the device step counter
("precompute per-step scalar table on host").
"""
from __future__ import annotations

import math

import torch
from torch import nn


def beta_linear_log_snr(t: torch.Tensor) -> torch.Tensor:
    """ip.py:212-214."""
    return -torch.log(torch.special.expm1(1e-4 + 10 * (t ** 2)))


def alpha_cosine_log_snr(t: torch.Tensor, s: float = 0.008) -> torch.Tensor:
    """ip.py:216-218 (its log() clamps at 1e-5)."""
    return -torch.log(((torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** -2) - 1).clamp(min=1e-5))


def log_snr_to_alpha_sigma(log_snr: torch.Tensor):
    """ip.py:220-221."""
    return torch.sqrt(torch.sigmoid(log_snr)), torch.sqrt(torch.sigmoid(-log_snr))


COEF_COLS = 8  # [alpha, sigma, alpha_next, sigma_next, c, nonzero, log_snr, guidance scale of the step | 0] — layout shared with csrc/sampler.hip
SOLVERS = ('ddim', 'dpmpp_2m')   # the few-step solvers of Imagen.sample(sampler=...); 'ddpm' is the ancestral step of step_coefficients()


def step_times(steps: int) -> list:
    """The continuous time t of every row of a [steps, 8] table on the grid linspace(1, 0, steps + 1) — the ancestral table of
    step_coefficients() and the solver tables alike — as python floats (steps - i) / steps: t = 1 is pure noise, the last row sits at
    1 / steps.  The quotient of two integers is the double nearest the rational, so a bound a caller writes as 0.2 meets the row at 1 / 5."""
    return [(steps - i) / steps for i in range(steps)]


def check_guidance_interval(interval, what: str = 'guidance_interval') -> tuple:
    """(t_lo, t_hi) as floats, 0 <= t_lo < t_hi <= 1; ValueError otherwise."""
    try:
        lo, hi = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError(f'{what} = {interval!r}: a pair (t_lo, t_hi) of times, t = 1 being pure noise') from None
    if not (0. <= lo <= 1. and 0. <= hi <= 1.):              # (NaN fails both)
        raise ValueError(f'{what} = ({lo}, {hi}) lies outside [0, 1]')
    if not lo < hi:
        raise ValueError(f'{what} = ({lo}, {hi}) is empty: t_lo < t_hi')
    return lo, hi


def guidance_scales(steps: int, cond_scale: float, schedule=None, interval=None, what: str = 'guidance') -> torch.Tensor:
    """The guidance scale of every denoiser evaluation of a stage of `steps` steps, as the fp32 [steps] vector that goes into column 7 of
    the stage's step table (CFG_X0 with cfg == 2).  `schedule`: None (`cond_scale` on every step), a callable f(t) -> float evaluated at
    step_times(steps), or a sequence of exactly `steps` floats.  `interval` = (t_lo, t_hi): the steps with t outside [t_lo, t_hi] run
    unguided, at scale 1.  ValueError for a sequence of another length, a value that is not finite, a bad interval."""
    ts = step_times(steps)
    if schedule is None:
        vals = [float(cond_scale)] * steps
    elif callable(schedule):
        vals = [float(schedule(t)) for t in ts]
    else:
        try:
            vals = [float(v) for v in schedule]
        except TypeError:
            raise ValueError(f'{what}: guidance_schedule is a callable f(t) -> float or a sequence of floats, got {type(schedule).__name__}') from None
        if len(vals) != steps:
            raise ValueError(f'{what}: guidance_schedule has {len(vals)} entries, the stage has {steps} denoiser evaluations.  A sequence of '
                             f'numbers is ONE schedule with an entry per step, for every unet (unlike cond_scale, where a tuple holds one value per '
                             f'unet); one schedule per unet is a tuple of sequences / callables / None, e.g. ([...], None)')
    out = torch.tensor(vals, dtype=torch.float64).float()
    if not bool(torch.isfinite(out).all()):
        raise ValueError(f'{what}: guidance_schedule gives a scale that is not finite (in fp32): {vals}')
    if interval is not None:
        lo, hi = check_guidance_interval(interval, what + ': guidance_interval')
        out[torch.tensor([not lo <= t <= hi for t in ts])] = 1.
    return out


class GaussianDiffusionContinuousTimes(nn.Module):
    def __init__(self, *, noise_schedule, timesteps=1000):
        super().__init__()
        if noise_schedule == "linear":
            self.log_snr = beta_linear_log_snr
        elif noise_schedule == "cosine":
            self.log_snr = alpha_cosine_log_snr
        else:
            raise ValueError(f'invalid noise schedule {noise_schedule}')
        self.noise_schedule = noise_schedule
        self.num_timesteps = timesteps

    def get_times(self, batch_size, noise_level, *, device=None):
        return torch.full((batch_size,), noise_level, device=device, dtype=torch.float32)

    def get_condition(self, times):
        return None if times is None else self.log_snr(times)

    def sample_random_times(self, batch_size, *, device=None):
        """ip.py:239-240."""
        return torch.rand((batch_size,), device=device, dtype=torch.float32)

    def get_sampling_timesteps(self, batch=None, *, device=None):
        """ip.py:245-250: T consecutive (t, t_next) pairs of linspace(1, 0, T+1).  With `batch` (the reference's call) every
        element is a (2, batch) tensor that unpacks into the per-sample `times, times_next`; without it (the coefficient tables
        below) the pairs are fp32 scalars."""
        times = torch.linspace(1., 0., self.num_timesteps + 1, device=device)
        if batch is None:
            return [(times[i], times[i + 1]) for i in range(self.num_timesteps)]
        pairs = torch.stack((times[:-1], times[1:]))                       # (2, T)
        return tuple(pairs[:, i, None].expand(2, batch) for i in range(self.num_timesteps))

    # ---- tensor forms of the reference's scheduler API (ip.py:252-318), for callers that drive single steps themselves
    # (Imagen.p_mean_variance / p_sample below); the sampling loop proper uses the coefficient tables instead
    @staticmethod
    def _per_sample(v: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
        return v.reshape(v.shape + (1,) * (like.ndim - v.ndim)) if v.ndim < like.ndim else v

    def _times(self, t, like: torch.Tensor) -> torch.Tensor:
        if isinstance(t, (int, float)):
            t = torch.full((like.shape[0],), float(t), device=like.device, dtype=like.dtype)
        return t

    def q_posterior(self, x_start, x_t, t, *, t_next=None):
        """Posterior q(x_{t_next} | x_t, x_0): mean, variance and log(variance clamped at 1e-20) (ip.py:252-270)."""
        if t_next is None:
            t_next = (t - 1. / self.num_timesteps).clamp(min=0.)
        l, ln = self._per_sample(self.log_snr(t), x_t), self._per_sample(self.log_snr(t_next), x_t)
        alpha, _ = log_snr_to_alpha_sigma(l)
        alpha_n, sigma_n = log_snr_to_alpha_sigma(ln)
        c = -torch.special.expm1(l - ln)
        mean = alpha_n * (x_t * (1 - c) / alpha + c * x_start)
        var = (sigma_n ** 2) * c
        return mean, var, torch.log(var.clamp(min=1e-20))

    def q_sample(self, x_start, t, noise=None):
        """x_t = alpha_t x_0 + sigma_t eps; also returns log_snr (unpadded), alpha, sigma (ip.py:272-284)."""
        t = self._times(t, x_start)
        if noise is None:
            noise = torch.randn_like(x_start)
        l = self.log_snr(t).type(x_start.dtype)
        alpha, sigma = log_snr_to_alpha_sigma(self._per_sample(l, x_start))
        return alpha * x_start + sigma * noise, l, alpha, sigma

    def q_sample_from_to(self, x_from, from_t, to_t, noise=None):
        """Move a sample between noise levels (the inpainting re-noising, ip.py:286-307)."""
        from_t, to_t = self._times(from_t, x_from), self._times(to_t, x_from)
        if noise is None:
            noise = torch.randn_like(x_from)
        alpha, sigma = log_snr_to_alpha_sigma(self._per_sample(self.log_snr(from_t), x_from))
        alpha_to, sigma_to = log_snr_to_alpha_sigma(self._per_sample(self.log_snr(to_t), x_from))
        return x_from * (alpha_to / alpha) + noise * (sigma_to * alpha - sigma * alpha_to) / alpha

    def predict_start_from_v(self, x_t, t, v):
        """ip.py:309-313."""
        alpha, sigma = log_snr_to_alpha_sigma(self._per_sample(self.log_snr(t), x_t))
        return alpha * x_t - sigma * v

    def predict_start_from_noise(self, x_t, t, noise):
        """ip.py:315-318."""
        alpha, sigma = log_snr_to_alpha_sigma(self._per_sample(self.log_snr(t), x_t))
        return (x_t - sigma * noise) / alpha.clamp(min=1e-8)

    def step_coefficients(self) -> torch.Tensor:
        """[T, 8] fp32 table for the sampler kernels: ip.py:256-268 (posterior), 315-318 (x0), 2162-2163 (nonzero mask)."""
        rows = []
        for t, t_next in self.get_sampling_timesteps():
            l, ln = self.log_snr(t), self.log_snr(t_next)
            alpha, sigma = log_snr_to_alpha_sigma(l)
            alpha_n, sigma_n = log_snr_to_alpha_sigma(ln)
            c = -torch.special.expm1(l - ln)
            nonzero = 0.0 if float(t_next) == 0.0 else 1.0
            rows.append(torch.stack([alpha, sigma, alpha_n, sigma_n, c, torch.tensor(nonzero), l, torch.tensor(0.0)]))
        return torch.stack(rows).float().contiguous()

    def solver_coefficients(self, sampler: str, steps: int, eta: float = 0., *, philox: bool = True, start: int = 0):
        """Tables of the few-step solvers on the grid linspace(1, 0, steps + 1), which is independent of `num_timesteps`:
        (step table [steps, 8] in the layout of step_coefficients() — what CFG_X0, the time embedding and the per-request time table
        read — , weight table [steps, 8] of the LINCOMB update, indexed by the same step counter).

        With l = log_snr(t), (alpha, sigma) from l, lambda = l / 2, h = lambda_next - lambda, c = -expm1(l - l_next):
          'ddim'      x_next = alpha_n x0 + sqrt(sigma_n^2 - s^2) (x - alpha x0) / sigma + nonzero s z,  s = eta sigma_n sqrt(c), 0 <= eta <= 1
                      (eta = 1 is the ancestral posterior of step_coefficients() on this grid, eta = 0 the deterministic DDIM step)
          'dpmpp_2m'  x_next = (sigma_n / sigma) x - alpha_n expm1(-h) D,  D = (1 + 1/(2r)) x0 - (1/(2r)) x0_prev,  r = h_prev / h;
                      D = x0 (first order) on row `start` — the first step of a run has no history — and on the last row.
        x0 and x0_prev are the thresholded estimates.  Weight columns: 0 on x, 1 on thr(x0), 3 on x0_prev, and the noise weight
        nonzero * s in column 4 (the kernel's own Philox draw) when `philox`, else in column 2 (an injected draw passed as t2).

        The grid and its log-SNR are the reference's own fp32 values (get_sampling_timesteps, log_snr): they are what the denoiser is
        conditioned on, and at t = 1 the cosine schedule is decided by the rounding of cos(pi / 2).  Everything derived from l is
        evaluated in fp64 and stored as fp32."""
        if sampler not in SOLVERS:
            raise ValueError(f"unknown solver '{sampler}': one of {SOLVERS}")
        steps, eta = int(steps), float(eta)
        if steps < (2 if sampler == 'dpmpp_2m' else 1):
            raise ValueError(f"'{sampler}' needs at least {2 if sampler == 'dpmpp_2m' else 1} steps, got {steps}")
        if not 0. <= eta <= 1.:
            raise ValueError(f'eta = {eta} is outside [0, 1]')
        if sampler == 'dpmpp_2m' and eta != 0.:
            raise ValueError("'dpmpp_2m' is deterministic: eta must be 0")
        t = torch.linspace(1., 0., steps + 1)
        l = self.log_snr(t).double()
        alpha, sigma = log_snr_to_alpha_sigma(l)
        a, s, a_n, s_n = alpha[:-1], sigma[:-1], alpha[1:], sigma[1:]
        c = -torch.special.expm1(l[:-1] - l[1:])
        nonzero = (t[1:] != 0).double()
        zero = torch.zeros_like(a)
        step = torch.stack([a, s, a_n, s_n, c, nonzero, l[:-1], zero], dim=1)
        w = torch.zeros(steps, COEF_COLS, dtype=torch.float64)
        if sampler == 'ddim':
            # sigma_n^2 - s^2 = sigma_n^2 (1 - eta^2 c), and 1 - c = exp(l - l_next): no difference of nearly equal numbers at c -> 1
            w[:, 0] = s_n * torch.sqrt((1. - eta * eta) + eta * eta * torch.exp(l[:-1] - l[1:])) / s
            w[:, 1] = a_n - a * w[:, 0]
            w[:, 4 if philox else 2] = nonzero * eta * s_n * torch.sqrt(c)
        else:
            h = 0.5 * (l[1:] - l[:-1])
            g = -a_n * torch.special.expm1(-h)
            inv_2r = torch.zeros_like(h)
            inv_2r[1:] = h[1:] / (2. * h[:-1])
            inv_2r[steps - 1] = 0.
            if 0 <= start < steps:
                inv_2r[start] = 0.
            w[:, 0], w[:, 1], w[:, 3] = s_n / s, g * (1. + inv_2r), -g * inv_2r
        return step.float().contiguous(), w.float().contiguous()

    def inpaint_coefficients(self, resample_times: int, philox: bool):
        """Tables for the inpainting resample loop (ip.py:2237-2275), one row per INNER iteration (timestep i, resample r = R-1..0):
        the step table with every row repeated R times, the blend weights of `img*~m + q_sample(known, t)*m` (w0 = alpha_t on the
        known image, sigma_t on the noise) and the re-noising weights of q_sample_from_to(x, t_next -> t) (ip.py:286-307), which are
        the identity on the last resample of a timestep and on the whole last timestep.  The noise weight sits in column 4 (the
        kernel's own Philox draw) when `philox`, else in column 1 (an injected noise image passed as t1)."""
        R = resample_times
        pairs = self.get_sampling_timesteps()
        blend, renoise = [], []
        nz = 4 if philox else 1
        for t, t_next in pairs:
            l, ln = self.log_snr(t), self.log_snr(t_next)
            alpha_t, sigma_t = log_snr_to_alpha_sigma(l)
            alpha_n, sigma_n = log_snr_to_alpha_sigma(ln)
            last_t = float(t_next) == 0.0
            for r in reversed(range(R)):
                b = torch.zeros(8)
                b[0], b[nz] = alpha_t, sigma_t
                blend.append(b)
                q = torch.zeros(8)
                if r == 0 or last_t:
                    q[0] = 1.0
                else:
                    q[0], q[nz] = alpha_t / alpha_n, (sigma_t * alpha_n - sigma_n * alpha_t) / alpha_n
                renoise.append(q)
        step = self.step_coefficients().repeat_interleave(R, dim=0).contiguous()
        return step, torch.stack(blend).float().contiguous(), torch.stack(renoise).float().contiguous()

    def q_sample_coefficients(self, t: float):
        """alpha, sigma of q(x_t | x_0) at noise level t (ip.py:272-284) as python floats (fp32-rounded)."""
        l = self.log_snr(torch.tensor(t, dtype=torch.float32))
        a, s = log_snr_to_alpha_sigma(l)
        return float(a), float(s), float(l)
