"""Drop-in `ElucidatedImagen` (Karras et al. EDM sampler over the same cascaded unets): constructor and `.sample()` signature of the
reference (imagen_pytorch/elucidated_imagen.py:76-745 = "el.py"), sampling half only.  SURVEY.md §8(f) NEXT-1 / BASELINE config C4.

A sampling step is [x_hat = x + churn noise, c_in * x_hat] -> denoiser plan (both CFG branches as one 2B-row batch) -> [CFG
combine + c_skip / c_out preconditioning -> exact 0.95-quantile -> Euler step, c_in * x_next] -> denoiser plan again ->
[preconditioning -> quantile -> Heun combination], all HIP kernels (LINCOMB / CFG_X0 / QUANTILE ops), captured ONCE into a
hipGraph and replayed for every step but the last (which has no second-order correction and its own graph).  The per-evaluation
scalars (c_skip, c_out, c_in, c_noise, step weights) live in device tables indexed by a device counter, so replay needs no host
patching.  Preconditioning is expressed through the existing CFG_X0 "noise" form: c_skip*x + c_out*F = (x - sigma'*F) / alpha'
with alpha' = 1/c_skip, sigma' = -c_out/c_skip.

The one_unet_sample options ride on the same tables: `skip_steps` moves the counter's start row, `init_images` is one add on the
initial noise, per-call `sigma_min` / `sigma_max` select another table set, and inpainting (RePaint resampling, el.py:459-470, 486-545)
repeats every timestep's rows `inpaint_resample_times` times with two extra LINCOMB launches in the same captured sequence — the known
pixels blended into x before the churn noise (x_hat = where(mask, known, x) + noise, el.py:497-498) and x += (sigma - sigma_next) * z
after the Heun combination, with identity weights on the rows where the reference skips it.  Video stages (Unet3D, prompt frames)
as in `Imagen`.  Self-conditioning unets (el.py:496, 518, 538): the Euler op also writes out the clamped model output it sums
(LINCOMB `thr1_out`) — the second evaluation's `self_cond` — and the Heun op that of the second evaluation (`thr3_out`) — the next
step's; both go straight into the engine's `self_cond_in`, which every evaluation packs at its start.  Training (`forward`) raises.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Callable, List, Optional

import torch

from . import ops
from .unet3d import Unet3D
from .imagen import DEFAULT_T5_NAME, Imagen, _cast_tuple, _out_of_scope
from .ops import Plan

Hparams_fields = ['num_sample_steps', 'sigma_min', 'sigma_max', 'sigma_data', 'rho', 'P_mean', 'P_std', 'S_churn', 'S_tmin', 'S_tmax', 'S_noise']
Hparams = namedtuple('Hparams', Hparams_fields)


class ElucidatedImagen(Imagen):
    _lowres_time_raw = True    # el.py:700, 728: the raw augmentation level conditions the unet at sample time

    def __init__(
        self,
        unets,
        *,
        image_sizes,
        text_encoder_name=DEFAULT_T5_NAME,
        text_embed_dim=None,
        channels=3,
        cond_drop_prob=0.1,
        random_crop_sizes=None,
        resize_mode='nearest',
        temporal_downsample_factor=1,
        resize_cond_video_frames=True,
        lowres_sample_noise_level=0.2,
        per_sample_random_aug_noise_level=False,
        condition_on_text=True,
        auto_normalize_img=True,
        dynamic_thresholding=True,
        dynamic_thresholding_percentile=0.95,
        only_train_unet_number=None,
        lowres_noise_schedule='linear',
        num_sample_steps=32,
        sigma_min=0.002,
        sigma_max=80,
        sigma_data=0.5,
        rho=7,
        P_mean=-1.2,
        P_std=1.2,
        S_churn=80,
        S_tmin=0.05,
        S_tmax=50,
        S_noise=1.003,
    ):
        num_unets = len(_cast_tuple(unets))
        steps = _cast_tuple(num_sample_steps, num_unets)
        super().__init__(unets, image_sizes=image_sizes, text_encoder_name=text_encoder_name, text_embed_dim=text_embed_dim, channels=channels,
                         timesteps=steps, cond_drop_prob=cond_drop_prob, random_crop_sizes=random_crop_sizes,
                         lowres_noise_schedule=lowres_noise_schedule, lowres_sample_noise_level=lowres_sample_noise_level,
                         per_sample_random_aug_noise_level=per_sample_random_aug_noise_level, condition_on_text=condition_on_text,
                         auto_normalize_img=auto_normalize_img, dynamic_thresholding=dynamic_thresholding,
                         dynamic_thresholding_percentile=dynamic_thresholding_percentile, only_train_unet_number=only_train_unet_number,
                         temporal_downsample_factor=temporal_downsample_factor, resize_cond_video_frames=resize_cond_video_frames,
                         resize_mode=resize_mode)
        hparams = [num_sample_steps, sigma_min, sigma_max, sigma_data, rho, P_mean, P_std, S_churn, S_tmin, S_tmax, S_noise]
        hparams = [_cast_tuple(hp, num_unets) for hp in hparams]
        self.hparams = [Hparams(*unet_hp) for unet_hp in zip(*hparams)]    # el.py:233-236

    # ---- schedule (el.py:373-391, 428-436) -------------------------------------------------------------------------------
    @staticmethod
    def sample_schedule(num_sample_steps, rho, sigma_min, sigma_max):
        N = num_sample_steps
        inv_rho = 1 / rho
        steps = torch.arange(N, dtype=torch.float32)
        sigmas = (sigma_max ** inv_rho + steps / (N - 1) * (sigma_min ** inv_rho - sigma_max ** inv_rho)) ** rho
        return torch.nn.functional.pad(sigmas, (0, 1), value=0.)

    @staticmethod
    def _row(i: int, r: int, N: int, R: int) -> int:
        """First table row of inner iteration (timestep i, resample r = R-1..0): two rows per iteration (the evaluations at sigma_hat
        and sigma_next) up to the last timestep, whose iterations have no second evaluation and take one row each."""
        k = R - 1 - r
        return 2 * (i * R + k) if i < N - 1 else 2 * (N - 1) * R + k

    def _tables(self, hp: Hparams, R: int = 1):
        """Per-evaluation device tables, fp32 [rows, 8] each: `coef` (CFG_X0 / time embedding: 1/c_skip, -c_out/c_skip, ..., col 6 =
        c_noise), `w_hat` (x_hat op), `w_euler`, `w_heun`, `w_renoise` (LINCOMB weights w0..w5).  Row layout: `_row` — every timestep
        is repeated R times (inpainting with resampling, el.py:486-535; R = 1 otherwise: row 2i / 2i+1 = first / second evaluation of
        step i).  `w_renoise` is read right after the Euler op's advance (second row of an iteration): x += (sigma - sigma_next) * z
        unless r == 0, the identity there."""
        sigmas = self.sample_schedule(hp.num_sample_steps, hp.rho, hp.sigma_min, hp.sigma_max)
        gammas = torch.where((sigmas >= hp.S_tmin) & (sigmas <= hp.S_tmax), min(hp.S_churn / hp.num_sample_steps, math.sqrt(2) - 1), 0.)
        N = hp.num_sample_steps
        sd = hp.sigma_data
        rows = 2 * (N - 1) * R + 2 * R
        coef = torch.zeros(rows, 8, dtype=torch.float64)
        w_hat, w_euler, w_heun, w_renoise = (torch.zeros(rows, 8, dtype=torch.float64) for _ in range(4))
        w_renoise[:, 0] = 1.0

        def precond(row, sigma):   # el.py:323-336
            c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
            c_out = sigma * sd * (sd ** 2 + sigma ** 2) ** -0.5
            coef[row, 0], coef[row, 1], coef[row, 6] = 1.0 / c_skip, -c_out / c_skip, math.log(max(sigma, 1e-20)) * 0.25

        for i in range(N):
            sigma, sigma_next, gamma = sigmas[i].item(), sigmas[i + 1].item(), gammas[i].item()
            sigma_hat = sigma + gamma * sigma
            for rs in range(R):
                e = self._row(i, rs, N, R)
                precond(e, sigma_hat)
                w_hat[e, 0] = 1.0
                w_hat[e, 4] = math.sqrt(sigma_hat ** 2 - sigma ** 2) * hp.S_noise          # el.py:489-492
                w_hat[e, 5] = (sigma_hat ** 2 + sd ** 2) ** -0.5                              # c_in(sigma_hat)
                ratio = sigma_next / sigma_hat
                w_euler[e, 0], w_euler[e, 1] = ratio, 1.0 - ratio                             # x_hat + (s_n - s_h)(x_hat - x0)/s_h
                if sigma_next != 0:
                    precond(e + 1, sigma_next)
                    w_euler[e, 5] = (sigma_next ** 2 + sd ** 2) ** -0.5                       # c_in(sigma_next)
                    d = 0.5 * (sigma_next - sigma_hat)
                    w_heun[e + 1, 0], w_heun[e + 1, 1] = 1.0 + d / sigma_hat, -d / sigma_hat
                    w_heun[e + 1, 2], w_heun[e + 1, 3] = d / sigma_next, -d / sigma_next      # el.py:528-529
                    if rs > 0:                                                                # el.py:532-535 (never at the last timestep)
                        w_renoise[e + 1, 4] = sigma - sigma_next
        return sigmas[0].item(), [t.float().contiguous() for t in (coef, w_hat, w_euler, w_heun, w_renoise)]

    # ---- per-stage plans --------------------------------------------------------------------------------------------------
    def _build_stage(self, idx: int, B: int, device, *, cond_scale: float, with_text: bool, inject_noise: bool, sample_offset: int,
                     resample_times: int = 0, frames: int = 0, prompt_frames: tuple = (0, 0), sigma_overrides: Optional[dict] = None, size=None):
        unet = self.unets[idx]
        size = self.image_sizes[idx] if size is None else size      # (an int, or (H, W): Imagen.sample(image_shapes=...))
        hp = self.hparams[idx]
        if sigma_overrides is not None:                  # sample(sigma_min=, sigma_max=), el.py:425-426, 647-648
            hp = hp._replace(**{k: v[idx] for k, v in sigma_overrides.items() if v[idx] is not None})
        cfg = cond_scale != 1.
        R = resample_times
        key = ("edm", idx, B, size, str(device), float(cond_scale), with_text, inject_noise, sample_offset,
               self.dynamic_thresholding[idx], self.dynamic_thresholding_percentile, tuple(hp), frames, prompt_frames, R, self._lane)

        def tables():                                    # `_tables` on the device, then w_init = (sigma_0, 0, ...), the scale of the initial noise
            init_sigma, tabs = self._tables(hp, max(R, 1))
            w_init = torch.zeros(1, 8, device=device)
            w_init[0, 0] = init_sigma
            return [t.to(device) for t in tabs] + [w_init]

        # (the time table of an image stage has this sampler's 2T evaluation rows: both denoiser evaluations of a step read it)
        st, built = self._new_stage(key, idx, B, device, cfg=cfg, with_text=with_text, inject_noise=inject_noise, sample_offset=sample_offset,
                                    resample_times=R, frames=frames, prompt_frames=prompt_frames, tables=tables, size=size)
        if not built:
            return st
        eng, n, dev, step_ptr, seed_dev, step_plan, noise, final = (st['eng'], st['n'], device, st['step_ptr'], st['seed_dev'], st['step_plan'],
                                                                    st['noise'], st['final'])
        # self-conditioning (el.py:496, 518, 538): every evaluation packs `sc`; the Euler op leaves the first evaluation's clamped output in
        # it for the Heun evaluation, the Heun op the second one's for the next step (or the next resample of the same timestep)
        sc = eng.self_cond_in if getattr(unet, 'self_cond', False) else None
        assert sc is None or sc.numel() == B * n
        coef, w_hat, w_euler, w_heun, w_renoise, w_init = st['tables']
        if inject_noise:   # the churn noise comes in through t1 (weight col 1) instead of the in-kernel Philox stream (col 4)
            for w in (w_hat, w_renoise):
                w[:, 1] = w[:, 4]
                w[:, 4] = 0
        mk = lambda: torch.empty_like(eng.x_in)
        x, xhat, xnext, x0a, x0b, absx0 = mk(), mk(), mk(), mk(), mk(), mk()
        qa, qb = torch.empty(B, device=dev), torch.empty(B, device=dev)
        W = ops.ENUMS["IMAGEN_QUANTILE_SCRATCH_WORDS"]
        scr_a, scr_b = (torch.empty(B * W, dtype=torch.int32, device=dev) for _ in range(2))
        dyn = bool(self.dynamic_thresholding[idx])
        thr = 1 if dyn else 2                      # clamp=True (el.py:399): dynamic threshold, else clamp to [-1, 1]
        q = float(self.dynamic_thresholding_percentile)
        kw = dict(B=B, n_per_sample=n, stream_id=idx, sample_offset=sample_offset, seed_ptr=seed_dev)

        w_one = torch.zeros(1, 8, device=dev)
        w_one[0, 0] = 1.0
        zero_ptr = torch.zeros(1, dtype=torch.int32, device=dev)

        def first_eval(plan):
            if R:   # inpainting (el.py:459-470, 497-498): x_hat = where(mask, known, x) + added noise — the known pixels go into x first
                ops.lincomb(plan, st['known'], x, w_one, zero_ptr, mask=st['mask'], mask_else=x, label="edm.inpaint.blend", **kw)
            ops.lincomb(plan, x, xhat, w_hat, step_ptr, t1=noise, out2=eng.x_in, label="edm.x_hat", **kw)
            plan.extend(step_plan)
            ops.cfg_x0(plan, xhat, eng.out, coef, step_ptr, x0a, absx0, B=B, n_per_sample=n, cfg=cfg, cond_scale=float(cond_scale),
                       objective="noise", label="edm.precond")
            if dyn:
                ops.quantile(plan, absx0, qa, scr_a, B=B, n=n, q=q)

        full = Plan(f"edm-stage{idx}-step")
        first_eval(full)
        ops.lincomb(full, xhat, xnext, w_euler, step_ptr, t1=x0a, q1=qa if dyn else None, out2=eng.x_in, thr_mode=thr, advance=True,
                    thr1_out=sc, label="edm.euler", **kw)
        full.extend(step_plan)
        ops.cfg_x0(full, xnext, eng.out, coef, step_ptr, x0b, absx0, B=B, n_per_sample=n, cfg=cfg, cond_scale=float(cond_scale),
                   objective="noise", label="edm.precond2")
        if dyn:
            ops.quantile(full, absx0, qb, scr_b, B=B, n=n, q=q)
        ops.lincomb(full, xhat, x, w_heun, step_ptr, t1=x0a, t2=xnext, t3=x0b, q1=qa if dyn else None, q3=qb if dyn else None,
                    thr_mode=thr, advance=not R, thr3_out=sc, label="edm.heun", **kw)
        if R:   # RePaint re-noising before the next resample of the same timestep (identity weights where the reference skips it)
            ops.lincomb(full, x, x, w_renoise, step_ptr, t1=st['noise_renoise'], advance=True, label="edm.inpaint.renoise",
                        **{**kw, "stream_id": idx | 0x200})

        last = Plan(f"edm-stage{idx}-last")       # sigma_next = 0: Euler step only, then clamp + unnormalise (el.py:515, 540-545)
        # self-conditioning: it reads what the preceding Heun op left, and only with resampling, where the last timestep runs again on
        # this evaluation's output (el.py:538), leaves anything behind
        first_eval(last)
        ops.lincomb(last, xhat, x, w_euler, step_ptr, t1=x0a, q1=qa if dyn else None, thr_mode=thr, final=True, final_out=final,
                    advance=True, thr1_out=sc if R > 1 else None, label="edm.euler.final", **kw)

        init_scale = Plan("edm-init-scale")             # images = init_sigma * randn (el.py:440-442; sigma_0 also when steps are skipped)
        ops.lincomb(init_scale, x, x, w_init, zero_ptr, B=B, n_per_sample=n)
        st.update(plan=full, last=last, graph_last=None, T=hp.num_sample_steps, x=x, w_init=w_init, zero_ptr=zero_ptr, init_scale=init_scale,
                  tables=(w_hat, w_euler, w_heun, w_renoise, w_one), self_cond=sc, bufs=(xhat, xnext, x0a, x0b, absx0, qa, qb, scr_a, scr_b))
        self._stages[key] = st
        return st

    # ---- what this sampler puts into Imagen._run_stage (el.py:393-545 for one stage) ------------------------------------------------
    _per_row_noise_keys = False    # the churn and re-noising launches (LINCOMB) take one key per batch
    _plan_prefix = 'edm-'
    _step_noun = 'step'

    def _rewind(self, st, skip: int, init_images):
        """x = sigma_0 * randn (+ init_images), no x_start, the counter on the first row of step `skip`."""
        st['init_scale'].run()
        if init_images is not None:
            st['x'].add_(init_images)                    # el.py:446-447
        if st['self_cond'] is not None:
            st['self_cond'].zero_()                      # el.py:451: x_start = None (also after the warm-up and when steps are skipped)
        st['step_ptr'].fill_(self._row(skip, max(st['R'], 1) - 1, st['T'], max(st['R'], 1)))   # el.py:477-479: the skipped steps are never run

    def _plans_of_steps(self, st, steps: range) -> list:
        """The last step (sigma_next = 0) has no second-order correction: its own plan and graph."""
        return [(st, 'last' if i == st['T'] - 1 else 'plan') for i in steps]

    def _capture(self, st, plans: list, rewind, stream):
        if st['graph'] is not None:
            return
        if st['noise'] is not None:
            st['noise'].zero_()
            if st['R']:
                st['noise_renoise'].zero_()
        # warm-up outside capture (kernel attributes), then rewind.  Both plans run from table row 0: `plan` advances the device
        # step counter by its two evaluations, and started from the last timestep's rows (skip_steps = T - 1) `last` would read past
        # the 2T-row tables (the kernels do not clamp *step_ptr) and `plan` would feed the all-zero final row into CFG_X0
        st['step_ptr'].zero_()
        st['plan'].run()
        st['step_ptr'].zero_()
        st['last'].run()
        torch.cuda.synchronize()
        st['graph'] = ops.Graph(st['plan'], stream)
        st['graph_last'] = ops.Graph(st['last'], stream)
        rewind()

    def _draw_step_noise(self, st, draw, stage: int, i: int, r: int):
        st['noise'].copy_(draw(("step", stage, i, r) if st['R'] else ("step", stage, i), st['noise']))
        if st['R'] and r > 0 and i < st['T'] - 1:        # the reference draws no re-noising sample otherwise (el.py:532)
            st['noise_renoise'].copy_(draw(("renoise", stage, i, r), st['noise']))

    # ---- public sampling API (el.py:547-745) ---------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(
        self,
        texts: Optional[List[str]] = None,
        text_masks=None,
        text_embeds=None,
        cond_images=None,
        cond_video_frames=None,
        post_cond_video_frames=None,
        inpaint_videos=None,
        inpaint_images=None,
        inpaint_masks=None,
        inpaint_resample_times=5,
        init_images=None,
        skip_steps=None,
        sigma_min=None,
        sigma_max=None,
        video_frames=None,
        batch_size=1,
        cond_scale=1.,
        lowres_sample_noise_level=None,
        start_at_unet_number=1,
        start_image_or_video=None,
        stop_at_unet_number=None,
        return_all_unet_outputs=False,
        return_pil_images=False,
        use_tqdm=True,
        use_one_unet_in_gpu=True,
        device=None,
        *,
        noise_fn: Optional[Callable] = None,   # extensions, as on Imagen.sample
        seed: Optional[int] = None,
        sample_offset: int = 0,
        use_graph: bool = True,
        max_steps: Optional[int] = None,
        conditioning=None,
        negative_texts: Optional[List[str]] = None,   # a second prompt on the null rows of guidance, as on Imagen.sample
        negative_text_embeds=None,
        negative_text_masks=None,
        image_shapes=None,                            # one (H, W) per unet for this call, as on Imagen.sample
        sampler=None,                                 # Imagen.sample's solver keywords: refused here (ValueError), this class has its own sampler
        sample_steps=None,
        eta=None,
        guidance_schedule=None,                       # Imagen.sample's guidance keywords: refused here (ValueError)
        guidance_interval=None,
        guidance_rescale=None,
        guidance_apg=None,
        compose=None,                                 # Imagen.sample's composed prompts: refused here (ValueError)
        compose_mask=None,
        tile_shapes=None,                             # Imagen.sample's tiled sampling: refused here (ValueError)
        tile_overlap=None,
        tile_blend=None,
    ):
        return self._sample(self._call(**{k: v for k, v in locals().items() if k != 'self'}))   # (the keywords, as given)

    # Imagen.sample's keywords that are not this sampler's (SampleCall._preflight).  A Heun step evaluates the denoiser twice per table row, so
    # a per-row scale, a per-step choice of plan and the running average of projected guidance — a state per evaluation of a first-order
    # step — are not what Imagen's are; this sampler guides with the plain extrapolation at the fixed cond_scale.
    _twice = 'ElucidatedImagen evaluates the denoiser twice per step of its second-order sampler'
    _refused_keywords = (
        (('sampler', 'sample_steps', 'eta'), 'ElucidatedImagen samples with its own second-order sampler (num_sample_steps); the solver keywords belong to Imagen.sample'),
        (('guidance_schedule', 'guidance_interval'), _twice + '; guidance schedules and intervals belong to Imagen.sample'),
        (('guidance_rescale', 'guidance_apg'), _twice + '; guidance rescale and projected guidance belong to Imagen.sample'),
        (('compose', 'compose_mask'), _twice + ' on the two-branch plan; composed prompts belong to Imagen.sample', 'compose'),
        (('tile_shapes', 'tile_overlap', 'tile_blend'), _twice + ', each on the whole canvas; tiled sampling belongs to Imagen.sample', 'tile_shapes'),
    )

    def _call(self, sigma_min=None, sigma_max=None, **kw):
        """Imagen._call behind the pre-flight (the refused keywords never make a record); this sampler's two extra keywords become the
        record's per-unet `sigma_overrides`, which `_build_stage` takes."""
        self._preflight(**kw)
        n_unets = len(self.unets)
        over = None if sigma_min is None and sigma_max is None else dict(sigma_min=_cast_tuple(sigma_min, n_unets),
                                                                         sigma_max=_cast_tuple(sigma_max, n_unets))
        return super()._call(sigma_overrides=over, **kw)
