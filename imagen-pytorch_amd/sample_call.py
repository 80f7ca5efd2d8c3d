"""The keyword layer of `sample()`: the record of one call (`_Call`) and `SampleCall`, the mixin of `Imagen` that turns the public keywords
into a resolved record.  Host Python alone: nothing here builds a stage, touches a plan or launches a kernel.  `_call(**keywords)` makes the
record, `_resolve` fills it:
  * first `_preflight`, the checks that need no batch, device or text — the keywords a sampler refuses outright (`_refused_keywords`), the solver,
    the guidance schedule / interval, guidance rescale / projected guidance.  `sample_requests` runs it on its common keywords before it encodes
    text or draws a seed, `ElucidatedImagen._call` before it makes the record; `sample_pipelined` checks a batch by `_resolve` of the
    whole-cascade call, so every entry refuses what `sample()` refuses;
  * then, in an order the refusals of a call with several faults depend on: sizes, device, text and batch, inpainting inputs, the per-unet tuples,
    the guidance vectors, `_check_guide`, composed prompts, tiled sampling (`_tiles_of`; its geometry and window weights are `tile_origins`,
    `tile_window`, `tile_geometry` below), the seed, the negative prompt, the start image.
What the resolvers share exists once: `per_unet`, `is_number`, `stage_range`, `_cannot_guide`, `_needs_text_branch`, `_refuse_inpainting`.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Callable, List, Optional

import torch

from . import ops
from .unet import Unet, check_negative_prompt
from .unet3d import Unet3D

GUIDANCE_KEYWORDS = ('guidance_schedule', 'guidance_interval', 'guidance_rescale', 'guidance_apg')


def _cast_tuple(val, length=None):
    if isinstance(val, list):
        val = tuple(val)
    out = val if isinstance(val, tuple) else ((val,) * (length or 1))
    if length is not None:
        assert len(out) == length
    return out


class Conditioning:
    """Handle on the timestep-invariant conditioning of a batch of prompts (SURVEY.md §8(f) NEXT-3).

    Everything the denoiser derives from the text alone — projected tokens, Perceiver-pooled latents, the non-attention text
    hidden, and the cross-attention K/V of every site (ip.py:1595-1660, 793-808) — is computed by the engines' static plan,
    once per `sample()` call.  Passing the SAME handle to several `sample(conditioning=...)` calls (more seeds for the same
    prompts, `start_at_unet_number` re-runs, ...) lets each stage keep what its static plan wrote the first time: the engine
    buffers are stamped with the handle's token and the static plan is skipped while the stamp matches."""

    def __init__(self, text_embeds: Optional[torch.Tensor], text_masks: Optional[torch.Tensor], batch_size: int,
                 negative_text_embeds: Optional[torch.Tensor] = None, negative_text_masks: Optional[torch.Tensor] = None):
        self.text_embeds, self.text_masks, self.batch_size = text_embeds, text_masks, batch_size
        self.negative_text_embeds, self.negative_text_masks = negative_text_embeds, negative_text_masks   # the negative prompt rides along
        self.token = object()


@dataclasses.dataclass
class _Call:
    """One sample() call: the public keywords as given (the defaults are sample()'s), what the callers inside the package add, and — once
    `SampleCall._resolve` has run — what was resolved from them, in place: `device` a torch.device, `text_embeds` / `text_masks` / `cond_images` on
    it, `batch_size` the rows, `cond_scale` / `skip_steps` one entry per unet, `init_images` a normalised list, `seed` drawn.  It is handed
    from `_resolve` to `_prepare_stage` to the stage loop; nothing of a call lives anywhere else."""
    texts: Any = None
    text_masks: Any = None
    text_embeds: Any = None
    video_frames: Any = None
    cond_images: Any = None
    cond_video_frames: Any = None
    post_cond_video_frames: Any = None
    inpaint_videos: Any = None
    inpaint_images: Any = None
    inpaint_masks: Any = None
    inpaint_resample_times: int = 5
    init_images: Any = None
    skip_steps: Any = None
    batch_size: int = 1
    cond_scale: Any = 1.
    lowres_sample_noise_level: Any = None
    start_at_unet_number: int = 1
    start_image_or_video: Any = None
    stop_at_unet_number: Any = None
    return_all_unet_outputs: bool = False
    return_pil_images: bool = False
    device: Any = None
    use_tqdm: bool = True
    use_one_unet_in_gpu: bool = True
    noise_fn: Optional[Callable] = None
    seed: Any = None
    sample_offset: int = 0
    use_graph: bool = True
    max_steps: Optional[int] = None
    conditioning: Optional[Conditioning] = None
    negative_texts: Any = None
    negative_text_embeds: Any = None
    negative_text_masks: Any = None
    image_shapes: Any = None                           # extension: one (H, W) per unet, overriding image_sizes for this call (image cascades)
    sampler: Any = None                                # extension: 'ddpm' (None: the same) | 'ddim' | 'dpmpp_2m' — SampleCall._solver_of
    sample_steps: Any = None                           # ... solver steps, an int or one per unet (None: that unet's timesteps)
    eta: Any = None                                    # ... 'ddim' only, 0 (None: the same) .. 1
    guidance_schedule: Any = None                      # extension: the guidance scale per step, a callable f(t) | a sequence, one or per unet
    guidance_interval: Any = None                      # ... (t_lo, t_hi), one or per unet: the steps outside it run unguided — SampleCall._guidance_of
    guidance_rescale: Any = None                       # extension: phi of guidance rescale, one or per unet — SampleCall._guide_of
    guidance_apg: Any = None                           # ... dict(eta=, norm_threshold=, momentum=) of projected guidance, one or per unet
    compose: Any = None                                # extension: further prompts, [dict(text_embeds= | texts=, text_masks=, weight=, mask=), ...] — SampleCall._compose_of
    compose_mask: Any = None                           # ... the main prompt's mask, [B | 1, H, W] or [H, W] in [0, 1]
    tile_shapes: Any = None                            # extension: tiled sampling, the (h, w) window of the denoiser, one or per unet (None: untiled) — SampleCall._tiles_of
    tile_overlap: Any = None                           # ... an int or (oy, ox), one or per unet (None: a quarter of the tile side)
    tile_blend: Any = None                             # ... the window: 'ramp' (None: the same) | 'uniform'
    # not public keywords: set by sample_requests, the sample_pipelined workers and ElucidatedImagen._call
    negative_rows: Optional[torch.Tensor] = None       # bool [rows]: the samples the merged negative prompt applies to
    pipelined_stage: bool = False                      # one stage of a cascade whose guidance scales sample_pipelined has checked as a whole
    sigma_overrides: Optional[dict] = None             # ElucidatedImagen.sample(sigma_min=, sigma_max=): one entry per unet each
    # resolved
    negative: Optional[tuple] = None                   # the negative prompt as _negative_of_call returns it
    neg_embeds: Any = None                             # ... resolved and checked (_check_negative)
    neg_masks: Any = None
    neg_rows: Any = None
    solver: Any = None                                 # None (the ancestral sampler), or per unet (sampler, steps, eta)
    guidance: Any = None                               # per unet: None (cond_scale as it stands) | the fp32 [steps] scales of a schedule that varies
    guide: Any = None                                  # None, or per unet: None | ('rescale', phi) | ('apg', eta, norm_threshold, momentum)
    composed: Any = None                               # None, or dict(K, prompts [(embeds, masks)] of the prompts 1 .. K - 1, weights per unet fp32 [K, B], masks None | K x (None | fp32 [B | 1, H, W]))
    tiles: Any = None                                  # None, or per unet: None | tile_geometry(...) of the stage's canvas
    sizes: Any = None                                  # per unet: image_sizes[i] (int, square), or (H, W) where image_shapes says H != W
    frames: int = 0                                    # video_frames of a video cascade, else 0
    known: Any = None                                  # inpainting: the normalised known image / clip (reference layout) and its mask
    known_mask: Any = None
    level: float = 0.                                  # low-res augmentation level
    img: Any = None                                    # the hand-off image (internal layout, [0, 1]): start_image_or_video, then each stage's output


def _seed_spans(seed, batch: int, sample_offset: int = 0):
    """[(Philox seed, first row, rows, global index of the first row)]: an int seed is one span over the whole batch; a list of (seed, rows)
    pairs — merged requests (Imagen.sample_requests) — one span per request, each with sample indices restarting at 0."""
    if isinstance(seed, (list, tuple)):
        spans, r0 = [], 0
        for sd, cnt in seed:
            spans.append((int(sd), r0, int(cnt), 0))
            r0 += int(cnt)
        assert r0 == batch, f'merged requests cover {r0} rows, the batch has {batch}'
        return spans
    return [(int(seed), 0, batch, sample_offset)]


# ---- tiled sampling: the geometry and the window weights of one stage (host code; the kernel side is TILES, include/imagen_hip.h) ----
TILE_BLENDS = ('ramp', 'uniform')


def tile_origins(N: int, L: int, o: int) -> list:
    """The tile origins along one axis of length N for tiles of length L at overlap o (0 <= o < L), stride s = L - o: 0, s, 2 s, ... while
    < N - L, then N - L — the last tile is clamped to the canvas, so its overlap may be larger.  N == L: one tile."""
    if N < L:
        raise ValueError(f'a tile side of {L} is larger than the canvas side of {N}')
    if not 0 <= o < L:
        raise ValueError(f'an overlap of {o} is outside [0, {L}) (the tile side)')
    return [*range(0, N - L, L - o), N - L]


def tile_window(L: int, o: int, blend: str) -> torch.Tensor:
    """The fp64 window of one axis: 'uniform' 1; 'ramp' min(i + 1, L - i, o + 1) / (o + 1) — linear over the overlap at both ends, 1 between."""
    if blend == 'uniform':
        return torch.ones(L, dtype=torch.float64)
    i = torch.arange(L, dtype=torch.float64)
    return torch.minimum(torch.minimum(i + 1, L - i), torch.tensor(o + 1., dtype=torch.float64)) / (o + 1)


def tile_geometry(H: int, W: int, h: int, w: int, oy: int, ox: int, blend: str = 'ramp') -> dict:
    """The tiles of an H x W canvas: dict(h, w, oy, ox, blend, Ty, Tx, T, origins int32 [T, 2] = (y0, x0) in row-major tile order (y outer), nw
    fp32 [T, h * w]).  nw[t][p] = w_t(p) / sum_s w_s(p) with the separable window w_y(i) w_x(j), computed in fp64 and rounded to fp32: exactly
    1.0 where one tile covers the pixel.  Raises ValueError as tile_origins does."""
    if blend not in TILE_BLENDS:
        raise ValueError(f"tile_blend = {blend!r}: {' | '.join(repr(b) for b in TILE_BLENDS)}")
    ys, xs = tile_origins(H, h, oy), tile_origins(W, w, ox)
    win = tile_window(h, oy, blend)[:, None] * tile_window(w, ox, blend)[None, :]
    origins = [(y0, x0) for y0 in ys for x0 in xs]
    total = torch.zeros(H, W, dtype=torch.float64)
    for y0, x0 in origins:
        total[y0:y0 + h, x0:x0 + w] += win
    nw = torch.stack([win / total[y0:y0 + h, x0:x0 + w] for y0, x0 in origins]).to(torch.float32)
    return dict(h=h, w=w, oy=oy, ox=ox, blend=blend, Ty=len(ys), Tx=len(xs), T=len(origins),
                origins=torch.tensor(origins, dtype=torch.int32), nw=nw.reshape(len(origins), h * w).contiguous())


# ---- what every resolver shares ---------------------------------------------------------------------------------------------------
def is_number(v, bools: bool = False) -> bool:
    """A Python number or a 0-d tensor.  bools: whether True / False count — among the entries of a guidance schedule they do, as they always
    have ([True, 2.] is the schedule [1., 2.]); a rescale phi, a setting of projected guidance and a compose weight refuse them."""
    return (isinstance(v, (int, float)) and (bools or not isinstance(v, bool))) or (isinstance(v, torch.Tensor) and v.ndim == 0)


def per_unet(val, kw: str, n: int, is_one: Callable, entry: str = 'one entry (or None)') -> tuple:
    """A keyword that takes one value for every unet (None, or whatever `is_one` admits) or a tuple / list with one entry per unet -> the
    n entries.  entry: how the refusal of anything else words the second choice."""
    if val is None or is_one(val):
        return (val,) * n
    if not isinstance(val, (list, tuple)):
        raise ValueError(f'{kw} = {val!r}: one value, or a tuple with {entry} per unet')
    if len(val) != n:
        raise ValueError(f'{kw}: {len(val)} entries for {n} unets (one entry, or None, per unet)')
    return tuple(val)


def stage_range(c: _Call, n_unets: int) -> tuple:
    """(first, last): the stages [first, last) a call runs."""
    return c.start_at_unet_number - 1, n_unets if c.stop_at_unet_number is None else c.stop_at_unet_number


class SampleCall:
    """What turns the keywords of `sample()` into a resolved `_Call`, as a mixin of `Imagen`: it reads the model (`unets`, `noise_schedulers`,
    `image_sizes`, `encode_text`, ...) and the image helpers `Imagen` keeps for its stage side (`_sampling_device`, `_to_internal`, `_resize`,
    `normalize_img`), and writes nothing but the record and the seed counter."""

    # (keywords, reason[, prefix]): the keyword groups this sampler refuses outright, with a ValueError '<the given ones, joined by ", "
    # — or the fixed prefix>: <reason>'.  Empty here; ElucidatedImagen lists Imagen's solver, guidance and compose keywords.
    _refused_keywords: tuple = ()

    def _call(self, **kw) -> _Call:
        """The record of one call from sample()'s keywords (+ the private ones of _Call)."""
        return _Call(**kw)

    def _cannot_guide(self, kw: str, dropout: Optional[str] = None, text: Optional[str] = None, no_text: bool = False):
        """The two refusals of a model that cannot guide: trained without conditional dropout ('... and <dropout>'), built without a text branch
        — or (no_text) called without text — ('... there is no text branch to <text>').  A tail of None skips that refusal."""
        if dropout is not None and not self.can_classifier_guidance:
            raise ValueError(f'{kw}: imagen was not trained with conditional dropout (cond_drop_prob == 0) and {dropout}')
        if text is not None and (self.unconditional or no_text):
            raise ValueError(f'{kw}: this model was built with condition_on_text=False, there is no text branch to {text}')

    def _needs_text_branch(self, idx: int, kw: str, verb: str):
        if not getattr(self.unets[idx], 'cond_on_text', False):
            raise ValueError(f'{kw}: unet {idx + 1} has no text branch (cond_on_text=False), there is nothing to {verb}')

    @staticmethod
    def _refuse_inpainting(c: _Call, what: str, why: str):
        if c.inpaint_images is not None or c.inpaint_videos is not None or c.inpaint_masks is not None:
            raise ValueError(f'{what} with inpainting: the resample loop (ip.py:2237-2275) {why}')

    # ---- the pre-flight: no batch, no device, no text
    def _preflight(self, **kw) -> tuple:
        """Every check of a call's keywords (`kw`: as given, whatever else is among them) that needs no batch, device or text, so that it can
        come before any text is encoded or any seed drawn.  Returns what `_solver_of`, `_guidance_of` and `_guide_of` return."""
        for keywords, reason, *prefix in self._refused_keywords:
            given = [k for k in keywords if kw.get(k) is not None]
            if given:
                raise ValueError(f"{prefix[0] if prefix else ', '.join(given)}: {reason}")
        return (self._solver_of(kw.get('sampler'), kw.get('sample_steps'), kw.get('eta')),
                self._guidance_of(kw.get('guidance_schedule'), kw.get('guidance_interval')),
                self._guide_of(kw.get('guidance_rescale'), kw.get('guidance_apg')))

    def _solver_of(self, sampler=None, sample_steps=None, eta=None):
        """The solver keywords of one call, checked: None for the ancestral sampler ('ddpm', the default: one step per training timestep),
        else one (sampler, steps, eta) per unet — `sample_steps` an int or one per unet, None meaning that unet's `timesteps`.  Raises
        ValueError for an unknown sampler, `sample_steps` / `eta` beside 'ddpm', eta outside [0, 1] or beside the deterministic
        'dpmpp_2m', and fewer steps than the solver's order."""
        from .schedules import SOLVERS

        sampler = 'ddpm' if sampler is None else sampler
        eta = 0. if eta is None else float(eta)
        if sampler == 'ddpm':
            if sample_steps is not None or eta != 0.:
                raise ValueError("sample_steps / eta belong to the solvers (sampler='ddim' | 'dpmpp_2m'): the ancestral sampler 'ddpm' runs "
                                 "every training timestep (Imagen(timesteps=...)) and draws its posterior noise")
            return None
        if sampler not in SOLVERS:
            raise ValueError(f"unknown sampler '{sampler}': 'ddpm', {', '.join(repr(s) for s in SOLVERS)}")
        if not 0. <= eta <= 1.:
            raise ValueError(f'eta = {eta} is outside [0, 1]')
        if sampler == 'dpmpp_2m' and eta != 0.:
            raise ValueError("sampler='dpmpp_2m' is deterministic: eta must be 0 ('ddim' takes 0 <= eta <= 1)")
        n = len(self.unets)
        steps = tuple(sample_steps) if isinstance(sample_steps, (list, tuple)) else (sample_steps,) * n
        if len(steps) != n:
            raise ValueError(f'sample_steps: {len(steps)} entries for {n} unets')
        steps = tuple(sched.num_timesteps if s is None else int(s) for s, sched in zip(steps, self.noise_schedulers))
        least = 2 if sampler == 'dpmpp_2m' else 1
        if min(steps) < least:
            raise ValueError(f"sampler='{sampler}' needs sample_steps >= {least}, got {steps}")
        return tuple((sampler, s, eta) for s in steps)

    def _guidance_of(self, guidance_schedule=None, guidance_interval=None):
        """The guidance keywords of one call, per unet and checked as far as that goes without the step counts: None when neither is given,
        else (schedules, intervals), one entry per unet each — a schedule None, a callable or a list of floats, an interval None or a
        checked (t_lo, t_hi).  A sequence of numbers is ONE schedule (a pair of numbers ONE interval) and serves every unet; a tuple whose
        entries are None, callables or sequences holds one per unet.  Raises ValueError where the keywords cannot act: a model trained
        without conditional dropout, or without a text branch (the conditions of _check_negative)."""
        from .schedules import check_guidance_interval

        if guidance_schedule is None and guidance_interval is None:
            return None
        n = len(self.unets)
        flat = lambda v: isinstance(v, torch.Tensor) and v.ndim == 1 or (isinstance(v, (list, tuple)) and len(v) > 0 and all(is_number(e, bools=True) for e in v))
        one = lambda v: callable(v) or flat(v)
        schedules = tuple(s if s is None or callable(s) else [float(v) for v in s] if flat(s) else s
                          for s in per_unet(guidance_schedule, 'guidance_schedule', n, one, entry='one entry'))
        for i, s in enumerate(schedules):
            if not (s is None or callable(s) or isinstance(s, list)):
                raise ValueError(f'guidance_schedule[{i}] = {s!r}: None, a callable f(t) -> float or a sequence of floats')
        intervals = tuple(None if v is None else check_guidance_interval(v, f'guidance_interval[{i}]')
                          for i, v in enumerate(per_unet(guidance_interval, 'guidance_interval', n, one, entry='one entry')))
        self._cannot_guide('guidance_schedule' if guidance_schedule is not None else 'guidance_interval',
                           'cannot do classifier free guidance', 'guide')
        return schedules, intervals

    def _guide_of(self, guidance_rescale=None, guidance_apg=None):
        """`guidance_rescale` / `guidance_apg` of one call, per unet and checked as far as that goes without the guidance scales: None when
        neither is given, else one entry per unet — None, ('rescale', phi) or ('apg', eta, norm_threshold, momentum) with norm_threshold 0.
        for "no cap".  One value serves every unet; a tuple holds one entry (or None) per unet.  Raises ValueError for malformed values,
        both keywords on one unet, a model trained without conditional dropout or without a text branch."""
        if guidance_rescale is None and guidance_apg is None:
            return None
        n = len(self.unets)

        def finite(v, what, none_ok=False):
            if v is None and none_ok:
                return 0.
            if not is_number(v) or not math.isfinite(float(v)):
                raise ValueError(f'{what} = {v!r}: a finite number')
            return float(v)

        out = []
        for i, (phi, apg) in enumerate(zip(per_unet(guidance_rescale, 'guidance_rescale', n, is_number),
                                           per_unet(guidance_apg, 'guidance_apg', n, lambda v: isinstance(v, dict)))):
            if phi is not None and apg is not None:
                raise ValueError(f'guidance_rescale and guidance_apg are both given for unet {i + 1}: a stage takes one of them')
            if phi is not None:
                phi = finite(phi, f'guidance_rescale[{i}]')
                if not 0. <= phi <= 1.:
                    raise ValueError(f'guidance_rescale[{i}] = {phi} is outside [0, 1]')
                out.append(('rescale', phi))
            elif apg is not None:
                if not isinstance(apg, dict) or set(apg) - {'eta', 'norm_threshold', 'momentum'}:
                    raise ValueError(f'guidance_apg[{i}] = {apg!r}: a dict with the keys eta, norm_threshold, momentum (each optional)')
                thr = finite(apg.get('norm_threshold'), f'guidance_apg[{i}][norm_threshold]', none_ok=True)
                out.append(('apg', finite(apg.get('eta', 0.), f'guidance_apg[{i}][eta]'), max(thr, 0.), finite(apg.get('momentum', 0.), f'guidance_apg[{i}][momentum]')))
            else:
                out.append(None)
        self._cannot_guide('guidance_rescale' if guidance_rescale is not None else 'guidance_apg', 'cannot do classifier free guidance', 'guide')
        return tuple(out)

    def _resolve_guidance(self, c: _Call, given) -> tuple:
        """What `_guidance_of` returned for one call whose solver and per-unet cond_scale are resolved -> per unet None, or the fp32 [steps]
        guidance scales of a stage whose scale varies (schedules.guidance_scales on the grid of the stage's sampler).  A stage whose resolved
        scales are all the same is an ordinary stage at that scale: it is written to c.cond_scale[idx] (left as given where it already is
        that value) and the entry stays None, so a constant schedule meets the stage — and the cache key — of the scalar call.  Only the
        stages the call runs are resolved; nothing is launched."""
        from .schedules import guidance_scales

        n = len(self.unets)
        if given is None:
            return (None,) * n
        self._refuse_inpainting(c, 'guidance_schedule / guidance_interval', 'runs every table row several times on one captured plan; '
                                'sample with a fixed cond_scale when inpainting')
        out, scales = [None] * n, list(c.cond_scale)
        for idx in range(*stage_range(c, n)):
            sched, interval = given[0][idx], given[1][idx]
            if sched is None and interval is None:
                continue
            self._needs_text_branch(idx, 'guidance_schedule / guidance_interval', 'guide')
            steps = self.noise_schedulers[idx].num_timesteps if c.solver is None else c.solver[idx][1]
            vec = guidance_scales(steps, scales[idx], sched, interval, what=f'unet {idx + 1}')
            if bool((vec == vec[0]).all()):
                if float(torch.tensor(float(scales[idx]), dtype=torch.float32)) != float(vec[0]):
                    scales[idx] = float(vec[0])
            else:
                out[idx] = vec
        c.cond_scale = tuple(scales)
        return tuple(out)

    def _check_guide(self, c: _Call, given):
        """What `_guide_of` returned against the stages of one call — their resolved cond_scale and guidance vectors.  Refused: inpainting, a
        stage whose unet has no text branch, and (not for one stage of a cascade sample_pipelined has checked as a whole) a call none of
        whose stages with a setting is guided, which would silently ignore the keyword."""
        if given is None:
            return None
        self._refuse_inpainting(c, 'guidance_rescale / guidance_apg', 'runs every table row several times on one captured plan; '
                                'sample with the plain guidance when inpainting')
        stages = [idx for idx in range(*stage_range(c, len(self.unets))) if given[idx] is not None]
        for idx in stages:
            self._needs_text_branch(idx, 'guidance_rescale / guidance_apg', 'guide')
        if not c.pipelined_stage and all(c.cond_scale[idx] == 1. and c.guidance[idx] is None for idx in stages):
            raise ValueError('guidance_rescale / guidance_apg: no stage of this call that has a setting is guided (cond_scale is 1 and there is '
                             'no schedule), so the keyword would be silently ignored')
        return given

    def _compose_of(self, c: _Call):
        """`compose=` / `compose_mask=` of one call whose text, batch, sizes, cond_scale and guidance are resolved: None without the keyword,
        else dict(K, prompts, weights, masks) — prompts: the (embeds, masks) of the prompts 1 .. K - 1 on the device, batch 1 or B; weights:
        per unet an fp32 [K, B] tensor (row 0 the main prompt's cond_scale); masks: None when no prompt has one, else K entries None | fp32
        [B | 1, H, W].  Every refusal is a ValueError; nothing is built or launched."""
        if c.compose is None and c.compose_mask is None:
            return None
        n, B, kmax = len(self.unets), c.batch_size, ops.ENUMS["IMAGEN_COMPOSE_MAX"]
        if not isinstance(c.compose, (list, tuple)) or not c.compose or not all(isinstance(e, dict) for e in c.compose):
            raise ValueError('compose: a non-empty list of dicts(text_embeds= | texts=, text_masks=, weight=, mask=), one per further prompt '
                             '(compose_mask alone composes nothing)')
        if len(c.compose) + 1 > kmax:
            raise ValueError(f'compose: {len(c.compose)} entries + the call\'s own prompt are {len(c.compose) + 1} prompts, at most {kmax} are composed')
        given = [k for k in GUIDANCE_KEYWORDS if getattr(c, k) is not None]
        if given:
            raise ValueError(f"compose with {', '.join(given)}: those act on the one scale of plain guidance (CFG_X0 / GUIDE_X0); composed prompts "
                             f"carry a weight per prompt at a fixed value")
        self._refuse_inpainting(c, 'compose', 'is planned on the two-branch step; inpaint with one prompt')
        if c.conditioning is not None:
            raise ValueError('compose with a `conditioning` handle: a handle stages one prompt per sample; pass text_embeds / texts with compose')
        if isinstance(c.seed, (list, tuple)) or c.negative_rows is not None:
            raise ValueError('compose inside merged requests (sample_requests): not covered')
        if any(isinstance(u, Unet3D) for u in self.unets):
            raise ValueError('compose: this cascade has a Unet3D stage; composed prompts run on the image engine (UnetEngine) only')
        self._cannot_guide('compose', 'has no null branch to compose against', 'compose prompts on', no_text=c.text_embeds is None)
        first, last = stage_range(c, n)
        for idx in range(first, last):
            self._needs_text_branch(idx, 'compose', 'compose')

        def weight_of(v, what):
            """-> per unet an fp32 [B] tensor"""
            if isinstance(v, torch.Tensor) and v.ndim == 1:
                if v.shape[0] != B:
                    raise ValueError(f'{what}: a [B] tensor of {v.shape[0]} weights, the batch is {B}')
                per = (v.detach().float().cpu(),) * n
            else:
                if not (is_number(v) or (isinstance(v, (list, tuple)) and len(v) == n and all(is_number(x) for x in v))):
                    raise ValueError(f'{what} = {v!r}: a float, a tuple of one float per unet ({n}), or a [B] tensor')
                per = tuple(torch.full((B,), float(x), dtype=torch.float32) for x in _cast_tuple(v, n))
            if not all(bool(torch.isfinite(w).all()) for w in per):
                raise ValueError(f'{what}: weights must be finite')
            return per

        def mask_of(m, what):
            if m is None:
                return None
            if not isinstance(m, torch.Tensor) or m.ndim not in (2, 3) or (m.ndim == 3 and m.shape[0] not in (1, B)) or 0 in m.shape:
                raise ValueError(f'{what}: a [B | 1, H, W] or [H, W] tensor (B = {B})' + (f', got {tuple(m.shape)}' if isinstance(m, torch.Tensor) else ''))
            m = m.detach().float().cpu()
            if not bool(((m >= 0.) & (m <= 1.)).all()):          # (also refuses nan)
                raise ValueError(f'{what}: values outside [0, 1]')
            return m[None] if m.ndim == 2 else m

        prompts, weights, masks = [], [weight_of(tuple(c.cond_scale), 'cond_scale')], [mask_of(c.compose_mask, 'compose_mask')]
        for i, e in enumerate(c.compose):
            unknown = set(e) - {'text_embeds', 'texts', 'text_masks', 'weight', 'mask'}
            if unknown:
                raise ValueError(f'compose[{i}]: unknown keys {sorted(unknown)}; text_embeds | texts, text_masks, weight, mask')
            texts, emb, tm = e.get('texts'), e.get('text_embeds'), e.get('text_masks')
            if (texts is None) == (emb is None):
                raise ValueError(f'compose[{i}]: one of text_embeds and texts')
            if texts is not None:
                texts = [texts] if isinstance(texts, str) else list(texts)
                if not all(map(len, texts)):
                    raise ValueError(f'compose[{i}].texts: text cannot be empty')
                emb, tm = self.encode_text(texts, return_attn_mask=True)
            kw = f'compose[{i}].text_embeds' if texts is None else f'compose[{i}].texts'
            if not isinstance(emb, torch.Tensor) or emb.ndim != 3 or emb.shape[-1] != self.text_embed_dim:
                raise ValueError(f"{kw}: invalid text embedding shape {tuple(emb.shape) if isinstance(emb, torch.Tensor) else emb!r} "
                                 f"(should be (b, n, {self.text_embed_dim}))")
            if emb.shape[0] not in (1, B):
                raise ValueError(f"{kw}: batch {emb.shape[0]} is neither 1 nor the prompts' {B}")
            if tm is not None and tuple(tm.shape) != tuple(emb.shape[:2]):
                raise ValueError(f"compose[{i}].text_masks: shape {tuple(tm.shape)} does not match the prompt's {tuple(emb.shape[:2])}")
            emb = emb.to(c.device)
            prompts.append((emb, tm.to(c.device) if tm is not None else torch.any(emb != 0., dim=-1)))
            weights.append(weight_of(e.get('weight', 1.), f'compose[{i}].weight'))
            masks.append(mask_of(e.get('mask'), f'compose[{i}].mask'))
        by_unet = [torch.stack([w[idx] for w in weights]) for idx in range(n)]
        if not c.pipelined_stage and all(c.cond_scale[idx] == 1. and not bool(by_unet[idx][1:].any()) for idx in range(first, last)):
            raise ValueError('compose: cond_scale is 1 and every further weight is 0 on every stage of this call, so the keyword would be silently ignored')
        return dict(K=len(prompts) + 1, prompts=prompts, weights=by_unet, masks=masks if any(m is not None for m in masks) else None)

    def _tiles_of(self, c: _Call):
        """`tile_shapes=` / `tile_overlap=` / `tile_blend=` of one call whose sizes, batch, cond_scale and guidance are resolved: None without
        `tile_shapes` (or with None for every stage the call runs), else per unet None | tile_geometry(...) of that stage's canvas (c.sizes).  One
        (h, w) — a pair of ints is ONE tile shape, never two stages' square sides —, an int or None serves every unet; a tuple of pairs / ints /
        None holds one entry per unet; the overlap likewise.  Every refusal is a ValueError; nothing is built or launched."""
        if c.tile_shapes is None:
            if c.tile_overlap is not None or c.tile_blend not in (None, 'ramp'):
                raise ValueError('tile_overlap / tile_blend without tile_shapes: there is no tile to overlap or blend')
            return None
        n = len(self.unets)
        pair = lambda v: isinstance(v, (tuple, list, torch.Size)) and len(v) == 2 and all(isinstance(e, int) and not isinstance(e, bool) for e in v)
        one = lambda v: (isinstance(v, int) and not isinstance(v, bool)) or pair(v)
        shapes = per_unet(c.tile_shapes, 'tile_shapes', n, one, entry='one (h, w), int or None')
        overlaps = per_unet(c.tile_overlap, 'tile_overlap', n, one, entry='one int, (oy, ox) or None')
        blend = 'ramp' if c.tile_blend is None else c.tile_blend
        if blend not in TILE_BLENDS:
            raise ValueError(f"tile_blend = {blend!r}: {' | '.join(repr(b) for b in TILE_BLENDS)}")
        first, last = stage_range(c, n)
        if all(shapes[idx] is None for idx in range(first, last)):
            return None
        if any(isinstance(u, Unet3D) for u in self.unets):
            raise ValueError('tile_shapes: this cascade has a Unet3D stage; tiled sampling runs on the image engine (UnetEngine) only')
        self._refuse_inpainting(c, 'tile_shapes', 'pastes the known pixels on the whole image; inpaint untiled')
        if c.compose is not None or c.compose_mask is not None:
            raise ValueError('tile_shapes with compose / compose_mask: COMPOSE_X0 reads its masks per engine row, which would be per tile; not covered')
        if c.guidance_rescale is not None or c.guidance_apg is not None:
            raise ValueError('tile_shapes with guidance_rescale / guidance_apg: their per-sample sums (GUIDE_X0) would be per-tile sums')
        if c.guidance_interval is not None:
            raise ValueError('tile_shapes with guidance_interval: the unguided steps run a sibling plan on the stage\'s state, which a tiled stage does not build')
        if any(g is not None and bool((g == 1.).any()) for g in c.guidance):
            raise ValueError('tile_shapes with a guidance_schedule that has unguided steps (scale 1): those run a sibling plan, which a tiled stage does not build')
        if c.conditioning is not None:
            raise ValueError('tile_shapes with a `conditioning` handle: a handle stamps the engine of one prompt row per sample; pass text_embeds / texts')
        if isinstance(c.seed, (list, tuple)) or c.negative_rows is not None:
            raise ValueError('tile_shapes inside merged requests (sample_requests): not covered')
        if c.cond_images is not None:
            raise ValueError('tile_shapes with cond_images: the conditioning image is staged per engine row, which would be per tile; not covered')
        out, tmax = [None] * n, ops.ENUMS['IMAGEN_TILE_MAX']
        for idx in range(first, last):
            s, o, unet = shapes[idx], overlaps[idx], self.unets[idx]
            if s is None:
                continue
            what = f'tile_shapes[{idx}]'
            if not one(s):
                raise ValueError(f'{what} = {s!r}: an (h, w) pair of ints, an int or None')
            if o is not None and not one(o):
                raise ValueError(f'tile_overlap[{idx}] = {o!r}: an int, an (oy, ox) pair of ints or None')
            if getattr(unet, 'self_cond', False):
                raise ValueError(f'{what}: unet {idx + 1} self-conditions on the previous x0 per engine row, which would be the unblended tile; not covered')
            if getattr(unet, 'has_cond_image', False):
                raise ValueError(f'{what}: unet {idx + 1} takes cond_images (cond_images_channels), staged per engine row; not covered')
            h, w = (int(s), int(s)) if isinstance(s, int) else (int(s[0]), int(s[1]))
            oy, ox = (h // 4, w // 4) if o is None else (int(o), int(o)) if isinstance(o, int) else (int(o[0]), int(o[1]))
            if min(h, w) <= 0:
                raise ValueError(f'{what} = {s!r}: positive sides')
            unet.check_image_size(h, w, what=what)
            H, W = (c.sizes[idx],) * 2 if isinstance(c.sizes[idx], int) else c.sizes[idx]
            if h > H or w > W:
                raise ValueError(f'{what} = {h} x {w} is larger than the canvas of unet {idx + 1}, {H} x {W}')
            for L, ov, ax in ((h, oy, 'y'), (w, ox, 'x')):
                if not 0 <= ov < L:
                    raise ValueError(f'tile_overlap[{idx}]: {ov} along {ax} is outside [0, {L}) (the tile side)')
            ty, tx = len(tile_origins(H, h, oy)), len(tile_origins(W, w, ox))
            if ty * tx > tmax:
                raise ValueError(f'{what}: {ty} x {tx} = {ty * tx} tiles on a canvas of {H} x {W}, at most {tmax} are blended (IMAGEN_TILE_MAX)')
            rows = ty * tx * c.batch_size * (1 if c.cond_scale[idx] == 1. and c.guidance[idx] is None else 2)
            heads = unet._attn_kwargs['heads']
            if rows * heads > 65535:
                raise ValueError(f'{what}: {ty * tx} tiles of a batch of {c.batch_size} are {rows} engine rows; rows x {heads} attention heads exceed '
                                 f'the 65535 workgroups of a launch axis, which the engine refuses')
            out[idx] = tile_geometry(H, W, h, w, oy, ox, blend)
        return tuple(out)

    # ---- the negative prompt: as given, encoded, checked
    def _negative_of_call(self, conditioning, negative_texts, negative_text_embeds, negative_text_masks, negative_rows=None):
        """The negative prompt of one sample() call as given — by keyword, or on the conditioning handle — for _resolve, which resolves and
        checks it once the batch and the guidance scales are known.  (The fourth entry, the samples it applies to, is sample_requests'.)"""
        given = negative_texts is not None or negative_text_embeds is not None or negative_text_masks is not None
        if conditioning is not None:
            if given:
                raise ValueError('negative_texts / negative_text_embeds: a `conditioning` handle carries its own negative prompt '
                                 '(prepare_conditioning(negative_text_embeds=...)); pass one or the other')
            negative_text_embeds, negative_text_masks = conditioning.negative_text_embeds, conditioning.negative_text_masks
            given = negative_text_embeds is not None
        return (negative_texts, negative_text_embeds, negative_text_masks, negative_rows) if given else None

    def _resolve_negative(self, texts, text_embeds, text_masks, device, batch=None, whose="the prompts'"):
        """negative_texts -> the `encode_text` hook; default mask = any non-zero feature (as _resolve_text does for the prompt).  Returns
        (embeds [b, n, text_embed_dim], mask [b, n]) with b = 1 or `batch`, or (None, None) when no negative prompt was given."""
        if texts is None and text_embeds is None:
            check_negative_prompt(None, text_masks, None, None)
            return None, None
        if texts is not None and text_embeds is not None:
            raise ValueError('negative_texts and negative_text_embeds are both given: pass one of them')
        kw = 'negative_texts' if texts is not None else 'negative_text_embeds'
        self._cannot_guide(kw, text='put a negative prompt on')
        if texts is not None:
            assert all([*map(len, texts)]), 'negative_texts: text cannot be empty'
            text_embeds, text_masks = self.encode_text(texts, return_attn_mask=True)
        check_negative_prompt(text_embeds, text_masks, batch, self.text_embed_dim, kw=kw, whose=whose)
        text_embeds = text_embeds.to(device)
        text_masks = text_masks.to(device) if text_masks is not None else torch.any(text_embeds != 0., dim=-1)
        return text_embeds, text_masks

    def _check_negative(self, negative, batch_size, cond_scales, device):
        """Resolve and check the negative prompt of one call (`negative`: what _negative_of_call returned) for `batch_size` samples.
        `cond_scales`: the guidance scales of the stages the call runs — all 1 would silently ignore the prompt, which is refused; None
        where no stage can be told unguided from its scale: one stage of a cascade sample_pipelined has checked as a whole, composed
        prompts.  Returns (embeds, masks, rows)."""
        kw = 'negative_texts' if negative[0] is not None else 'negative_text_embeds'
        neg_embeds, neg_masks = self._resolve_negative(*negative[:3], device, batch=batch_size)
        neg_rows = negative[3]
        if neg_rows is not None and tuple(neg_rows.shape) != (batch_size,):
            raise ValueError(f'{kw}: the merged requests mark {tuple(neg_rows.shape)} samples, the batch has {batch_size}')
        self._cannot_guide(kw, 'cannot do classifier free guidance, which is where a negative prompt acts')
        if cond_scales is not None and all(cs == 1. for cs in cond_scales):
            raise ValueError(f'{kw}: cond_scale is 1 on every stage of this call, so the negative prompt would be silently ignored')
        return neg_embeds, neg_masks, neg_rows

    def _resolve_text(self, texts, text_embeds, text_masks, device):
        """ip.py:2326-2337: texts -> encoder hook; default mask = any non-zero feature."""
        if texts is not None and text_embeds is None and not self.unconditional:
            assert all([*map(len, texts)]), 'text cannot be empty'
            text_embeds, text_masks = self.encode_text(texts, return_attn_mask=True)
        if not self.unconditional:
            assert text_embeds is not None, 'text must be passed in if the network was not trained without text `condition_on_text` must be set to `False` when training'
            text_embeds = text_embeds.to(device)
            text_masks = text_masks.to(device) if text_masks is not None else torch.any(text_embeds != 0., dim=-1)
        return text_embeds, text_masks

    def _check_text(self, text_embeds):
        """ip.py:2353-2357, on the resolved text."""
        assert not (self.condition_on_text and text_embeds is None), 'text or text encodings must be passed into imagen if specified'
        assert not (not self.condition_on_text and text_embeds is not None), 'imagen specified not to be conditioned on text, yet it is presented'
        assert not (text_embeds is not None and text_embeds.shape[-1] != self.text_embed_dim), \
            f'invalid text embedding dimension being passed in (should be {self.text_embed_dim})'

    @torch.no_grad()
    def prepare_conditioning(self, texts: Optional[List[str]] = None, *, text_embeds=None, text_masks=None, batch_size: int = 1,
                             device=None, negative_texts: Optional[List[str]] = None, negative_text_embeds=None,
                             negative_text_masks=None) -> Conditioning:
        """Encode / stage the prompts (and the negative prompt, if any) once; reuse the returned handle with
        `sample(conditioning=handle, ...)`."""
        device = torch.device(device) if device is not None else self.device
        text_embeds, text_masks = self._resolve_text(texts, text_embeds, text_masks, device)
        self._check_text(text_embeds)
        neg, neg_masks = self._resolve_negative(negative_texts, negative_text_embeds, negative_text_masks, device,
                                                batch=None if text_embeds is None else text_embeds.shape[0])
        return Conditioning(text_embeds, text_masks, text_embeds.shape[0] if text_embeds is not None else batch_size, neg, neg_masks)

    def _resolve_sizes(self, image_shapes) -> tuple:
        """The size of every stage of one call: image_sizes, or the call's `image_shapes` — one (H, W) per unet, each divisible by its
        unet's downsamples, no stage smaller than the one before it on either axis; an image cascade only.  A square entry is the int
        of that side, so that it meets the stage (and the engine) a square call builds."""
        if image_shapes is None:
            return tuple(self.image_sizes)
        if self.is_video:
            raise ValueError('image_shapes: rectangular sampling covers image cascades; a video cascade samples square frames')
        shapes = [tuple(int(v) for v in s) if isinstance(s, (tuple, list, torch.Size)) else s for s in image_shapes]
        if len(shapes) != len(self.unets):
            raise ValueError(f'image_shapes: {len(shapes)} entries for {len(self.unets)} unets (one (H, W) per unet)')
        for i, (s, unet) in enumerate(zip(shapes, self.unets)):
            if not (isinstance(s, tuple) and len(s) == 2):
                raise ValueError(f'image_shapes[{i}] = {s!r}: an (H, W) pair per unet')
            if isinstance(unet, Unet):
                unet.check_image_size(*s, what=f'image_shapes[{i}]')
            if i and (s[0] < shapes[i - 1][0] or s[1] < shapes[i - 1][1]):
                raise ValueError(f'image_shapes[{i}] = {s} is smaller than image_shapes[{i - 1}] = {shapes[i - 1]}: the stages of a cascade only upsample')
        return tuple(s[0] if s[0] == s[1] else s for s in shapes)

    def _resolve(self, c: _Call) -> _Call:
        """Everything of sample() (ip.py:2291-2404) up to the stage loop, written back into the record: the pre-flight, then device, text, batch
        size, inpainting inputs, the per-unet tuples, guidance, composed prompts, the seed, the negative prompt with its refusals, the start
        image.  Builds no stage and launches nothing."""
        c.negative = self._negative_of_call(c.conditioning, c.negative_texts, c.negative_text_embeds, c.negative_text_masks, c.negative_rows)
        c.solver, guidance, guide = self._preflight(**vars(c))
        if c.solver is not None:
            self._refuse_inpainting(c, f"sampler='{c.solver[0][0]}'", "is defined on the ancestral step; inpaint with sampler='ddpm'")
            if c.solver[0][2] > 0. and isinstance(c.seed, (list, tuple)):
                raise ValueError('merged requests take the deterministic solvers (eta = 0)')
        c.sizes = self._resolve_sizes(c.image_shapes)
        if c.conditioning is not None:
            assert c.texts is None and c.text_embeds is None and c.text_masks is None, 'pass either `conditioning` or texts / text_embeds'
            c.text_embeds, c.text_masks = c.conditioning.text_embeds, c.conditioning.text_masks
            if c.text_embeds is None:
                c.batch_size = c.conditioning.batch_size
        device = c.device = self._sampling_device(c.device)
        self.reset_unets_all_one_device(device)
        if c.inpaint_videos is not None:                 # ip.py:2342: the video argument wins
            c.inpaint_images = c.inpaint_videos
        if not self.is_video:                            # ip.py:2417-2427: only video cascades hand the prompt frames to their unets
            c.cond_video_frames = c.post_cond_video_frames = None
        if c.cond_images is not None:
            c.cond_images = c.cond_images.to(device)
            if c.cond_images.dtype == torch.uint8:       # cast_uint8_images_to_float, ip.py:2324
                c.cond_images = c.cond_images.float() / 255
        assert not (self.is_video and c.video_frames is None), 'video_frames must be passed in on sample time if training on video'   # ip.py:2381
        if self.is_video:
            for f in self.temporal_downsample_factor:                       # calc_all_frame_dims, ip.py:170-183
                assert int(c.video_frames) % f == 0, f'video_frames {c.video_frames} must be divisible by the temporal downsample factor {f}'
        c.frames = int(c.video_frames) if self.is_video else 0
        assert not (c.return_pil_images and self.is_video), 'converting sampled video tensor to video file is not supported yet'   # ip.py:2494

        c.text_embeds, c.text_masks = self._resolve_text(c.texts, c.text_embeds, c.text_masks, device)
        text_embeds, inpaint_images = c.text_embeds, c.inpaint_images
        if not self.unconditional:
            c.batch_size = text_embeds.shape[0]
        if inpaint_images is not None:                   # ip.py:2344-2351
            if self.unconditional and c.batch_size == 1:
                c.batch_size = inpaint_images.shape[0]
            assert inpaint_images.shape[0] == c.batch_size, \
                'number of inpainting images must be equal to the specified batch size on sample `sample(batch_size=<int>)``'
            assert not (self.condition_on_text and inpaint_images.shape[0] != text_embeds.shape[0]), \
                'number of inpainting images must be equal to the number of text to be conditioned on'
        self._check_text(text_embeds)
        assert not ((inpaint_images is not None) ^ (c.inpaint_masks is not None)), \
            'inpaint images and masks must be both passed in to do inpainting'
        num_unets = len(self.unets)
        assert not (self.is_video and self.resize_mode != 'nearest'), 'video cascades resize with nearest only in this build'
        if inpaint_images is not None:                   # ip.py:2217-2220
            c.known = self.normalize_img(inpaint_images.to(device).float())
            known_mask = c.inpaint_masks.to(device)
            if self.is_video:                            # ip.py:2373-2379
                assert c.known.ndim == 5, 'inpaint_videos must be (b, c, f, h, w)'
                if known_mask.ndim == 3:
                    known_mask = known_mask[:, None].expand(-1, c.frames, -1, -1)
                assert known_mask.shape[1] == c.frames
            c.known_mask = known_mask[:, None].float()
        c.init_images = [None if im is None else self.normalize_img(im.to(device).float()) for im in _cast_tuple(c.init_images, num_unets)]  # ip.py:2390-2391
        c.skip_steps = _cast_tuple(c.skip_steps, num_unets)
        c.level = c.lowres_sample_noise_level if c.lowres_sample_noise_level is not None else self.lowres_sample_noise_level
        c.cond_scale = _cast_tuple(c.cond_scale, num_unets)
        c.guidance = self._resolve_guidance(c, guidance)
        c.guide = self._check_guide(c, guide)
        c.composed = self._compose_of(c)
        c.tiles = self._tiles_of(c)
        if c.seed is None:
            c.seed = self._next_seed()
        # the negative prompt of this call: resolved and checked here, before any stage is built or anything is launched
        if c.negative is not None:
            scales = [cs if g is None else None for cs, g in zip(c.cond_scale, c.guidance)]      # (None: a schedule that varies, so not 1)
            scales = None if c.pipelined_stage or c.composed is not None else scales[slice(*stage_range(c, num_unets))]   # (a composed stage has null rows at any cond_scale)
            c.neg_embeds, c.neg_masks, c.neg_rows = self._check_negative(c.negative, c.batch_size, scales, device)
        if c.start_at_unet_number > 1:
            assert c.start_at_unet_number <= num_unets, 'must start a unet that is less than the total number of unets'
            assert c.stop_at_unet_number is None or c.start_at_unet_number <= c.stop_at_unet_number
            assert c.start_image_or_video is not None, 'starting image or video must be supplied if only doing upscaling'
            img = self._to_internal(c.start_image_or_video.to(device).float()).contiguous()
            prev_size = c.sizes[c.start_at_unet_number - 2]
            prev_hw = (prev_size, prev_size) if isinstance(prev_size, int) else prev_size
            assert img.shape[-3] == self.channels, f'start image must have {self.channels} channels'
            if tuple(img.shape[-2:]) != prev_hw:         # ip.py:2400-2404: first to the PREVIOUS stage's size (lowres_prep then resizes to this one's)
                lead = img.shape[:-3]
                img = self._resize(img.reshape(-1, *img.shape[-3:]), prev_size).reshape(*lead, self.channels, *prev_hw).contiguous()
            c.img = img
        return c
