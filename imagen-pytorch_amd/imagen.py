"""Drop-in `Imagen` (cascaded DDPM): constructor and `.sample()` signature of the reference
(imagen_pytorch/imagen_pytorch.py:1787-2498 = "ip.py"), sampling half only.

Each cascade stage runs T timesteps; one timestep = [denoiser plan of the stage's UnetEngine (both CFG branches
as one 2B-row batch)] + [CFG combine / x0 / exact 0.95-quantile / dynamic threshold / posterior / noise kernels],
captured ONCE into a hipGraph and replayed T times — the step index lives in a device counter that every
sampler kernel (and the time embedding) reads, so replay needs no host-side parameter patching.

Implemented options: text embeddings or the T5 hook (`texts=`), classifier-free guidance, dynamic thresholding, init_images /
skip_steps, inpainting (images and videos), cond_images, self-conditioning unets, start/stop_at_unet_number, video cascades (Unet3D
stages) with cond_video_frames / post_cond_video_frames.  Training (`forward`, p_losses) raises.  Extensions beyond
the reference signature: `noise_fn`,
`seed`, `sample_offset` (batch sharding), `conditioning` handles, lanes (`with imagen.lane(i)`), `sample_pipelined`, negative prompts
(`negative_texts` / `negative_text_embeds` / `negative_text_masks`: a second prompt on the null rows of guidance) and few-step solvers
(`sampler='dpmpp_2m' | 'ddim'`, `sample_steps`, `eta`: the same checkpoint in tens of steps — the ancestral update replaced by one or two
LINCOMB launches on the tables of `schedules.solver_coefficients`).
"""
from __future__ import annotations

import contextlib
import functools
import os
import queue
import threading
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .ops import Plan
from .sample_call import GUIDANCE_KEYWORDS, Conditioning, SampleCall, _Call, _cast_tuple, _seed_spans  # noqa: F401  (re-exported: the names this module always had)
from .schedules import GaussianDiffusionContinuousTimes
from .t5 import t5_encode_text
from .unet import NullUnet, Unet
from .unet3d import Unet3D

T5_DIMS = {  # d_model of the encoders the reference accepts by name (t5.py:47-58 reads it from the HF config)
    't5-small': 512, 't5-base': 768, 't5-large': 1024, 't5-3b': 1024, 't5-11b': 1024,
    'google/t5-v1_1-small': 512, 'google/t5-v1_1-base': 768, 'google/t5-v1_1-large': 1024,
    'google/t5-v1_1-xl': 2048, 'google/t5-v1_1-xxl': 4096,
}
DEFAULT_T5_NAME = 'google/t5-v1_1-base'

TIME_TABLE = int(os.environ.get("IMAGEN_TIME_TABLE", "1"))   # A/B switch: the timestep-only conditioning of the image stages from a per-request table (engine.enable_time_table)
_SAMPLING_DEVICE_TYPES = ('cuda',)   # where plans can be launched; tests/test_sample_cpu_replay.py widens it after replacing the launcher
TAG_INIT, TAG_LOWRES = 0x7FFF0001, 0x7FFF0002  # RANDN counter tags (step noise uses the step index)


def nearest_indices(n_in: int, n_out: int) -> torch.Tensor:
    """Source indices of F.interpolate(mode='nearest') along one axis: floor(dst * fp32(n_in / n_out)), capped at n_in - 1.  Torch
    rounds the scale to fp32, so for some ratios (2 -> 82, 14 -> 46) this is not the integer dst * n_in // n_out; taken from torch itself."""
    return F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in), n_out, mode='nearest').view(n_out).long()


def _pad_tuple(t, length, fill):
    return t if len(t) >= length else (*t, *((fill,) * (length - len(t))))


def _to_pil_images(batch: torch.Tensor) -> list:
    """torchvision's ToPILImage for float (c, h, w) tensors in [0, 1] (`pic.mul(255).byte()`, HWC; ip.py:2496), without torchvision."""
    from PIL import Image

    modes = {1: 'L', 3: 'RGB', 4: 'RGBA'}
    assert batch.ndim == 4 and batch.shape[1] in modes, 'PIL conversion needs (b, 1 | 3 | 4, h, w) images'
    arr = batch.detach().mul(255).byte().permute(0, 2, 3, 1).cpu().numpy()
    return [Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a, mode=modes[a.shape[-1]]) for a in arr]


def _out_of_scope(what):
    raise NotImplementedError(f"{what} is outside the MI355X sampling hot path of this build (SURVEY.md §2 / §8)")


class Imagen(SampleCall, nn.Module):
    """The model, its stages and their run loop; the mixin, sample_call.SampleCall, turns a call's keywords into the record the stages read."""
    _lowres_time_raw = False   # the low-res stages are conditioned on the log-SNR of the augmentation level (ip.py:2081), not the level itself

    def __init__(
        self,
        unets,
        *,
        image_sizes,
        text_encoder_name=DEFAULT_T5_NAME,
        text_embed_dim=None,
        channels=3,
        timesteps=1000,
        cond_drop_prob=0.1,
        loss_type='l2',
        noise_schedules='cosine',
        pred_objectives='noise',
        random_crop_sizes=None,
        lowres_noise_schedule='linear',
        lowres_sample_noise_level=0.2,
        per_sample_random_aug_noise_level=False,
        condition_on_text=True,
        auto_normalize_img=True,
        dynamic_thresholding=True,
        dynamic_thresholding_percentile=0.95,
        only_train_unet_number=None,
        temporal_downsample_factor=1,
        resize_cond_video_frames=True,
        resize_mode='nearest',
        min_snr_loss_weight=True,
        min_snr_gamma=5,
    ):
        super().__init__()
        if loss_type not in ('l1', 'l2', 'huber'):
            raise NotImplementedError()
        self.loss_type = loss_type
        self.condition_on_text = condition_on_text
        self.unconditional = not condition_on_text
        self.channels = channels

        unets = _cast_tuple(unets)
        num_unets = len(unets)
        timesteps = _cast_tuple(timesteps, num_unets)

        # 'cosine', 'cosine', then 'linear' for further super-resolution stages (ip.py:1853-1855)
        noise_schedules = _pad_tuple(_pad_tuple(_cast_tuple(noise_schedules), 2, 'cosine'), num_unets, 'linear')
        self.noise_schedulers = nn.ModuleList([GaussianDiffusionContinuousTimes(noise_schedule=s, timesteps=t)
                                               for t, s in zip(timesteps, noise_schedules)])
        self.random_crop_sizes = _cast_tuple(random_crop_sizes, num_unets)
        self.lowres_noise_schedule = GaussianDiffusionContinuousTimes(noise_schedule=lowres_noise_schedule)
        self.pred_objectives = _cast_tuple(pred_objectives, num_unets)

        self.text_encoder_name = text_encoder_name
        # hook of sample(texts=...), ip.py:1832 / 2326-2332; replace it to plug in another encoder
        self.encode_text = functools.partial(t5_encode_text, name=text_encoder_name)
        if text_embed_dim is None:
            if text_encoder_name not in T5_DIMS:
                raise ValueError(f"unknown text encoder '{text_encoder_name}': pass text_embed_dim explicitly")
            text_embed_dim = T5_DIMS[text_encoder_name]
        self.text_embed_dim = text_embed_dim

        self.unets = nn.ModuleList([])
        self.unet_being_trained_index = -1
        self.only_train_unet_number = only_train_unet_number
        for ind, one_unet in enumerate(unets):
            assert isinstance(one_unet, (Unet, Unet3D, NullUnet))
            one_unet = one_unet.cast_model_parameters(
                lowres_cond=ind > 0, cond_on_text=self.condition_on_text,
                text_embed_dim=self.text_embed_dim if self.condition_on_text else None,
                channels=self.channels, channels_out=self.channels)   # ip.py:1897-1903 (may re-instantiate with fresh weights)
            self.unets.append(one_unet)

        image_sizes = _cast_tuple(image_sizes)
        self.image_sizes = image_sizes
        assert num_unets == len(image_sizes), f'you did not supply the correct number of u-nets ({len(unets)}) for resolutions {image_sizes}'
        self.sample_channels = _cast_tuple(self.channels, num_unets)
        self.is_video = any(isinstance(u, Unet3D) for u in self.unets)     # ip.py:1918-1919
        self.resize_mode = resize_mode                    # ip.py:1924: every image resize of the cascade goes through this mode
        self.temporal_downsample_factor = _cast_tuple(temporal_downsample_factor, num_unets)
        self.resize_cond_video_frames = resize_cond_video_frames                                                           # ip.py:1931
        assert self.temporal_downsample_factor[-1] == 1, 'downsample factor of last stage must be 1'                       # ip.py:1934
        assert tuple(sorted(self.temporal_downsample_factor, reverse=True)) == self.temporal_downsample_factor, \
            'temporal downsample factor must be in order of descending'                                                   # ip.py:1935

        lowres_conditions = tuple(u.lowres_cond for u in self.unets)
        assert lowres_conditions == (False, *((True,) * (num_unets - 1))), \
            'the first unet must be unconditioned (by low resolution image), and the rest of the unets must have `lowres_cond` set to True'

        self.lowres_sample_noise_level = lowres_sample_noise_level
        self.per_sample_random_aug_noise_level = per_sample_random_aug_noise_level
        self.cond_drop_prob = cond_drop_prob
        self.can_classifier_guidance = cond_drop_prob > 0.
        self.auto_normalize_img = auto_normalize_img
        self.input_image_range = (0. if auto_normalize_img else -1., 1.)
        self.normalize_img = (lambda img: img * 2 - 1) if auto_normalize_img else (lambda img: img)          # ip.py:1885-1888
        self.unnormalize_img = (lambda img: (img + 1) * 0.5) if auto_normalize_img else (lambda img: img)
        self.dynamic_thresholding = _cast_tuple(dynamic_thresholding, num_unets)
        self.dynamic_thresholding_percentile = dynamic_thresholding_percentile
        min_snr_loss_weight = _cast_tuple(min_snr_loss_weight, num_unets)
        min_snr_gamma = _cast_tuple(min_snr_gamma, num_unets)
        self.min_snr_gamma = tuple((g if use else None) for use, g in zip(min_snr_loss_weight, min_snr_gamma))

        self.register_buffer('_temp', torch.tensor([0.]), persistent=False)
        self.to(next(self.unets.parameters()).device)
        self._stages = {}
        self._streams: Dict[tuple, torch.cuda.Stream] = {}   # (lane, device) -> private stream
        self._tls = threading.local()                        # per-thread: the lane index, nothing else (a call's state is its _Call record)
        self._mode_lock = threading.Lock()
        self._build_lock = threading.RLock()                 # stage construction (engine plans + shared weight packing) is serialised
        self._mode_depth = 0
        self._call_counter = 0

    def _next_seed(self) -> int:
        """Derived Philox key of a call without `seed=`: distinct per call, also when lanes call concurrently (the counter is locked)."""
        with self._mode_lock:
            self._call_counter += 1
            c = self._call_counter
        return (int(torch.initial_seed()) * 1000003 + c) & ((1 << 62) - 1)

    # ---- device bookkeeping (API parity; weights stay resident as packed copies, nothing is shuffled over PCIe) ----
    @property
    def device(self):
        return self._temp.device

    def force_unconditional_(self):
        self.condition_on_text = False
        self.unconditional = True
        for unet in self.unets:
            unet.cond_on_text = False

    def get_unet(self, unet_number):
        assert 0 < unet_number <= len(self.unets)
        return self.unets[unet_number - 1]

    def reset_unets_all_one_device(self, device=None):
        device = device if device is not None else self.device
        self.unets.to(device)
        self.unet_being_trained_index = -1

    def state_dict(self, *args, **kwargs):
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        return super().load_state_dict(*args, **kwargs)

    def forward(self, *args, **kwargs):
        _out_of_scope("Imagen.forward (training loss, ip.py:2500-2734)")

    # ---- lanes: independent sampling contexts (own stream, own stage buffers + graphs, shared packed weights) ------------------
    @property
    def _lane(self) -> int:
        return getattr(self._tls, 'lane', 0)

    @contextlib.contextmanager
    def lane(self, index: int):
        """Extension: `with imagen.lane(i): imagen.sample(...)` runs the call on lane i — its own HIP stream and its own
        per-stage buffers / captured graphs; the packed weights are shared.  Calls on different lanes may be issued from
        different threads and overlap on the GPU (results are those of the same calls made one after the other)."""
        prev = self._lane
        self._tls.lane = int(index)
        try:
            yield self
        finally:
            self._tls.lane = prev

    @contextlib.contextmanager
    def _eval_mode(self):
        """eval() for the duration of a sample() call, restored when the LAST concurrent call ends."""
        with self._mode_lock:
            if self._mode_depth == 0:
                self._was_training = self.training
                self.eval()
            self._mode_depth += 1
        try:
            yield
        finally:
            with self._mode_lock:
                self._mode_depth -= 1
                if self._mode_depth == 0:
                    self.train(self._was_training)

    @torch.no_grad()
    def sample_requests(self, requests: List[dict], **common) -> List[torch.Tensor]:
        """Extension (serving): several independent `sample()` requests MERGED into one batch — one set of kernel launches per denoiser step for
        all of them (48 images as two merged batches of 24 sample 16 % faster on MI355X than as six concurrent requests of 8, profiles/r06_q_*).
        `requests` is a list of per-request keyword dicts (`text_embeds=` | `texts=`, `text_masks=`, `seed=`, `batch_size=` for unconditional
        cascades, `negative_texts=` | `negative_text_embeds=`, `negative_text_masks=`), `common` the keywords shared by all (`cond_scale=`,
        `max_steps=`, ...).  Requests with and without a negative prompt merge: the null rows of those without stay the learned ones.  Every row draws the noise of ITS OWN request — that
        request's Philox key and sample indices 0 .. b-1 (ABI 11: ImagenDdpmUpdateParams.row_keys) — so a request's images are the ones
        `sample(**common, **request)` produces up to the fp16 rounding of a different batch's tile configuration.  Returns one tensor per request.
        Not covered (raise): inpainting, init images, conditioning images / frames, `noise_fn`, `start_image_or_video`.  The solver keywords
        (`sampler=`, `sample_steps=`, `eta=`) are common ones; a stochastic solver (`eta > 0`) is refused: its update (LINCOMB) draws with one
        key per batch, and the deterministic ones draw nothing after the initial image, which carries every request's own key.  The guidance
        keywords (`guidance_schedule=`, `guidance_interval=`, `guidance_rescale=`, `guidance_apg=`) are common ones too, as `cond_scale=` is: inside
        a request they are refused.  (Rescale and projected guidance take their statistics per row, so a merged row is guided as in its own call.)"""
        solver, _, _ = self._preflight(**common)       # (raises before any text is encoded or any seed drawn)
        if common.get('compose') is not None or common.get('compose_mask') is not None or any('compose' in r or 'compose_mask' in r for r in requests):
            raise ValueError('sample_requests: compose / compose_mask inside or beside merged requests; the merged rows share one stage of 2 rows '
                             'per sample, composed prompts run K + 1: sample composed prompts with sample() or sample_pipelined()')
        tile_keys = ('tile_shapes', 'tile_overlap', 'tile_blend')
        if any(common.get(k) is not None for k in tile_keys) or any(k in r for r in requests for k in tile_keys):
            raise ValueError('sample_requests: tile_shapes / tile_overlap / tile_blend inside or beside merged requests; the merged rows share one stage of '
                             'one row per sample, a tiled stage runs T: sample tiled with sample() or sample_pipelined()')
        for k in GUIDANCE_KEYWORDS:
            if any(k in r for r in requests):
                raise ValueError(f'sample_requests: {k} inside a request; merged requests run one plan, so it is a common keyword, as cond_scale is')
        if solver is not None and solver[0][2] > 0.:
            raise ValueError(f"sample_requests(sampler='{solver[0][0]}', eta={solver[0][2]}): merged requests take the deterministic solvers "
                             f"(eta = 0); the stochastic update has no per-request noise keys")
        for k in ('inpaint_images', 'inpaint_videos', 'inpaint_masks', 'init_images', 'cond_images', 'cond_video_frames', 'post_cond_video_frames',
                  'noise_fn', 'start_image_or_video', 'conditioning', 'return_pil_images', 'return_all_unet_outputs', 'sample_offset'):
            if common.get(k) is not None or any(r.get(k) is not None for r in requests):
                _out_of_scope(f"sample_requests(..., {k}=...)")
        if not self._per_row_noise_keys:
            _out_of_scope(f"{type(self).__name__}.sample_requests (its sampler's noise launches take one key per batch)")
        if not requests:
            return []
        embeds, masks, seeds, sizes, negs, neg_rows = [], [], [], [], [], None
        neg_keys = ('negative_texts', 'negative_text_embeds', 'negative_text_masks')
        if any(common.get(k) is not None for k in neg_keys) and any(r.get(k) is not None for r in requests for k in neg_keys):
            raise ValueError('negative_texts / negative_text_embeds: pass the negative prompt per request or as a common keyword, not both')
        for r in requests:
            extra = set(r) - {'texts', 'text_embeds', 'text_masks', 'seed', 'batch_size', *neg_keys}
            assert not extra, f'per-request keywords {sorted(extra)} must be the same for all merged requests: pass them as common keywords'
            te, tm = self._resolve_text(r.get('texts'), r.get('text_embeds'), r.get('text_masks'), self.device)
            b = te.shape[0] if te is not None else int(r.get('batch_size', 1))
            ne, nm = self._resolve_negative(r.get('negative_texts'), r.get('negative_text_embeds'), r.get('negative_text_masks'), self.device,
                                            batch=b, whose="the request's")
            negs.append(None if ne is None else (ne.expand(b, -1, -1), nm.expand(b, -1)))
            embeds.append(te)
            masks.append(tm)
            sizes.append(b)
            seeds.append((self._next_seed() if r.get('seed') is None else int(r['seed']), b))
        kw = dict(common)
        kw.setdefault('use_tqdm', False)
        if embeds[0] is not None:
            width = max(e.shape[1] for e in embeds)       # (prompts of different lengths: zero-padded, masked)
            pad = lambda t, fill, w: torch.cat((t, t.new_full((t.shape[0], w - t.shape[1], *t.shape[2:]), fill)), 1) if t.shape[1] < w else t
            kw['text_embeds'] = torch.cat([pad(e, 0.0, width) for e in embeds])
            kw['text_masks'] = torch.cat([pad(m, False, width) for m in masks])
            if any(n is not None for n in negs):      # one row per sample; the requests without a negative prompt get zero rows that nothing reads
                nwidth = max(n[0].shape[1] for n in negs if n is not None)
                zero = lambda b: (torch.zeros(b, nwidth, self.text_embed_dim, device=self.device), torch.zeros(b, nwidth, dtype=torch.bool, device=self.device))
                pairs = [zero(b) if n is None else n for n, b in zip(negs, sizes)]
                kw['negative_text_embeds'] = torch.cat([pad(e, 0.0, nwidth) for e, _ in pairs])
                kw['negative_text_masks'] = torch.cat([pad(m, False, nwidth) for _, m in pairs])
                neg_rows = torch.cat([torch.full((b,), n is not None) for n, b in zip(negs, sizes)])
        else:
            kw['batch_size'] = sum(sizes)
        out = self._sample(self._call(seed=seeds, negative_rows=neg_rows, **kw))
        return list(torch.split(out, sizes))

    @torch.no_grad()
    def sample_pipelined(self, batches: List[dict], **common) -> List[torch.Tensor]:
        """Extension: sample successive batches with the cascade stages OVERLAPPED — stage s of batch k runs (own thread, own
        lane / stream / graph) while stage s+1 of batch k-1 does.  `batches` is a list of per-batch `sample()` keyword dicts
        (text_embeds=..., seed=..., ...), `common` the keywords shared by all.  Returns the final-stage images per batch, each
        bit-identical to `sample(**common, **batches[k])` (the stage hand-off is the same [0, 1] image the sequential cascade
        passes on, ip.py:2487-2490).  The base stage is latency-bound (few workgroups per launch at 64^2), the super-resolution
        stage throughput-bound: overlapped they fill the chip, so the sustained rate is set by the slower stage alone."""
        n_stages = len(self.unets)
        for k in ('start_at_unet_number', 'stop_at_unet_number', 'start_image_or_video', 'return_all_unet_outputs'):
            assert k not in common and all(k not in b for b in batches), f'sample_pipelined drives `{k}` itself'
        jobs = []
        for b in batches:
            kw = {**common, **b}
            if kw.get('seed') is None:                   # the seed must be the same for every stage of a batch (as in one sample() call)
                kw['seed'] = self._next_seed()
            kw.setdefault('use_tqdm', False)
            # every refusal of the whole cascade — what sample() with these keywords refuses — before a thread starts; nothing is launched.  (A
            # worker runs one stage per call, `pipelined_stage`: a stage at cond_scale 1 beside guided ones is no error there.)
            c = self._resolve(self._call(**kw))
            if c.neg_embeds is not None and c.conditioning is None:      # the negative prompt: encoded once for all stages of the batch
                kw.pop('negative_texts', None)
                kw['negative_text_embeds'], kw['negative_text_masks'] = c.neg_embeds, c.neg_masks
            jobs.append(kw)
        if n_stages == 1 or len(jobs) == 0:
            return [self.sample(**kw) for kw in jobs]
        caller = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(caller)
        qs = [queue.Queue() for _ in range(n_stages + 1)]
        errors: List[BaseException] = []

        def worker(s: int):
            try:
                with self.lane(0x100 + s), torch.cuda.device(self.device):
                    torch.cuda.current_stream().wait_event(ready)
                    while True:
                        item = qs[s].get()
                        if item is None or errors:
                            break
                        k, img = item
                        kw = dict(jobs[k])
                        if s > 0:
                            kw.update(start_at_unet_number=s + 1, start_image_or_video=img)
                        # (pipelined_stage: a single stage of a cascade checked above); returns after this lane's stream has drained
                        out = self._sample(self._call(**kw, stop_at_unet_number=s + 1, pipelined_stage=True))
                        qs[s + 1].put((k, out))
            except BaseException as e:   # noqa: BLE001 — re-raised in the caller
                errors.append(e)
            finally:
                qs[s + 1].put(None)

        threads = [threading.Thread(target=worker, args=(s,), daemon=True) for s in range(n_stages)]
        for t in threads:
            t.start()
        for k in range(len(jobs)):
            qs[0].put((k, None))
        qs[0].put(None)
        results: Dict[int, torch.Tensor] = {}
        while True:
            item = qs[n_stages].get()
            if item is None:
                break
            results[item[0]] = item[1]
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
        return [results[k] for k in range(len(jobs))]

    # ---- one cascade stage -------------------------------------------------------------------------------------
    def _stage(self, *args, **kwargs):
        """`_build_stage` under the construction lock; a NEW stage's packing kernels (weights shared with the other lanes) have
        completed before the stage becomes visible."""
        with self._build_lock:
            before = {k: id(v) for k, v in self._stages.items()}
            st = self._build_stage(*args, **kwargs)
            # a stage was constructed (new key, or a stale one rebuilt under its old key after a weight swap): its packing work runs on
            # THIS lane's stream and the packed weights are shared, so it must be complete before another lane can see the stage
            built = any(before.get(k) != id(v) for k, v in self._stages.items())
            if built and torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
            return st

    # The sampler state of a stage: what `_new_stage` allocates or, with share=, adopts (beside the engine's `x_in` / low-res image, adopted
    # through `eng.share_sampler_state`).  The one list of it: a buffer both plans of a guidance schedule must see is added here alone.
    SHARED_STATE = ('step_ptr', 'seed_dev', 'row_keys', 'noise', 'final', 'x0_thr', 'x0_prev', 'tables')
    _per_row_noise_keys = True      # this sampler's noise launches take per-row Philox keys (st['row_keys']): what sample_requests merges on
    _plan_prefix = ''               # of the names of the plans `_run_stage` builds
    _step_noun = 'timestep'
    _GRAPH_OF = {'plan': 'graph', 'last': 'graph_last'}     # the stage entry that holds a plan's captured graph

    def _new_stage(self, key: tuple, idx: int, B: int, device, *, cfg: bool, with_text: bool, inject_noise: bool, sample_offset: int,
                   resample_times: int, frames: int, prompt_frames: tuple, tables: Callable, size=None, buffers: tuple = (),
                   share: Optional[dict] = None, prompts: int = 1, tile: Optional[dict] = None):
        """What both samplers' `_build_stage` do first.  Returns (the cached stage of `key`, False) while its engine is not stale; else
        (a new stage dict, True): the engine (image or video), the sampler state (SHARED_STATE), the engine bound to the step counter and to
        `coef` = tables[0], the per-request time table where it applies, the buffers of inpainting.  EVERY key the run side reads is present
        (None where unused); the sampler adds its plan(s) and files the stage.  tables: () -> the sampler's device tables, [rows, 8] each,
        the per-evaluation one first; called only on a cache miss.  buffers: which of the optional [B, n] state buffers ('x0_thr',
        'x0_prev') the step needs.  prompts: K, the prompt sets of a guided stage — (K + 1) B denoiser rows, the null rows last; 1 is plain
        guidance's 2 B.  share: the stage whose sampler state this one runs on (the unguided sibling of a stage with a guidance
        schedule): the very objects of `share` are this stage's own, and its engine reads that stage's `x_in` / low-res image.  tile: the
        tile_geometry of a tiled stage (sample_call.tile_geometry) — the engine is built at the tile's size for T B samples (src_batch = T B,
        tile-major), the sampler state at the canvas's `size`: st['x'] is a canvas of its own that TILES gathers into the engine's `x_in`."""
        st = self._stages.get(key)
        if st is not None and not st['eng'].stale():
            return st, False
        unet, S, R = self.unets[idx], self.image_sizes[idx] if size is None else size, resample_times
        EB = B if tile is None else tile['T'] * B       # the engine's samples
        rows = (prompts + 1) * EB if cfg else EB
        video = isinstance(unet, Unet3D)
        assert prompts == 1 or (cfg and not video), 'composed prompts run on the guided image engine'
        assert tile is None or (prompts == 1 and not video and not R and share is None), 'a tiled stage is a plain image stage'
        if video:
            # Imagen-Video stage: the sampler state is the engine's frame-major clip (b, f, c, h, w); every sampler kernel is
            # elementwise per sample (the dynamic threshold is one quantile over the whole clip, ip.py:1921, 2097-2101), so only
            # the sample size changes.  sample() converts from / to the reference's (b, c, f, h, w) at the API boundary.
            assert frames > 0, 'video_frames must be passed in on sample time if training on video'
            from . import engine3d
            eng = engine3d.UnetEngine3D(unet, rows, B, frames, S, device, with_text=with_text, pre_frames=prompt_frames[0],
                                        post_frames=prompt_frames[1])
        else:
            from . import engine
            eng = engine.UnetEngine(unet, rows, EB, S if tile is None else (tile['h'], tile['w']), device, with_text=with_text)
        canvas = None
        if tile is not None:
            H, Wd = (S, S) if isinstance(S, int) else S
            canvas = torch.zeros(B, unet.channels, H, Wd, device=device)
        x_state = eng.x_in if canvas is None else canvas
        n = x_state[0].numel()
        if share is not None:
            assert not R, 'a shared sampler state does not cover the inpainting plan'
            eng.share_sampler_state(share['eng'])
            state = {k: share[k] for k in self.SHARED_STATE}
        else:
            per_sample = lambda k: torch.zeros(B, n, device=device) if k in buffers else None   # (video: the frame-major clip, as the state)
            state = dict(step_ptr=torch.zeros(1, dtype=torch.int32, device=device), seed_dev=torch.zeros(2, dtype=torch.int32, device=device),
                         # (Philox key lo, hi, global sample index, 0) of every row: _run_stage fills it per call
                         row_keys=torch.zeros(B, 4, dtype=torch.int32, device=device) if self._per_row_noise_keys else None,
                         noise=torch.empty_like(x_state) if inject_noise else None, final=torch.empty_like(x_state),
                         x0_thr=per_sample('x0_thr'), x0_prev=per_sample('x0_prev'), tables=tables())
            assert tuple(state) == self.SHARED_STATE
        coef, step_ptr = state['tables'][0], state['step_ptr']
        eng.bind_step_counter(coef, step_ptr)
        # image stages without inpainting resampling: the timestep-only conditioning chain of the denoiser is evaluated for all steps at
        # once per request (engine.enable_time_table: the table has one row per evaluation of `coef`), each step copies its rows; the
        # video engine builds none and keeps the per-step chain
        step_plan = eng.step_plan
        if TIME_TABLE and not R:
            step_plan = eng.enable_time_table(coef, step_ptr) or step_plan
        zeros = lambda: torch.zeros_like(eng.x_in)
        # (x: the image the sampler steps.  scales / sibling: Imagen's guidance schedules, None for every stage without one, under both samplers;
        # guide / avg / head: Imagen's guidance rescale | projected guidance, its running average and the plan that zeroes it at a run's start;
        # compose: Imagen's composed prompts, the per-call weights [K, B] and masks [K, B, hw] | None that COMPOSE_X0 reads)
        # tile: Imagen's tiled sampling — the geometry with the origins and window weights on the device, and the canvas the low-res image is
        # augmented on before TILES gathers it into the engine's
        if tile is not None:
            tile = dict(tile, origins=tile['origins'].to(device), nw=tile['nw'].to(device), lowres=torch.zeros_like(canvas) if unet.lowres_cond else None)
        return dict(eng=eng, step_plan=step_plan, plan=None, graph=None, coef=coef, **state, x=eng.x_in if canvas is None else canvas, B=B,   # (eng.x_in: after share_sampler_state)
                    key=key, scales=None, sibling=None, guide=None, avg=None, head=None, compose=None, tile=tile,
                    n=n, S=S, R=R, video=video, frames=frames, sample_offset=sample_offset,
                    # inpainting: the known image (video: frame-major clip), normalised, at this stage's size; 1.0 where it is kept
                    known=zeros() if R else None, mask=zeros() if R else None,
                    noise_renoise=zeros() if R and inject_noise else None), True

    def _step_tables(self, idx: int, device, *, solver: Optional[tuple], R: int, inject_noise: bool, guidance: Optional[torch.Tensor]) -> list:
        """The device tables of a stage of this sampler, the step table (`coef`) first: the ancestral step's, inpainting's three, or a
        solver's two — for 'dpmpp_2m' followed by the one row (1, 0, ...) its history copy reads."""
        sched = self.noise_schedulers[idx]
        if solver is not None:
            host = sched.solver_coefficients(*solver, philox=not inject_noise)
        else:
            host = sched.inpaint_coefficients(R, philox=not inject_noise) if R else (sched.step_coefficients(),)
        if guidance is not None:
            host[0][:, 7] = guidance                     # column 7, the pad slot of the step table: read by CFG_X0 (cfg = 2) alone
        tables = [t.to(device) for t in host]
        if solver is not None and solver[0] == 'dpmpp_2m':
            tables.append(torch.tensor([[1., 0., 0., 0., 0., 0., 0., 0.]], device=device))
        return tables

    def _emit_step(self, plan: Plan, st: dict, idx: int, *, cfg: int, cond_scale: float, inject_noise: bool) -> dict:
        """One sampling step of stage `st`, on the sampler state it holds, into `plan`:

            [inpaint.blend]  eng.step_plan  CFG_X0 | GUIDE_X0 (reduce, apply) | COMPOSE_X0  [QUANTILE]  update  [dpmpp_2m.history]  [inpaint.renoise]

        The update is the DDPM_UPDATE launch, or — st['solver'] = (sampler, steps, eta) — one LINCOMB x = w0 x + w1 thr(x0) + w3 x0_prev
        (+ the noise term of 'ddim' at eta > 0), which also emits thr(x0) (`thr1_out`: the next step's self-conditioning input and, for
        'dpmpp_2m', the history) and the unnormalised image (`final_out`, rewritten every step: the last one's is the stage's).
        'dpmpp_2m' hands thr(x0) to `x0_prev` with a second LINCOMB used as a copy — LINCOMB forbids thr1_out aliasing an input of its own
        launch — so that ONE captured graph serves every step.  Allocates only the scratch of these launches, private to the plan."""
        eng, n, R, solver, tables, coef, step_ptr, seed_dev = (st[k] for k in ('eng', 'n', 'R', 'solver', 'tables', 'coef', 'step_ptr', 'seed_dev'))
        B, device, x, tile = st['B'], coef.device, st['x'], st['tile']
        x0, absx0 = (torch.empty(B, n, device=device) for _ in range(2))
        quant = torch.empty(B, device=device)
        scratch = torch.empty(B * ops.ENUMS["IMAGEN_QUANTILE_SCRATCH_WORDS"], dtype=torch.int32, device=device)
        noise_blend = None
        if R:
            noise_blend = torch.zeros_like(eng.x_in) if inject_noise else None
            ops.lincomb(plan, st['known'], eng.x_in, tables[1], step_ptr, B=B, n_per_sample=n, t1=noise_blend, mask=st['mask'], mask_else=eng.x_in,
                        stream_id=idx | 0x100, sample_offset=st['sample_offset'], seed_ptr=seed_dev, label="inpaint.blend")
        if tile is not None:                             # the canvas x_t -> the engine's tile rows
            geo = dict(B=B, C=x.shape[1], H=x.shape[2], W=x.shape[3], h=tile['h'], w=tile['w'])
            ops.tiles(plan, x, eng.x_in, tile['origins'], mode='gather', **geo)
        plan.extend(st['step_plan'])
        guide = st['guide'] if cfg else None             # (an unguided step is CFG_X0's, and leaves the running average alone)
        if tile is not None:
            # CFG_X0 on the tile rows against the gathered x: the tiles' x0 (its |x0| goes to a scratch nobody reads), blended into the canvas's
            EB, tn = eng.src_batch, eng.x_in[0].numel()
            tx0, tabs = (torch.empty(EB, tn, device=device) for _ in range(2))
            ops.cfg_x0(plan, eng.x_in, eng.out, coef, step_ptr, tx0, tabs, B=EB, n_per_sample=tn, cfg=cfg, cond_scale=float(cond_scale),
                       objective=self.pred_objectives[idx])
            ops.tiles(plan, tx0, x0, tile['origins'], mode='blend', nw=tile['nw'], absdst=absx0, **geo)
        elif st['compose'] is not None:
            H, Wd = eng.x_in.shape[-2:]
            ops.compose_x0(plan, eng.x_in, eng.out, coef, step_ptr, x0, absx0, B=B, n_per_sample=n, hw=H * Wd, weights=st['compose']['weights'],
                           masks=st['compose']['masks'], objective=self.pred_objectives[idx])
        elif guide is None:
            ops.cfg_x0(plan, eng.x_in, eng.out, coef, step_ptr, x0, absx0, B=B, n_per_sample=n, cfg=cfg, cond_scale=float(cond_scale),
                       objective=self.pred_objectives[idx])
        else:
            kw = dict(phi=guide[1]) if guide[0] == 'rescale' else dict(eta=guide[1], norm_threshold=guide[2], momentum=guide[3], avg=st['avg'])
            ops.guide_x0(plan, eng.x_in, eng.out, coef, step_ptr, x0, absx0, B=B, n_per_sample=n, cfg=cfg, cond_scale=float(cond_scale),
                         objective=self.pred_objectives[idx], mode=guide[0], **kw)
        dyn = bool(self.dynamic_thresholding[idx])
        if dyn:
            ops.quantile(plan, absx0, quant, scratch, B=B, n=n, q=float(self.dynamic_thresholding_percentile))
        if getattr(self.unets[idx], 'self_cond', False):     # ip.py:2249: each step conditions on the previous step's thresholded x0
            eng.bind_self_cond(st['x0_thr'])
        if solver is not None:
            sampler, _, eta = solver
            # 'dpmpp_2m', the history: x0_prev enters the update as t3 (already thresholded: thr(.) with no quantile is the identity on
            # [-1, 1]), and receives this step's thr(x0) from a copy launch (weights (1, 0, ...) of row 0 of a table of its own)
            ops.lincomb(plan, x, x, tables[1], step_ptr, B=B, n_per_sample=n, t1=x0, q1=quant if dyn else None,
                        t2=st['noise'] if eta > 0. else None, t3=st['x0_prev'], thr_mode=1 if dyn else 2, thr1_out=st['x0_thr'], final=True,
                        final_out=st['final'], advance=True, stream_id=idx, sample_offset=st['sample_offset'], seed_ptr=seed_dev,
                        label=f"{sampler}.update")
            if sampler == 'dpmpp_2m':
                zero_ptr = torch.zeros(1, dtype=torch.int32, device=device)
                ops.lincomb(plan, st['x0_thr'], st['x0_prev'], tables[2], zero_ptr, B=B, n_per_sample=n, label="dpmpp_2m.history")
        else:
            ops.ddpm_update(plan, x, x0, quant if dyn else None, coef, st['noise'], st['final'], step_ptr, B=B, n_per_sample=n,
                            dynamic_threshold=dyn, total_steps=st['T'] * max(R, 1), seed=0, stream_id=idx, sample_offset=st['sample_offset'],
                            seed_ptr=seed_dev, advance=not R, x0_thr=st['x0_thr'], row_keys=None if inject_noise else st['row_keys'])
        if R:
            ops.lincomb(plan, x, x, tables[2], step_ptr, B=B, n_per_sample=n, t1=st['noise_renoise'], advance=True,
                        stream_id=idx | 0x200, sample_offset=st['sample_offset'], seed_ptr=seed_dev, label="inpaint.renoise")
        return dict(quant=quant, x0=x0, noise_blend=noise_blend)

    def _build_stage(self, idx: int, B: int, device, *, cond_scale: float, with_text: bool, inject_noise: bool, sample_offset: int,
                     resample_times: int = 0, frames: int = 0, prompt_frames: tuple = (0, 0), size=None, solver: Optional[tuple] = None,
                     guidance: Optional[torch.Tensor] = None, guide: Optional[tuple] = None, compose: Optional[tuple] = None, tile: Optional[dict] = None):
        """Build (or fetch) the per-timestep plan + graph of stage `idx` for batch B, at image_sizes[idx] or at `size` (an int, or (H, W)):
        form the key, get or make the stage (`_new_stage`), emit its step (`_emit_step`), file it.

        solver = (sampler, steps, eta): a few-step solver on the tables of `solver_coefficients` over a grid of `steps` steps.
        resample_times = R > 0 selects the inpainting plan (ip.py:2237-2275): the device counter then counts INNER iterations
        (timestep i, resample r = R-1..0), every coefficient table has one row per inner iteration, and one launch sequence
        [blend known pixels at level t -> denoiser -> posterior step -> re-noise t_next -> t] serves all of them: the re-noising
        weights are the identity on the rows where the reference skips it, so a single captured graph covers the whole loop.

        guidance = the fp32 [T] guidance scales of a schedule that varies (SampleCall._resolve_guidance): the stage is the
        guided one (2B rows) with CFG_X0 at cfg = 2, which reads the step's scale from column 7 of the step table; `cond_scale` is not
        used.  Where the schedule has steps at exactly 1 — outside a guidance interval — st['sibling'] is the stage `cond_scale = 1`
        builds (B rows, cfg = 0), made here with share = this stage: it runs on this stage's sampler state (SHARED_STATE and the engine's
        x / low-res image) and `_run_stage` replays it on those steps.

        guide = ('rescale', phi) | ('apg', eta, norm_threshold, momentum) (SampleCall._guide_of): the guided steps launch GUIDE_X0 in place of
        CFG_X0; the setting ends the stage's key.  Projected guidance with momentum keeps its running average in st['avg'], zeroed by the
        one-launch plan st['head'] that `_rewind` runs at the start of every run; the unguided sibling neither reads nor writes it.

        compose = (K, masks present) (SampleCall._compose_of): the stage runs (K + 1) B denoiser rows and COMPOSE_X0 in place of CFG_X0, whatever
        `cond_scale` is — the main prompt's weight like every other lives in st['compose']['weights'] (device memory, filled per call by
        `_prepare_stage`, as the masks are), so the key holds no scale and ends with (K, masks present).

        tile = the tile_geometry of a tiled stage (SampleCall._tiles_of): `size` stays the canvas's, the engine runs T B (2 T B) rows at the
        tile's size, and the step is TILES gather, the denoiser, CFG_X0 on the tile rows, TILES blend, then the canvas's threshold and update.
        The geometry is a function of (canvas, tile shape, overlap, blend): the key ends with ('tile', (tile shape, overlap, blend))."""
        sched = self.noise_schedulers[idx]
        T, R = sched.num_timesteps if solver is None else solver[1], resample_times
        assert solver is None or not R, 'the solvers do not cover inpainting'
        assert guidance is None or (not R and tuple(guidance.shape) == (T,) and guidance.dtype == torch.float32)
        assert guide is None or (not R and (guidance is not None or cond_scale != 1.)), 'guidance rescale / projected guidance act on guided steps'
        suffix = () if guide is None else (('guide', guide),)     # (a call without the keywords keeps the key it always had)
        if tile is not None:
            assert guide is None and compose is None and not R, 'a tiled stage takes the plain guided step'
            suffix += (('tile', ((tile['h'], tile['w']), (tile['oy'], tile['ox']), tile['blend'])),)
        size = self.image_sizes[idx] if size is None else size
        two = solver is not None and solver[0] == 'dpmpp_2m'
        buffers = ('x0_thr',) * bool(two or getattr(self.unets[idx], 'self_cond', False)) + ('x0_prev',) * two
        key_at = lambda scale: (idx, B, size, str(device), float(scale), with_text, inject_noise, sample_offset, self.dynamic_thresholding[idx],
                                self.pred_objectives[idx], self.dynamic_thresholding_percentile, resample_times, frames, prompt_frames,
                                self._lane, solver)

        def stage(key, cfg, scale, scales=None, share=None, prompts=1):
            st, built = self._new_stage(key, idx, B, device, cfg=bool(cfg), prompts=prompts, with_text=with_text, inject_noise=inject_noise, sample_offset=sample_offset,
                                        resample_times=R, frames=frames, prompt_frames=prompt_frames, size=size, buffers=buffers, share=share, tile=tile,
                                        tables=functools.partial(self._step_tables, idx, device, solver=solver, R=R, inject_noise=inject_noise,
                                                                 guidance=guidance))
            if built:
                # ('dpmpp_2m': the first step of a run has no history: its row is first order, wherever skip_steps starts the run — _rewind)
                st.update(plan=Plan(f"stage{idx}-step"), T=T, solver=solver, scales=scales, weights=st['tables'][1] if solver is not None else None,
                          weights_at=(lambda start: sched.solver_coefficients(*solver, philox=not inject_noise, start=start)[1]) if two else None,
                          weights_start=0, guide=guide if cfg else None)
                if cfg and guide is not None and guide[0] == 'apg' and guide[3] != 0.:
                    st['avg'], st['head'] = torch.zeros(B, st['n'], device=device), Plan(f"stage{idx}-head")
                    ops.memset32(st['head'], st['avg'], 0)
                if compose is not None:
                    H, Wd = st['eng'].x_in.shape[-2:]
                    st['compose'] = dict(K=compose[0], weights=torch.zeros(compose[0], B, device=device),
                                         masks=torch.ones(compose[0], B, H * Wd, device=device) if compose[1] else None)
                st.update(self._emit_step(st['plan'], st, idx, cfg=cfg, cond_scale=scale, inject_noise=inject_noise))
                self._stages[key] = st
            return st, built

        if compose is not None:
            assert guidance is None and guide is None and not R, 'composed prompts take the plain guided step'
            return stage(key_at(0.) + ('compose', (int(compose[0]), bool(compose[1]))), 1, cond_scale, prompts=int(compose[0]))[0]
        if guidance is None:
            return stage(key_at(cond_scale) + suffix, int(cond_scale != 1.), cond_scale)[0]
        key = key_at(cond_scale) + (('guidance', guidance.numpy().tobytes()),) + suffix   # (a call without a schedule keeps the key it always had)
        st, built = stage(key, 2, cond_scale, scales=[float(v) for v in guidance])
        if built and 1. in st['scales']:
            st['sibling'] = stage(key_at(1.) + (('shares', key),), 0, 1., share=st)[0]
        return st

    # ---- the run loop of both samplers, and what they put into it
    @staticmethod
    def _draw(st, noise_fn, tag, like):
        """Injected Gaussian draw for the internal buffer `like`; videos are drawn in the reference's (b, c, f, h, w) layout."""
        if not st['video']:
            return noise_fn(tag, tuple(like.shape))
        b, f, c, h, w = like.shape
        return noise_fn(tag, (b, c, f, h, w)).permute(0, 2, 1, 3, 4)

    @staticmethod
    def _seed_words(seed: int) -> tuple:
        """A Philox key as the two 31-bit words the kernels take (seed_ptr, row_keys)."""
        return seed & 0x7FFFFFFF, (seed >> 31) & 0x7FFFFFFF

    @staticmethod
    def _stage_output(st, state, complete: bool):
        """The stage's [0, 1] result: what the last step's kernel wrote, or — a truncated loop (tests) — the same epilogue on the state
        (ip.py:2281-2288, el.py:540-545); then the paste of the known pixels (ip.py:2283-2288, el.py:542-545)."""
        out = st['final'] if complete else (state.clamp(-1., 1.) + 1) * 0.5
        if st['R']:
            out = torch.where(st['mask'] != 0, (st['known'] + 1) * 0.5, out)
        return out

    def _rewind(self, st, skip: int, init_images):
        """The sampler state behind the fresh x_T ~ N(0, I), for a run that starts at timestep `skip`."""
        if init_images is not None:
            st['x'].add_(init_images)                   # ip.py:2205-2206
        if st['head'] is not None:
            st['head'].run()                            # projected guidance: the running average starts every run at zero
        if st['x0_thr'] is not None:
            st['x0_thr'].zero_()                        # no x0 estimate yet: the first step self-conditions on zeros (ip.py:2210, 1542)
        if st['x0_prev'] is not None:                   # 'dpmpp_2m': no history yet, and the run's first row is first order
            st['x0_prev'].zero_()
            if st['weights_start'] != skip:
                st['weights'].copy_(st['weights_at'](skip))
                st['weights_start'] = skip
        st['step_ptr'].fill_(skip * max(st['R'], 1))    # ip.py:2228-2229: the skipped timesteps are simply never run

    def _plans_of_steps(self, st, steps: range) -> list:
        """(stage, 'plan' | 'last') of every step: the stage's one plan, but on the unguided steps of a guidance schedule (st['scales'], read
        on the host) its B-row sibling's, which runs on the same state."""
        return [(st['sibling'] if st['sibling'] is not None and st['scales'][i] == 1. else st, 'plan') for i in steps]

    def _capture(self, st, plans: list, rewind: Callable, stream):
        """Warm-up outside capture (sets kernel attributes) from the run's own row, then rewind and capture, for each plan the run launches."""
        for s in ([st] if st['sibling'] is None else [s for s in (st, st['sibling']) if any(p[0] is s for p in plans)]):
            if s['graph'] is None:
                s['plan'].run()
                rewind()
                torch.cuda.synchronize()
                s['graph'] = ops.Graph(s['plan'], stream)

    def _draw_step_noise(self, st, draw: Callable, stage: int, i: int, r: int):
        """The injected draws that precede inner iteration (i, r); the tags and their order are the contract of `noise_fn`."""
        if st['R']:
            st['noise_blend'].copy_(draw(("inpaint", stage, i, r), st['noise']))
            st['noise'].copy_(draw(("step", stage, i, r), st['noise']))
            if r > 0 and i < st['T'] - 1:                # the reference draws no re-noising sample otherwise (ip.py:2268)
                st['noise_renoise'].copy_(draw(("renoise", stage, i, r), st['noise']))
        elif st['solver'] is None or st['solver'][2] > 0.:          # (the deterministic solvers draw nothing after the initial image)
            st['noise'].copy_(draw(("step", stage, i), st['noise']))

    @torch.no_grad()
    def _run_stage(self, st, *, noise_fn: Optional[Callable], stage: int, seed: int, use_graph: bool = True, use_tqdm: bool = False,
                      max_steps: Optional[int] = None, trace: Optional[list] = None, init_images: Optional[torch.Tensor] = None,
                      skip_steps: Optional[int] = None):
        """One stage under either sampler (ip.py:2167-2289, el.py:393-545): the initial noise (+ init_images), the steps from `skip_steps`
        on (each run `inpaint_resample_times` times when st is an inpainting stage), clamp + unnormalise (done by the last step's kernel)
        and the final paste of the known pixels.  What the samplers differ in: `_rewind` (the state at the start of a run),
        `_plans_of_steps` (which captured plan a step replays), `_capture` (warm-up and capture), `_draw_step_noise` (the injected draws)."""
        x, T, R, B = st['x'], st['T'], st['R'], st['B']
        stream = torch.cuda.current_stream()
        skip = skip_steps or 0
        assert 0 <= skip < T, f'skip_steps must leave at least one {self._step_noun}'
        spans = _seed_spans(seed, B, st['sample_offset'])
        assert not (R and len(spans) > 1), 'merged requests do not cover inpainting (its re-noising launches take one key per batch)'
        draw = functools.partial(self._draw, st, noise_fn)
        if noise_fn is None:
            init = Plan(self._plan_prefix + "init-noise")
            for sd, r0, cnt, i0 in spans:               # (one span per merged request: its own key, its own sample indices)
                ops.randn(init, x[r0:r0 + cnt], seed=sd, stream_id=stage, tag=TAG_INIT, sample_offset=i0)

        def rewind():
            if noise_fn is not None:
                x.copy_(draw(("init", stage), x))
            else:
                init.run()
            self._rewind(st, skip, init_images)

        st['seed_dev'].copy_(torch.tensor(self._seed_words(spans[0][0]), dtype=torch.int32))
        if st['row_keys'] is not None:
            keys = torch.zeros(B, 4, dtype=torch.int64)
            for sd, r0, cnt, i0 in spans:
                keys[r0:r0 + cnt, 0], keys[r0:r0 + cnt, 1] = self._seed_words(sd)
                keys[r0:r0 + cnt, 2] = torch.arange(i0, i0 + cnt)
            st['row_keys'].copy_(keys.to(torch.int32))
        steps = T - skip if max_steps is None else min(T - skip, max_steps)
        it = range(skip, skip + steps)
        plans = self._plans_of_steps(st, it)
        rewind()
        if use_graph:
            self._capture(st, plans, rewind, stream)
        launches = [s[self._GRAPH_OF[p]].launch if use_graph else s[p].run for s, p in plans]
        if use_tqdm:
            try:
                from tqdm.auto import tqdm
                it = tqdm(it, desc='sampling loop time step', total=steps)
            except ImportError:
                pass
        for i, launch in zip(it, launches):
            for r in reversed(range(max(R, 1))):
                if noise_fn is not None:
                    self._draw_step_noise(st, draw, stage, i, r)
                launch()
                if trace is not None:
                    trace.append(x.clone())
        return self._stage_output(st, x, skip + steps == T)

    # ---- the reference's step-level sampler methods (ip.py:2042-2289) ------------------------------------------------------
    # `sample()` below runs a whole stage as one captured graph per timestep and never calls these.  They are the reference's
    # per-step API, kept for callers that drive single steps themselves (custom loops, guidance experiments): the denoiser
    # evaluation goes through the same kernel plan (Unet.forward_with_cond_scale), the O(B*3*S*S) posterior arithmetic around it is
    # plain device-side tensor code with the reference's signatures, argument meaning and return values.
    def resize_to(self, img, size, **kwargs):
        """resize_image_to with this model's resize_mode (ip.py:152-168, 1924)."""
        assert not kwargs or self.is_video, 'frame arguments are for video stages'
        if img.ndim == 5:                                # resize_video_to (iv.py:134-156): (b, c, f, h, w), optional target_frames
            frames = kwargs.get('target_frames') or img.shape[2]
            if tuple(img.shape[-3:]) == (frames, size, size):
                return img
            return F.interpolate(img, (frames, size, size), mode=self.resize_mode)
        return img if img.shape[-1] == size else F.interpolate(img, size, mode=self.resize_mode)

    def _step_conditioning_checks(self, unet, cond_video_frames, post_cond_video_frames, cond_scale):
        assert not (cond_scale != 1. and not self.can_classifier_guidance), \
            'imagen was not trained with conditional dropout, and thus one cannot use classifier free guidance (cond_scale anything other than 1)'
        # (prompt frames given to an image cascade are ignored, as in the reference: ip.py:2057-2070 builds video_kwargs only if is_video)

    @torch.no_grad()
    def p_mean_variance(self, unet, x, t, *, noise_scheduler, text_embeds=None, text_mask=None, cond_images=None, cond_video_frames=None,
                        post_cond_video_frames=None, lowres_cond_img=None, self_cond=None, lowres_noise_times=None, cond_scale=1.,
                        model_output=None, t_next=None, pred_objective='noise', dynamic_threshold=True):
        """ip.py:2042-2110: denoiser output (or `model_output`) -> x_0 estimate -> threshold -> posterior (mean, variance,
        log variance) of x_{t_next}; returns that triple and the thresholded x_0."""
        self._step_conditioning_checks(unet, cond_video_frames, post_cond_video_frames, cond_scale)
        pred = model_output
        if pred is None:
            video_kwargs = dict(cond_video_frames=cond_video_frames, post_cond_video_frames=post_cond_video_frames) if self.is_video else {}
            pred = unet.forward_with_cond_scale(x, noise_scheduler.get_condition(t), text_embeds=text_embeds, text_mask=text_mask,
                                                cond_images=cond_images, self_cond=self_cond, cond_scale=cond_scale,
                                                lowres_cond_img=lowres_cond_img,
                                                lowres_noise_times=self.lowres_noise_schedule.get_condition(lowres_noise_times),
                                                **video_kwargs)                      # ip.py:2057-2070
        if pred_objective == 'noise':
            x_start = noise_scheduler.predict_start_from_noise(x, t=t, noise=pred)
        elif pred_objective == 'x_start':
            x_start = pred
        elif pred_objective == 'v':
            x_start = noise_scheduler.predict_start_from_v(x, t=t, v=pred)
        else:
            raise ValueError(f'unknown objective {pred_objective}')
        if dynamic_threshold:
            # per-sample percentile of |x_0|, never below 1: clamp to it and rescale into [-1, 1] (Imagen paper, appendix)
            s = torch.quantile(x_start.flatten(1).abs(), self.dynamic_thresholding_percentile, dim=-1).clamp(min=1.)
            s = s.reshape(-1, *((1,) * (x_start.ndim - 1)))
            x_start = x_start.clamp(-s, s) / s
        else:
            x_start = x_start.clamp(-1., 1.)
        return noise_scheduler.q_posterior(x_start=x_start, x_t=x, t=t, t_next=t_next), x_start

    @torch.no_grad()
    def p_sample(self, unet, x, t, *, noise_scheduler, t_next=None, text_embeds=None, text_mask=None, cond_images=None,
                 cond_video_frames=None, post_cond_video_frames=None, cond_scale=1., self_cond=None, lowres_cond_img=None,
                 lowres_noise_times=None, pred_objective='noise', dynamic_threshold=True):
        """ip.py:2112-2165: one ancestral step, x_{t_next} = mean + [t_next != 0] * exp(log_var / 2) * eps; returns it and x_0."""
        (mean, _, log_var), x_start = self.p_mean_variance(
            unet, x=x, t=t, t_next=t_next, noise_scheduler=noise_scheduler, text_embeds=text_embeds, text_mask=text_mask,
            cond_images=cond_images, cond_video_frames=cond_video_frames, post_cond_video_frames=post_cond_video_frames,
            cond_scale=cond_scale, self_cond=self_cond, lowres_cond_img=lowres_cond_img, lowres_noise_times=lowres_noise_times,
            pred_objective=pred_objective, dynamic_threshold=dynamic_threshold)
        noise = torch.randn_like(x)
        last = (t_next == 0) if isinstance(noise_scheduler, GaussianDiffusionContinuousTimes) else (t == 0)
        nonzero = (1 - last.float()).reshape(x.shape[0], *((1,) * (x.ndim - 1)))
        return mean + nonzero * (0.5 * log_var).exp() * noise, x_start

    @torch.no_grad()
    def p_sample_loop(self, unet, shape, *, noise_scheduler, lowres_cond_img=None, lowres_noise_times=None, text_embeds=None,
                      text_mask=None, cond_images=None, cond_video_frames=None, post_cond_video_frames=None, inpaint_images=None,
                      inpaint_videos=None, inpaint_masks=None, inpaint_resample_times=5, init_images=None, skip_steps=None, cond_scale=1,
                      pred_objective='noise', dynamic_threshold=True, use_tqdm=True):
        """ip.py:2167-2289 with the reference's signature: the loop of one stage, step by step through `p_sample` (torch's
        generator supplies the noise, in the reference's draw order).  `sample()` is the fast way to run a stage."""
        device = self.device
        batch = shape[0]
        resize_kwargs = dict(target_frames=shape[-3]) if len(shape) == 5 else {}      # ip.py:2198-2200
        img = torch.randn(shape, device=device)
        if init_images is not None:
            img = img + init_images
        if inpaint_videos is not None:                   # ip.py:2214
            inpaint_images = inpaint_videos
        inpainting = inpaint_images is not None and inpaint_masks is not None
        if inpainting:
            known = self.resize_to(self.normalize_img(inpaint_images), shape[-1], **resize_kwargs)
            keep = self.resize_to(inpaint_masks[:, None].float(), shape[-1], **resize_kwargs).bool()
        steps = noise_scheduler.get_sampling_timesteps(batch, device=device)[(skip_steps or 0):]
        if use_tqdm:
            try:
                from tqdm.auto import tqdm
                steps = tqdm(steps, desc='sampling loop time step', total=len(steps))
            except ImportError:
                pass
        x_start = None
        for times, times_next in steps:
            final_step = bool(torch.all(times_next == 0))
            for r in reversed(range(inpaint_resample_times if inpainting else 1)):
                if inpainting:       # known region at this step's noise level
                    img = torch.where(keep, noise_scheduler.q_sample(known, t=times)[0], img)
                img, x_start = self.p_sample(unet, img, times, t_next=times_next, text_embeds=text_embeds, text_mask=text_mask,
                                       cond_images=cond_images, cond_scale=cond_scale, lowres_cond_img=lowres_cond_img,
                                       self_cond=x_start if getattr(unet, 'self_cond', False) else None,
                                       lowres_noise_times=lowres_noise_times, noise_scheduler=noise_scheduler,
                                       pred_objective=pred_objective, dynamic_threshold=dynamic_threshold,
                                       cond_video_frames=cond_video_frames, post_cond_video_frames=post_cond_video_frames)
                if inpainting and r > 0 and not final_step:      # resample: back up to this step's level (RePaint)
                    img = noise_scheduler.q_sample_from_to(img, times_next, times)
        img = img.clamp(-1., 1.)
        if inpainting:
            img = torch.where(keep, known, img)
        return self.unnormalize_img(img)

    # ---- public sampling API (ip.py:2291-2498) ------------------------------------------------------------------
    @torch.no_grad()
    def sample(
        self,
        texts: Optional[List[str]] = None,
        text_masks=None,
        text_embeds=None,
        video_frames=None,
        cond_images=None,
        cond_video_frames=None,
        post_cond_video_frames=None,
        inpaint_videos=None,
        inpaint_images=None,
        inpaint_masks=None,
        inpaint_resample_times=5,
        init_images=None,
        skip_steps=None,
        batch_size=1,
        cond_scale=1.,
        lowres_sample_noise_level=None,
        start_at_unet_number=1,
        start_image_or_video=None,
        stop_at_unet_number=None,
        return_all_unet_outputs=False,
        return_pil_images=False,
        device=None,
        use_tqdm=True,
        use_one_unet_in_gpu=True,
        *,
        noise_fn: Optional[Callable] = None,   # extension: injectable Gaussian noise (parity tests), tags as in oracle/sampler_oracle.py
        seed: Optional[int] = None,            # extension: Philox seed of this call (sample_requests passes [(seed, rows), ...]: one key per merged request)
        sample_offset: int = 0,                # extension: global index of sample 0 (batch sharding)
        use_graph: bool = True,
        max_steps: Optional[int] = None,
        conditioning: Optional[Conditioning] = None,   # extension: handle from prepare_conditioning() instead of texts / text_embeds
        negative_texts: Optional[List[str]] = None,    # extension: a second prompt on the null rows of guidance (batch 1 or the prompts' batch):
        negative_text_embeds=None,                     #   every guided evaluation is neg + (pos - neg) * cond_scale
        negative_text_masks=None,
        image_shapes=None,                             # extension: one (H, W) per unet for this call instead of image_sizes (image cascades):
                                                       #   rectangular sampling; sides divisible by each unet's downsamples, stages never shrink
        sampler: str = 'ddpm',                         # extension: 'ddpm' (the reference's ancestral step, one per training timestep), or a few-step
        sample_steps=None,                             #   solver on the same checkpoint: 'dpmpp_2m' (DPM-Solver++ 2M) | 'ddim', in `sample_steps`
        eta: float = 0.,                               #   steps (an int or one per unet; None: the unet's timesteps); eta: 'ddim' only, 0 .. 1
        guidance_schedule=None,                        # extension: the guidance scale of every step in place of the fixed cond_scale: a callable
                                                       #   f(t) -> float (t = 1: pure noise) or a sequence with one entry per denoiser evaluation
        guidance_interval=None,                        # extension: (t_lo, t_hi): the steps with t outside it run unguided (scale 1, the B-row plan);
                                                       #   both: one value for every unet, or a tuple with one entry (or None) per unet.
                                                       #   Every distinct per-step vector is a cached stage of its own (engine, time table, graph;
                                                       #   with unguided steps also the B-row sibling) that is kept, as every stage is: a sweep
                                                       #   over many schedules grows the cache — sample from a fresh Imagen, or clear `_stages`
        guidance_rescale=None,                         # extension: phi in [0, 1] of guidance rescale (Lin et al. 2023): the guided model output
                                                       #   brought back to the conditional one's per-sample standard deviation, blended by phi
        guidance_apg=None,                             # extension: dict(eta=0., norm_threshold=None, momentum=0.) of adaptive projected guidance
                                                       #   (Sadat et al. 2024), in x0 space; both: one value for every unet, or a tuple with one
                                                       #   entry (or None) per unet; not both on one unet.  They act on the guided steps (GUIDE_X0
                                                       #   in place of CFG_X0); a distinct setting is a cached stage of its own
        compose=None,                                  # extension: composed prompts (Liu et al. 2022).  A list of up to 3 dicts, each one more prompt:
                                                       #   dict(text_embeds= | texts=, text_masks=, weight=, mask=).  The call's own prompt is prompt 0 at
                                                       #   weight cond_scale; the guided output is nul + sum_k w_k m_k (cond_k - nul) (COMPOSE_X0 in place
                                                       #   of CFG_X0, (K + 1) B denoiser rows).  weight: a float, a per-unet tuple or a [B] tensor, negative =
                                                       #   negation; mask: [B | 1, H, W] or [H, W] in [0, 1], resized to every stage (nearest): regional
                                                       #   prompts.  Weights and masks are per-call state: every call of one K shares the stage and its graph
        compose_mask=None,                             #   ... the mask of the call's own prompt
        tile_shapes=None,                              # extension: tiled sampling (MultiDiffusion, Bar-Tal et al. 2023).  One (h, w), an int or None, or a
                                                       #   tuple of one per unet (a pair of ints is ONE shape): every step runs the denoiser on overlapping
                                                       #   h x w windows of the stage's canvas (image_shapes / image_sizes) — T B rows, 2 T B under guidance —
                                                       #   and blends their x0 into one canvas x0 (TILES); threshold, solver and noise act on the canvas
        tile_overlap=None,                             #   ... an int or (oy, ox), one or per unet; None: a quarter of the tile side
        tile_blend='ramp',                             #   ... the window of the blend: 'ramp' (linear over the overlap) | 'uniform'
    ):
        return self._sample(self._call(**{k: v for k, v in locals().items() if k != 'self'}))   # (the keywords, as given)

    # ---- one call: resolve (nothing is built or launched) -> per stage: prepare, run --------------------------------------------
    def _sampling_device(self, device) -> torch.device:
        """The device of one call (None: the model's), refused where no plan can be launched."""
        device = torch.device(device) if device is not None else self.device
        if device.type not in _SAMPLING_DEVICE_TYPES:
            raise RuntimeError("imagen_pytorch_amd.Imagen.sample runs on MI355X only (move the module to 'cuda'); there is no CPU path")
        return device

    def _to_internal(self, t):
        """(b, c, f, h, w) <-> (b, f, c, h, w) of a video cascade (the permutation is its own inverse); images as they are."""
        return t.permute(0, 2, 1, 3, 4).contiguous() if self.is_video else t

    def _resize(self, im, size):
        """resize_image_to (ip.py:152-168, 1924) to a square `size`, or to size = (H, W)."""
        hw = (size, size) if isinstance(size, int) else tuple(size)
        return im if tuple(im.shape[-2:]) == hw else F.interpolate(im, hw, mode=self.resize_mode)

    def _resize_clip(self, v, size, f):
        """resize_video_to (iv.py:134-156) of a (b, c, f', h, w) clip to f frames of size x size — nearest over all three axes —
        returned in the internal frame-major layout."""
        if tuple(v.shape[-3:]) != (f, size, size):
            v = F.interpolate(v, (f, size, size), mode='nearest')
        return self._to_internal(v)

    def _prepare_stage(self, c: _Call, idx: int) -> dict:
        """Stage `idx` made ready for `_run_stage`: the prompt frames at its frame rate, the stage itself (built or fetched), its conditioning
        images / frames, the known pixels at its size, the augmented low-res image (one launch sequence) and the static conditioning plan."""
        unet, device, batch_size, noise_fn = self.unets[idx], c.device, c.batch_size, c.noise_fn
        assert not isinstance(unet, NullUnet), 'one cannot sample from null / placeholder unets'
        cs = c.cond_scale[idx]
        assert not (cs != 1. and not self.can_classifier_guidance), \
            'imagen was not trained with conditional dropout, and thus one cannot use classifier free guidance (cond_scale anything other than 1)'
        with_text = c.text_embeds is not None and unet.cond_on_text
        prompts = [None, None]
        if isinstance(unet, Unet3D):                # ip.py:2417-2434: the same prompt frames for every stage, at the stage's frame rate
            tds = self.temporal_downsample_factor[idx]
            for k, v in enumerate((c.cond_video_frames, c.post_cond_video_frames)):
                if v is not None and self.resize_cond_video_frames and tds != 1:     # scale_video_time, iv.py:158-178
                    assert v.shape[2] % tds == 0, f'trying to temporally downsample a conditioning video frames of length ' \
                                                  f'{v.shape[2]} by {tds}, however it is not neatly divisible'
                    v = F.interpolate(v.float(), (v.shape[2] // tds, v.shape[-2], v.shape[-1]), mode='nearest')
                prompts[k] = v
        extra = {} if c.sigma_overrides is None else dict(sigma_overrides=c.sigma_overrides)
        if c.solver is not None:
            extra['solver'] = c.solver[idx]
        if c.guidance is not None and c.guidance[idx] is not None:
            extra['guidance'] = c.guidance[idx]
        if c.guide is not None and c.guide[idx] is not None and (cs != 1. or 'guidance' in extra):     # (an unguided stage has nothing to rescale)
            extra['guide'] = c.guide[idx]
        comp = c.composed if with_text else None
        if comp is not None:
            extra['compose'] = (comp['K'], comp['masks'] is not None)
        tile = None if c.tiles is None else c.tiles[idx]
        if tile is not None:
            extra['tile'] = tile
        st = self._stage(idx, batch_size, device, cond_scale=cs, with_text=with_text, inject_noise=noise_fn is not None,
                         sample_offset=c.sample_offset, resample_times=c.inpaint_resample_times if c.known is not None else 0,
                         frames=c.frames // self.temporal_downsample_factor[idx] if isinstance(unet, Unet3D) else 0,
                         prompt_frames=tuple(0 if v is None else v.shape[2] for v in prompts), size=c.sizes[idx], **extra)
        eng = st['eng']
        S = st['S']
        assert not (getattr(unet, 'has_cond_image', False) ^ (c.cond_images is not None)), \
            'you either requested to condition on an image on the unet, but the conditioning image is not supplied, or vice versa'   # ip.py:1555
        # (a stage with a guidance schedule that has unguided steps: its B-row sibling reads the same sampler state, and is conditioned alike)
        engines = [eng] if st['sibling'] is None else [eng, st['sibling']['eng']]
        for e in engines:
            if c.cond_images is not None:
                e.set_cond_images(c.cond_images)
            if prompts[0] is not None or prompts[1] is not None:
                e.set_cond_video_frames(*prompts)
        if c.known is not None and st['video']:
            st['known'].copy_(self._resize_clip(c.known, S, st['frames']))
            st['mask'].copy_(self._resize_clip(c.known_mask, S, st['frames']).bool().expand(-1, -1, self.channels, -1, -1))
        elif c.known is not None:
            st['known'].copy_(self._resize(c.known, S))
            st['mask'].copy_(self._resize(c.known_mask, S).bool().expand(-1, self.channels, -1, -1))
        lowres_logsnr = None
        if unet.lowres_cond:
            img = c.img
            assert img is not None
            a, s, lsnr = self.lowres_noise_schedule.q_sample_coefficients(c.level)
            # Imagen conditions on the log-SNR of the augmentation level (ip.py:2081); ElucidatedImagen.sample passes the
            # raw level (elucidated_imagen.py:700, 728): `_lowres_time_raw`
            lowres_logsnr = torch.full((eng.src_batch,), c.level if self._lowres_time_raw else lsnr, dtype=torch.float32)
            # (a tiled stage: the low-res image is resized and augmented once, on the canvas; one TILES gather then fills the engine's tile rows)
            lowres_out = eng.lowres_in if tile is None else st['tile']['lowres']
            aug = torch.empty_like(lowres_out)
            if noise_fn is not None:
                aug.copy_(self._draw(st, noise_fn, ("lowres", idx), aug))
            prep = Plan("lowres-prep")
            if noise_fn is None:
                for sd, r0, cnt, i0 in _seed_spans(c.seed, batch_size, c.sample_offset):
                    ops.randn(prep, aug[r0:r0 + cnt], seed=sd, stream_id=idx, tag=TAG_LOWRES, sample_offset=i0)
            src = img if self.auto_normalize_img else (img + 1) * 0.5                  # kernel normalises [0,1] -> [-1,1]
            if st['video'] and src.shape[1] != aug.shape[1]:
                # a stage sampled at a lower frame rate feeds this one: nearest over the frame axis (resize_video_to,
                # iv.py:134-156); once per stage
                src = src[:, nearest_indices(src.shape[1], aug.shape[1]).to(src.device)]
            if self.resize_mode != 'nearest' and tuple(src.shape[-2:]) != tuple(lowres_out.shape[-2:]):
                # LOWRES_PREP resizes with nearest in-kernel; any other mode is resized here, once per stage, and the kernel's
                # own resize becomes the identity.  The resize acts on the [0, 1] image as in ip.py:2444-2446 (normalisation after).
                src = self._resize(img, S) if self.auto_normalize_img else (self._resize(img, S) + 1) * 0.5
            src = src.contiguous()
            # frames are independent images for the nearest resize (resize_video_to with unchanged frame count, iv.py:134-156)
            as_images = lambda t: t.reshape(-1, *t.shape[-3:])
            ops.lowres_prep(prep, as_images(src), as_images(aug), as_images(lowres_out), alpha=a, sigma=s)
            if tile is not None:
                ops.tiles(prep, lowres_out, eng.lowres_in, st['tile']['origins'], mode='gather', B=batch_size, C=lowres_out.shape[1],
                          H=lowres_out.shape[2], W=lowres_out.shape[3], h=tile['h'], w=tile['w'])
            prep.keep += [src, aug, lowres_out]
            prep.run()
        if comp is not None:                         # the call's weights and masks, into the buffers COMPOSE_X0 reads: no launch list changes
            st['compose']['weights'].copy_(comp['weights'][idx])
            if comp['masks'] is not None:
                H, Wd = eng.x_in.shape[-2:]
                for k, m in enumerate(comp['masks']):
                    if m is None:
                        st['compose']['masks'][k].fill_(1.)
                    else:                             # nearest, as the cascade resizes its images (nearest_indices), once per stage and call
                        m = m[:, nearest_indices(m.shape[1], H)][:, :, nearest_indices(m.shape[2], Wd)]
                        st['compose']['masks'][k].copy_(m.expand(batch_size, -1, -1).reshape(batch_size, H * Wd))
        cond = c.conditioning
        stamp = None if cond is None else (cond.token, None if lowres_logsnr is None else float(lowres_logsnr[0]))
        # (a tiled stage: engine row t B + b is tile t of sample b, so the prompts — and the negative prompt's rows — repeat per tile)

        def per_tile(t, keep_one=False):
            """A per-sample conditioning tensor for the engine's T B samples; keep_one: a batch-1 tensor stays batch 1 (the negative prompt, which
            the engine repeats over its samples itself)."""
            if tile is None or t is None or (keep_one and t.shape[0] == 1):
                return t
            return t.repeat(tile['T'], *((1,) * (t.ndim - 1)))

        for eng in engines:
            rows, eb = eng.R, eng.src_batch
            keep = torch.ones(rows, dtype=torch.bool)
            if rows > eb:
                keep[rows - eb:] = False             # the last B rows = null-conditioned CFG branch (cond_drop_prob = 1, ip.py:1521)
            if stamp is None or getattr(eng, '_cond_stamp', None) != stamp:
                neg_kw = {}
                if c.neg_embeds is not None and with_text and rows > eb:                  # (a stage at cond_scale 1 has no null rows)
                    neg_kw = dict(negative_text_embeds=per_tile(c.neg_embeds, True), negative_text_mask=per_tile(c.neg_masks, True), negative_rows=c.neg_rows)
                if comp is not None:
                    neg_kw['extra_prompts'] = comp['prompts']
                eng.set_conditioning(text_embeds=per_tile(c.text_embeds) if with_text else None, text_mask=per_tile(c.text_masks) if with_text else None,
                                     keep=keep, lowres_noise_times=lowres_logsnr, **neg_kw)
                eng.static_runs = getattr(eng, 'static_runs', 0) + 1
            eng._cond_stamp = stamp
        return st

    @torch.no_grad()
    def _sample(self, c: _Call):
        """The one private entry of sample(), sample_requests and the sample_pipelined workers."""
        with self._eval_mode():
            self._resolve(c)
            device = c.device
            stream = self._streams.get((self._lane, str(device)))
            if stream is None:
                stream = self._streams[(self._lane, str(device))] = torch.cuda.Stream(device=device)
            outputs = []
            # inputs were produced on the caller's stream: order this lane's stream behind it (no device-wide drain — other lanes keep running)
            stream.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.device(device), torch.cuda.stream(stream):
                for idx in range(c.start_at_unet_number - 1, len(self.unets)):
                    st = self._prepare_stage(c, idx)
                    S = st['S']
                    timing = os.environ.get("IMAGEN_TIMING")
                    if timing:
                        stream.synchronize()
                        import time as _time
                        t_stage = _time.perf_counter()
                    init = c.init_images[idx]
                    out = self._run_stage(st, noise_fn=c.noise_fn, stage=idx, seed=c.seed, use_graph=c.use_graph, use_tqdm=c.use_tqdm,
                                          max_steps=c.max_steps, skip_steps=c.skip_steps[idx],
                                          init_images=None if init is None else
                                          (self._resize_clip(init, S, st['frames']) if st['video'] else self._resize(init, S)))
                    if timing:
                        stream.synchronize()
                        dt = _time.perf_counter() - t_stage
                        self.last_stage_seconds = getattr(self, "last_stage_seconds", {})
                        self.last_stage_seconds[idx] = dt
                        print(f"[imagen] stage {idx} ({'x'.join(str(v) for v in st['eng'].HW)}, rows {st['eng'].R}): {dt * 1e3:.1f} ms for {st['T'] if c.max_steps is None else min(st['T'], c.max_steps)} steps "
                              f"({len(st['plan'])} launches/step)", flush=True, file=__import__('sys').stderr)
                    c.img = out.clone()                  # internal layout (videos: frame-major), feeds the next stage's low-res conditioning
                    if not self.auto_normalize_img:
                        c.img = c.img * 2 - 1
                    outputs.append(self._to_internal(c.img) if st['video'] else c.img)
                    if c.stop_at_unet_number is not None and c.stop_at_unet_number == idx + 1:
                        break
            stream.synchronize()
        if c.return_pil_images:                              # ip.py:2488-2498: a list of PIL images (one list per unet with return_all_unet_outputs)
            pil = [_to_pil_images(o) for o in (outputs if c.return_all_unet_outputs else outputs[-1:])]
            return pil if c.return_all_unet_outputs else pil[-1]
        return outputs if c.return_all_unet_outputs else outputs[-1]
