"""Multi-GPU sampling: one process per GPU, batch sharded by independent samples, ONE collective.

The sampling path has no cross-sample interaction (all norms are per pixel / token / sample, the dynamic
threshold quantile is per sample — SURVEY.md §8e), so every rank runs the whole cascade on its shard with its
own hipGraphs and the only exchange is a single RCCL all-gather of the final images over xGMI
(`torch.distributed` backend "nccl" = RCCL on ROCm).  The reference has no counterpart: under `accelerate
launch` each rank just samples independently (trainer.py:947-961).

Noise is counter-based and keyed by the GLOBAL sample index (`sample_offset`), so the gathered result equals the
single-GPU result for the same seed regardless of the world size.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from .unet import check_negative_prompt


def shard_bounds(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, balanced split of `total` samples: the first (total % world) ranks get one extra."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_negative(lo: int, hi: int, total: int, negative_text_embeds: Optional[torch.Tensor], negative_text_masks: Optional[torch.Tensor]) -> dict:
    """The negative-prompt keywords of the shard [lo, hi) of `total` samples: a per-sample negative prompt is sliced with its rows, a
    batch-1 one (it serves every sample) goes to every rank as it is."""
    check_negative_prompt(negative_text_embeds, negative_text_masks, total, None)
    if negative_text_embeds is None:
        return {}
    cut = (lambda t: t) if negative_text_embeds.shape[0] == 1 else (lambda t: t[lo:hi])
    return dict(negative_text_embeds=cut(negative_text_embeds), negative_text_masks=None if negative_text_masks is None else cut(negative_text_masks))


def shard_compose(lo: int, hi: int, total: int, compose=None, compose_mask=None) -> dict:
    """The composed-prompt keywords (Imagen.sample(compose=, compose_mask=)) of the shard [lo, hi) of `total` samples: whatever has one row per
    sample — embeddings and text masks of batch `total`, [total] weights, [total, H, W] masks — is sliced with its rows; batch-1 prompts and
    masks, [H, W] masks, floats, per-unet tuples and `texts` of one string go to every rank as they are (per-sample `texts` are sliced)."""
    out = {}
    rows = lambda t, nd: t[lo:hi] if isinstance(t, torch.Tensor) and t.ndim == nd and t.shape[0] == total and total != 1 else t
    if compose_mask is not None:
        out['compose_mask'] = rows(compose_mask, 3)
    if compose is not None:
        if not isinstance(compose, (list, tuple)) or not all(isinstance(e, dict) for e in compose):
            return dict(out, compose=compose)            # malformed: `sample_fn` refuses it in its own words
        entries = []
        for e in compose:
            e = dict(e)
            for k, nd in (('text_embeds', 3), ('text_masks', 2), ('weight', 1), ('mask', 3)):
                if k in e:
                    e[k] = rows(e[k], nd)
            if isinstance(e.get('texts'), (list, tuple)) and len(e['texts']) == total and total != 1:
                e['texts'] = list(e['texts'][lo:hi])
            entries.append(e)
        out['compose'] = entries
    return out


def sample_sharded(sample_fn: Callable[..., torch.Tensor], text_embeds: torch.Tensor, *, text_masks: Optional[torch.Tensor] = None,
                   negative_text_embeds: Optional[torch.Tensor] = None, negative_text_masks: Optional[torch.Tensor] = None,
                   negative_texts=None, compose=None, compose_mask=None, group=None, gather: bool = True, **kwargs) -> torch.Tensor:
    """Run `sample_fn(text_embeds=shard, text_masks=shard, sample_offset=lo, **kwargs)` on this rank's shard and all-gather.

    `sample_fn` is normally `Imagen.sample`; it must return a (b_local, C, H, W) tensor on the rank's device.
    Returns the full (B, C, H, W) batch on every rank (or the local shard if gather=False).
    A negative prompt (negative_text_embeds / negative_text_masks, or negative_texts: one string for all samples or one per sample) is
    sharded with its rows.  Every other keyword reaches `sample_fn` as given — the solver keywords `sampler=`, `sample_steps=`, `eta=`
    among them: a stochastic solver's draws are keyed by the global sample index (`sample_offset`), as the ancestral sampler's are; and the
    guidance keywords (`guidance_schedule=`, `guidance_interval=`, `guidance_rescale=`, `guidance_apg=`): rescale and projected guidance take
    their statistics per sample, so a shard's rows are guided as in the whole batch.  Composed prompts (`compose=`, `compose_mask=`) are
    sharded by `shard_compose`: per-sample entries, weights and masks are sliced with the prompts.
    """
    B = text_embeds.shape[0]
    if negative_texts is not None:
        if negative_text_embeds is not None:
            raise ValueError('negative_texts and negative_text_embeds are both given: pass one of them')
        if len(negative_texts) not in (1, B):
            raise ValueError(f"negative_texts: {len(negative_texts)} strings, neither 1 nor the prompts' {B}")
    neg_of = lambda lo, hi: (shard_negative(lo, hi, B, negative_text_embeds, negative_text_masks) if negative_texts is None else
                             dict(negative_texts=list(negative_texts) if len(negative_texts) == 1 else list(negative_texts[lo:hi])))
    neg = lambda lo, hi: {**neg_of(lo, hi), **shard_compose(lo, hi, B, compose, compose_mask)}
    if not dist.is_available() or not dist.is_initialized():
        return sample_fn(text_embeds=text_embeds, text_masks=text_masks, sample_offset=0, **neg(0, B), **kwargs)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    lo, hi = shard_bounds(B, rank, world)
    local = None
    if hi > lo:
        local = sample_fn(text_embeds=text_embeds[lo:hi], text_masks=None if text_masks is None else text_masks[lo:hi],
                          sample_offset=lo, **neg(lo, hi), **kwargs)
    if not gather:
        return local
    return all_gather_images(local, B, group=group)


def all_gather_images(local: Optional[torch.Tensor], total: int, *, group=None) -> torch.Tensor:
    """One all-gather of the final images.  Equal shards use all_gather_into_tensor (a single ring collective over
    xGMI); ragged shards are padded to the largest shard first (the payload is ~0.8 MB/image, bandwidth is irrelevant)."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    sizes = [shard_bounds(total, r, world)[1] - shard_bounds(total, r, world)[0] for r in range(world)]
    if local is not None and all(s == sizes[0] for s in sizes):
        # the common case (B divisible by the world size): exactly one collective, no metadata exchange
        out = torch.empty((total, *local.shape[1:]), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out
    shapes = [None]
    if local is not None:
        shapes = [tuple(local.shape[1:]), str(local.dtype), str(local.device)]
    # every rank needs the image shape (ranks with an empty shard learn it from rank 0, which always has the first shard)
    obj = [shapes if rank == 0 else None]
    dist.broadcast_object_list(obj, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    img_shape = obj[0][0]
    dtype = local.dtype if local is not None else torch.float32
    device = local.device if local is not None else (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    mx = max(sizes)
    if all(s == mx for s in sizes):
        out = torch.empty((total, *img_shape), dtype=dtype, device=device)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out
    padded = torch.zeros((mx, *img_shape), dtype=dtype, device=device)
    if local is not None:
        padded[: local.shape[0]] = local
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded, group=group)
    return torch.cat([p[:s] for p, s in zip(parts, sizes)], dim=0)
