"""What the sampling front end refuses, as data: a fixed list of malformed and out-of-scope calls through `sample`, `sample_requests`,
`sample_pipelined` and `prepare_conditioning` of `Imagen` and `ElucidatedImagen` — at least one per `raise` and per `assert` with a message of
the keyword layer — and per call the exception type with its full message.  Run by `tools/sampler_digests.py --mode refusals`, on the CPU.

Nothing is built or launched: `Plan.run` raises (NoLaunch), and `_sample` is replaced by its resolve part, after which a call that was NOT refused
is recorded as "accepted".  After every refused call `_stages` is empty and the seed sequence (`_next_seed`) stands where it stood.  The calls pass
`seed=` so that this holds wherever the refusal comes from; the cases named `*.noseed` leave it out: they are the checks that have to come before
any seed is drawn (the pre-flight of `sample` and of `sample_requests`).
"""
from __future__ import annotations

import torch

SEED = 20240229


class NoLaunch:
    """The interpreter of this mode: there is nothing to interpret."""

    def run(self, plan):
        raise AssertionError(f"a refusal case launched {plan.name}")


class Accepted(Exception):
    pass


def _encode_text(texts, return_attn_mask=True):
    """The `encode_text` hook of the models here: 5 tokens per text, drawn from its length."""
    emb = torch.stack([torch.randn(5, 32, generator=torch.Generator().manual_seed(len(t))) for t in texts])
    return emb, torch.ones(len(texts), 5, dtype=torch.bool)


def model(key: str):
    """The fixture cascades of tests/golden, unloaded (nothing runs): 'ddpm' | 'karras' | 'video' | 'karras_video', and the variants 'uncond'
    (condition_on_text=False), 'nodrop' (cond_drop_prob == 0), 'mixed' (unet 2 without a text branch), 'tampered' (condition_on_text set back
    on an unconditional model: the only way to the asserts that repeat `_resolve_text`'s), 'video_bilinear', 'video_tds'."""
    import sampler_snapshot as ss
    from imagen_pytorch_amd import ElucidatedImagen, Imagen, Unet, Unet3D

    video = 'video' in key
    g = ss._load("sample_tiny_video.pt" if video else "sample_tiny_cascade.pt")
    torch.manual_seed(0)
    unets = [(Unet3D if video else Unet)(**spec["kwargs"]).eval() for spec in g["unets"]]
    kw = dict(image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0. if key == 'nodrop' else 0.1,
              condition_on_text=key not in ('uncond', 'tampered'))
    if key == 'video_bilinear':
        kw.update(resize_mode='bilinear')
    if key == 'video_tds':
        kw.update(temporal_downsample_factor=(2, 1))
    m = ElucidatedImagen(unets, num_sample_steps=ss.T, **kw) if 'karras' in key else Imagen(unets, timesteps=ss.T, **kw)
    if key == 'mixed':
        m.unets[1].cond_on_text = False
    if key == 'tampered':
        m.condition_on_text = True
    m.encode_text = _encode_text
    return m.eval()


def cases():
    """[(case name, model key, method, args, keywords)]"""
    import sampler_snapshot as ss
    from imagen_pytorch_amd import Conditioning

    g = ss._load("sample_tiny_cascade.pt")
    te, (s0, s1) = g["text_embeds"], g["image_sizes"]
    B, nan, inf = te.shape[0], float('nan'), float('inf')
    p = te.flip(0) * 0.75
    neg = dict(negative_text_embeds=te.flip(0) * 0.5)
    paint = dict(inpaint_images=torch.zeros(B, 3, s1, s1), inpaint_masks=torch.zeros(B, s1, s1, dtype=torch.bool))
    ramp, merged = [3.0, 2.5, 2.0, 1.5], [(1, 1), (2, 1)]
    handle = Conditioning(te, None, B, te.flip(0) * 0.5, None)
    base = dict(text_embeds=te, cond_scale=3.0, seed=SEED, device='cpu', use_tqdm=False)
    out = []

    def S(name, mkey='ddpm', method='sample', drop=(), **kw):
        """One call of `method` with sample()'s keywords: the guided two-prompt call, `kw` over it, without the keywords of `drop`."""
        full = {**base, **kw}
        out.append((name, mkey, method, (), {k: v for k, v in full.items() if k not in drop}))

    def R(name, requests, mkey='ddpm', **common):
        out.append((name, mkey, 'sample_requests', (requests,), dict(device='cpu', **common)))

    def P(name, batches, mkey='ddpm', **common):
        out.append((name, mkey, 'sample_pipelined', ([dict(seed=SEED + i, **b) for i, b in enumerate(batches)],), dict(device='cpu', **common)))

    C = lambda name, entry, mkey='ddpm', **kw: S(name, mkey, compose=[entry] if isinstance(entry, dict) else entry, **kw)
    nt = ('text_embeds',)

    # ---- the pre-flight: what needs no batch, device or text
    S('solver.steps_with_ddpm', sample_steps=3)
    S('solver.eta_with_ddpm', eta=0.5)
    S('solver.unknown', sampler='euler')
    S('solver.unknown.noseed', sampler='euler', drop=('seed',))
    S('solver.eta_range', sampler='ddim', eta=1.5)
    S('solver.dpmpp_eta', sampler='dpmpp_2m', eta=0.5)
    S('solver.steps_len', sampler='ddim', sample_steps=(3, 3, 3))
    S('solver.too_few', sampler='dpmpp_2m', sample_steps=1)
    S('solver.inpaint', sampler='ddim', sample_steps=3, **paint)
    S('solver.merged_eta', sampler='ddim', sample_steps=3, eta=0.5, seed=merged)
    S('guidance.schedule_number', guidance_schedule=3.0)
    S('guidance.schedule_len', guidance_schedule=(None, None, None))
    S('guidance.schedule_entry', guidance_schedule=('abc', None))
    S('guidance.schedule_entries', guidance_schedule=[3.0] * 5)
    S('guidance.schedule_bools', guidance_schedule=[True, 2.0, 2.0, 2.0])        # (accepted: this predicate takes a bool for a number)
    S('guidance.interval_order', guidance_interval=(0.8, 0.3))
    S('guidance.interval_len', guidance_interval=(None, None, None))
    S('guidance.interval_len.noseed', guidance_interval=(None, None, None), drop=('seed',))
    S('guidance.nodrop', 'nodrop', guidance_schedule=ramp)
    S('guidance.nodrop.interval', 'nodrop', guidance_interval=(0.3, 0.8))
    S('guidance.uncond', 'uncond', guidance_schedule=ramp, batch_size=B, drop=nt)
    S('guidance.inpaint', guidance_interval=(0.3, 0.8), **paint)
    S('guidance.no_text_branch', 'mixed', guidance_schedule=ramp)
    S('guide.rescale_type', guidance_rescale='x')
    S('guide.rescale_bool', guidance_rescale=True)                                # (refused: this predicate does not)
    S('guide.rescale_len', guidance_rescale=(0.5, 0.5, 0.5))
    S('guide.apg_type', guidance_apg=3)
    S('guide.rescale_nan', guidance_rescale=(nan, None))
    S('guide.rescale_entry_bool', guidance_rescale=(True, None))
    S('guide.both', guidance_rescale=0.5, guidance_apg={})
    S('guide.rescale_range', guidance_rescale=1.5)
    S('guide.rescale_range.noseed', guidance_rescale=1.5, drop=('seed',))
    S('guide.apg_keys', guidance_apg=dict(foo=1.0))
    S('guide.apg_entry', guidance_apg=(3, None))
    S('guide.apg_eta', guidance_apg=dict(eta='x'))
    S('guide.apg_threshold_inf', guidance_apg=dict(norm_threshold=inf))
    S('guide.nodrop', 'nodrop', guidance_rescale=0.5)
    S('guide.nodrop.apg', 'nodrop', guidance_apg={})
    S('guide.uncond', 'uncond', guidance_rescale=0.5, batch_size=B, drop=nt)
    S('guide.inpaint', guidance_rescale=0.5, **paint)
    S('guide.no_text_branch', 'mixed', guidance_rescale=0.5)
    S('guide.unguided', guidance_rescale=0.5, cond_scale=1.0)
    S('guide.unguided_stage', guidance_rescale=(None, 0.5), cond_scale=(3.0, 1.0))
    S('guide.guided_by_schedule', guidance_rescale=0.5, cond_scale=1.0, guidance_schedule=ramp)       # (accepted)
    S('karras.sampler', 'karras', sampler='ddim')
    S('karras.sampler.noseed', 'karras', sampler='ddim', drop=('seed',))
    S('karras.steps_eta', 'karras', sample_steps=3, eta=0.0)
    S('karras.schedule_interval', 'karras', guidance_schedule=ramp, guidance_interval=(0.3, 0.8))
    S('karras.rescale', 'karras', guidance_rescale=0.5)
    S('karras.apg', 'karras', guidance_apg={})
    S('karras.compose', 'karras', compose=[dict(text_embeds=p)])
    S('karras.compose_mask', 'karras', compose_mask=torch.ones(s0, s0))
    S('karras.negative_unguided', 'karras', cond_scale=1.0, **neg)
    S('karras.sigmas', 'karras', sigma_min=0.01)                                   # (accepted)
    # ---- composed prompts
    S('compose.mask_alone', compose_mask=torch.ones(s0, s0))
    C('compose.not_list', (dict(text_embeds=p), 3))
    C('compose.empty', [])
    C('compose.too_many', [dict(text_embeds=p)] * 4)
    C('compose.with_schedule', dict(text_embeds=p), guidance_schedule=ramp)
    C('compose.with_rescale_apg', dict(text_embeds=p), guidance_rescale=0.5, guidance_apg={})
    C('compose.inpaint', dict(text_embeds=p), **paint)
    C('compose.conditioning', dict(text_embeds=p), conditioning=Conditioning(te, None, B), drop=nt)
    C('compose.merged', dict(text_embeds=p), seed=merged)
    C('compose.video', dict(text_embeds=p), 'video', video_frames=4)
    C('compose.nodrop', dict(text_embeds=p), 'nodrop')
    C('compose.uncond', dict(text_embeds=p), 'uncond', batch_size=B, drop=nt)
    C('compose.no_text_branch', dict(text_embeds=p), 'mixed')
    C('compose.weight_rows', dict(text_embeds=p, weight=torch.ones(3)))
    C('compose.weight_tuple_len', dict(text_embeds=p, weight=(1.0,)))
    C('compose.weight_type', dict(text_embeds=p, weight='a'))
    C('compose.weight_bool', dict(text_embeds=p, weight=True))
    C('compose.weight_inf', dict(text_embeds=p, weight=inf))
    C('compose.cond_scale_nan', dict(text_embeds=p), cond_scale=nan)
    C('compose.mask_shape', dict(text_embeds=p, mask=torch.ones(3, s0, s0)))
    C('compose.mask_type', dict(text_embeds=p, mask=[[1.0]]))
    C('compose.mask_values', dict(text_embeds=p, mask=torch.full((s0, s0), 2.0)))
    C('compose.own_mask_nan', dict(text_embeds=p), compose_mask=torch.full((s0, s0), nan))
    C('compose.unknown_key', dict(text_embeds=p, scale=2.0))
    C('compose.both_texts', dict(text_embeds=p, texts=['a', 'b']))
    C('compose.no_text', dict(weight=1.0))
    C('compose.empty_text', dict(texts=['a', '']))
    C('compose.embed_dim', dict(text_embeds=torch.zeros(B, 9, 16)))
    C('compose.embed_type', dict(text_embeds=[1.0]))
    C('compose.embed_batch', dict(text_embeds=torch.zeros(3, 9, 32)))
    C('compose.text_masks_shape', dict(text_embeds=p, text_masks=torch.ones(B, 4, dtype=torch.bool)))
    C('compose.ignored', dict(text_embeds=p, weight=0.0), cond_scale=1.0)
    C('compose.ignored_per_unet', dict(text_embeds=p, weight=(0.0, 0.0)), cond_scale=(1.0, 1.0))
    C('compose.texts', dict(texts='one prompt for all', weight=(1.5, -0.5), mask=torch.ones(1, s0, s0)), cond_scale=1.0, **neg)   # (accepted)
    # ---- the negative prompt
    S('negative.handle_and_keyword', conditioning=handle, drop=nt, **neg)
    S('negative.both', negative_texts=['a', 'b'], **neg)
    S('negative.uncond', 'uncond', negative_texts=['a'], batch_size=B, drop=nt)
    S('negative.empty_text', negative_texts=['a', ''])
    S('negative.masks_alone', negative_text_masks=torch.ones(B, 9, dtype=torch.bool))
    S('negative.batch', negative_text_embeds=torch.zeros(3, 9, 32))
    S('negative.embed_dim', negative_text_embeds=torch.zeros(B, 9, 16))
    S('negative.rows_shape', method='resolve', negative_rows=torch.ones(3, dtype=torch.bool), **neg)
    S('negative.nodrop', 'nodrop', cond_scale=1.0, **neg)
    S('negative.unguided', cond_scale=1.0, **neg)
    S('negative.unguided_texts', cond_scale=1.0, negative_texts=['a'])
    S('negative.unguided_handle', cond_scale=1.0, conditioning=handle, drop=nt)
    S('negative.unguided_stage', cond_scale=(3.0, 1.0), stop_at_unet_number=None, start_at_unet_number=2, start_image_or_video=torch.zeros(B, 3, s0, s0), **neg)
    S('negative.constant_schedule_1', guidance_schedule=[1.0] * 4, **neg)
    S('negative.varying_schedule', cond_scale=1.0, guidance_schedule=ramp, **neg)                    # (accepted)
    S('negative.constant_schedule_3', cond_scale=1.0, guidance_schedule=[3.0] * 4, **neg)            # (accepted)
    # ---- text, batch, sizes, the start image
    S('text.empty', texts=['a', ''], drop=nt)
    S('text.missing', drop=nt)
    S('resolve.conditioning_and_text', conditioning=handle)
    S('resolve.device', device='meta')
    S('resolve.video_frames', 'video')
    S('resolve.video_frames_tds', 'video_tds', video_frames=3)
    S('resolve.pil_video', 'video', video_frames=4, return_pil_images=True)
    S('resolve.inpaint_batch', inpaint_images=torch.zeros(3, 3, s1, s1), inpaint_masks=torch.zeros(3, s1, s1, dtype=torch.bool))
    S('resolve.inpaint_text_rows', 'tampered', inpaint_images=torch.zeros(3, 3, s1, s1), inpaint_masks=torch.zeros(3, s1, s1, dtype=torch.bool))
    S('resolve.text_required', 'tampered', drop=nt)
    S('resolve.text_unexpected', 'uncond')
    S('resolve.embed_dim', text_embeds=torch.zeros(B, 9, 16))
    S('resolve.inpaint_pair', inpaint_images=paint['inpaint_images'])
    S('resolve.video_resize', 'video_bilinear', video_frames=4)
    S('resolve.inpaint_video_ndim', 'video', video_frames=4, inpaint_videos=torch.zeros(B, 3, 16, 16), inpaint_masks=torch.zeros(B, 16, 16, dtype=torch.bool))
    S('resolve.start_past_last', start_at_unet_number=3)
    S('resolve.start_image_missing', start_at_unet_number=2)
    S('resolve.start_channels', start_at_unet_number=2, start_image_or_video=torch.zeros(B, 4, s0, s0))
    S('sizes.video', 'video', video_frames=4, image_shapes=((8, 8), (16, 16)))
    S('sizes.len', image_shapes=((16, 16),))
    S('sizes.entry', image_shapes=(16, (32, 32)))
    S('sizes.shrinks', image_shapes=((32, 32), (16, 16)))
    S('sizes.divisible', image_shapes=((15, 16), (32, 32)))
    S('sizes.rectangular', image_shapes=((16, 24), (32, 48)))                                        # (accepted)
    out.append(('spans.rows', 'ddpm', '_seed_spans', (merged, 3), {}))
    # ---- prepare_conditioning
    H = lambda name, mkey='ddpm', **kw: out.append((name, mkey, 'prepare_conditioning', (), kw))
    H('prepare.text_missing')
    H('prepare.text_required', 'tampered')
    H('prepare.text_unexpected', 'uncond', text_embeds=te)
    H('prepare.embed_dim', text_embeds=torch.zeros(B, 9, 16))
    H('prepare.negative_both', text_embeds=te, negative_texts=['a'], **neg)
    H('prepare.negative_batch', text_embeds=te, negative_text_embeds=torch.zeros(3, 9, 32))
    H('prepare.negative_uncond', 'uncond', batch_size=B, **neg)
    H('prepare.karras', 'karras', texts=['a', 'bc'], negative_texts=['d'])                            # (returns a handle)
    # ---- sample_requests: the common keywords go through the pre-flight before any text is encoded or any seed is drawn
    reqs = lambda **kw: [dict(text_embeds=te[:1], **kw), dict(text_embeds=te[1:])]
    seeded = lambda **kw: [dict(text_embeds=te[:1], seed=1, **kw), dict(text_embeds=te[1:], seed=2)]
    R('requests.solver_unknown.noseed', reqs(), cond_scale=3.0, sampler='euler')
    R('requests.schedule_nodrop.noseed', reqs(), 'nodrop', cond_scale=3.0, guidance_schedule=ramp)
    R('requests.rescale_range.noseed', reqs(), cond_scale=3.0, guidance_rescale=1.5)
    R('requests.karras_solver.noseed', reqs(), 'karras', cond_scale=3.0, sampler='ddim')
    R('requests.karras.noseed', reqs(), 'karras', cond_scale=3.0)
    R('requests.compose.noseed', reqs(), cond_scale=3.0, compose=[dict(text_embeds=p)])
    R('requests.compose_inside.noseed', reqs(compose_mask=None), cond_scale=3.0)
    R('requests.schedule_inside.noseed', reqs(guidance_schedule=ramp), cond_scale=3.0)
    R('requests.apg_inside.noseed', reqs(guidance_apg={}), cond_scale=3.0)
    R('requests.eta.noseed', reqs(), cond_scale=3.0, sampler='ddim', sample_steps=3, eta=0.5)
    R('requests.init_images.noseed', reqs(), cond_scale=3.0, init_images=torch.zeros(B, 3, s0, s0))
    R('requests.conditioning_inside.noseed', reqs(conditioning=handle), cond_scale=3.0)
    R('requests.both_negative.noseed', reqs(**{k: v[:1] for k, v in neg.items()}), cond_scale=3.0, negative_texts=['a'])
    R('requests.none', [], cond_scale=3.0)                                                            # (returns [])
    R('requests.extra_key', seeded(cond_scale=2.0), cond_scale=3.0)
    R('requests.text_missing', [dict(seed=1)], cond_scale=3.0)
    R('requests.negative_batch', seeded(negative_text_embeds=torch.zeros(3, 9, 32)), cond_scale=3.0)
    R('requests.negative_unguided', seeded(**{k: v[:1] for k, v in neg.items()}), cond_scale=1.0)
    R('requests.rescale_unguided', seeded(), cond_scale=1.0, guidance_rescale=0.5)
    R('requests.rescale_negative', seeded(**{k: v[:1] for k, v in neg.items()}), cond_scale=3.0, guidance_rescale=0.5)   # (accepted)
    # ---- sample_pipelined: every refusal of the whole cascade comes before a thread starts (the batches carry their seeds)
    one = [dict(text_embeds=te)]
    P('pipelined.drives', one, cond_scale=3.0, stop_at_unet_number=1)
    P('pipelined.solver_unknown', one, cond_scale=3.0, sampler='euler')
    P('pipelined.karras_schedule', one, 'karras', cond_scale=3.0, guidance_schedule=ramp)
    P('pipelined.schedule_inpaint', one, cond_scale=3.0, guidance_schedule=ramp, **paint)
    P('pipelined.schedule_entries', one, cond_scale=3.0, guidance_schedule=[3.0] * 5)
    P('pipelined.rescale_inpaint', one, cond_scale=3.0, guidance_rescale=0.5, **paint)
    P('pipelined.rescale_unguided', one, cond_scale=1.0, guidance_rescale=0.5)
    P('pipelined.rescale_unguided_stage', one, cond_scale=(3.0, 1.0), guidance_rescale=(None, 0.5))
    P('pipelined.rescale_one_stage', one, cond_scale=(3.0, 1.0), guidance_rescale=0.5)                # (accepted: one stage of the cascade is guided)
    P('pipelined.compose_ignored', one, cond_scale=1.0, compose=[dict(text_embeds=p, weight=0.0)])
    P('pipelined.text_missing', [{}], cond_scale=3.0)
    P('pipelined.negative_unguided', one, cond_scale=1.0, **neg)
    P('pipelined.negative_unguided_texts', [dict(texts=['a', 'bc'])], cond_scale=1.0, negative_texts=['d'])
    P('pipelined.negative_handle_and_keyword', [dict(conditioning=handle)], cond_scale=3.0, **neg)
    P('pipelined.negative_unguided_handle', [dict(conditioning=handle)], cond_scale=1.0)
    P('pipelined.negative_nodrop', one, 'nodrop', cond_scale=1.0, **neg)
    P('pipelined.negative_batch', one, cond_scale=3.0, negative_text_embeds=torch.zeros(3, 9, 32))
    P('pipelined.negative_one_stage', one, cond_scale=(3.0, 1.0), **neg)                             # (accepted: one stage has null rows)
    # where the two pre-flights of the parent of "one pre-flight for every entry" disagreed: a negative prompt against the raw cond_scale
    # (sample_pipelined) or against the scales the schedule resolves to, and not at all beside composed prompts (sample)
    P('pipelined.negative_varying_schedule', one, cond_scale=1.0, guidance_schedule=ramp, **neg)
    P('pipelined.negative_constant_schedule_3', one, cond_scale=1.0, guidance_schedule=[3.0] * 4, **neg)
    P('pipelined.negative_constant_schedule_1', one, cond_scale=3.0, guidance_schedule=[1.0] * 4, **neg)
    P('pipelined.negative_compose', one, cond_scale=1.0, compose=[dict(text_embeds=p)], **neg)
    return out


def collect() -> dict:
    from imagen_pytorch_amd import imagen as imagen_mod

    def resolve_only(self, c):
        self._resolve(c)
        raise Accepted()

    saved = imagen_mod.Imagen._sample
    imagen_mod.Imagen._sample = resolve_only
    models, result = {}, {}
    try:
        for name, mkey, method, args, kw in cases():
            m = models.get(mkey) or models.setdefault(mkey, model(mkey))
            fn = {'resolve': lambda **k: m._resolve(m._call(**{x: v for x, v in k.items() if x != 'use_tqdm'})),
                  '_seed_spans': imagen_mod._seed_spans}.get(method) or getattr(m, method)
            drawn = m._call_counter
            try:
                ret = fn(*args, **kw)
                rec = {"returned": type(ret).__name__ if not isinstance(ret, list) else f"list of {len(ret)}"}
            except Accepted:
                rec = {"accepted": True}
            except Exception as e:  # noqa: BLE001 — the record of this tool
                rec = {"raised": type(e).__name__, "message": str(e)}
                assert m._call_counter == drawn, f"{name}: the refused call drew {m._call_counter - drawn} seed(s)"
            assert not m._stages, f"{name}: {len(m._stages)} stage(s) were built"
            result[name] = rec
            print(f"{name}: {rec.get('raised') or next(iter(rec))}", flush=True)
    finally:
        imagen_mod.Imagen._sample = saved
    print(f"{len(result)} calls: {sum('raised' in r for r in result.values())} refused, nothing built or launched")
    return result
