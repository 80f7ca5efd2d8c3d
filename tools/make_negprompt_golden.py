#!/usr/bin/env python
"""tests/golden/negprompt_*: recorded runs of the LIVE REFERENCE with a second text prompt on the null branch of classifier-free guidance,
every Gaussian draw recorded, and the launch lists of the fixture stages.

    python tools/make_negprompt_golden.py --launch-list   # only negprompt_parent_launch_list_abi<N>.json, from THIS tree: run it on the
                                                          # commit BEFORE a change whose no-regression it is to witness
    python tools/make_negprompt_golden.py                 # the recordings; needs the reference's tree (oracle/ref_shim.py); CPU only

  negprompt_unet_sr.pt   weights of the low-res-conditioned second stage (dim 16, dim_mults (1, 2)); stage 1 is the flag-off `twin` of
                         linxattn_unet.pt, the video unet the first stage of sample_tiny_video.pt: both stored there
  negprompt_forward.pt   (a) stage 1 at 16^2, batch 2: prompt of 5 tokens, negative of 7, as a batch-2 and as a batch-1 negative;
                         (b) prompt of 7 tokens, negative of 3; and the ordinary pair (null branch = cond_drop_prob 1) of each prompt
  negprompt_runs.pt      (c) Imagen.sample 16 -> 32, 4 steps, cond_scale 3; (d) ElucidatedImagen.sample, 4 Karras steps; (e) a video DDPM run
                         of 4 frames; (f) each once more without the negative prompt, from the same draws

The reference has no negative prompt.  Its guided evaluation is `null + (cond - null) * cond_scale` with null = forward(cond_drop_prob = 1)
(ip.py:1510-1522, iv.py:1636-1648); the recordings are made with `forward_with_cond_scale` of the reference's unets replaced, at run time and
in this process only, by the same combination of two calls of the reference's own `forward`, the second with the negative prompt and
cond_drop_prob = 0.  Only tensors and constructor kwargs are stored.

Every run with the negative prompt must lie at least DISCRIMINATION times its test's bar from its twin without one, so that no test passes
by ignoring the negative prompt: asserted here, stored, re-asserted by tests/test_negative_prompt_cpu.py from the stored tensors."""
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import fixtures_negprompt as npf  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DISCRIMINATION = 10.0
# the bars of the replay tests for runs of the same kind without a negative prompt (tests/test_sample_cpu_replay.py: the DDPM cascade and
# the video DDPM replays 2e-2, ::test_elucidated_sample_driver 3e-2); forward: the 1e-2 every tiny-unet forward test of the suite uses stands
# in for the tests' bar, which is 1.5 x what the ordinary pair measures in the same run and lies below it
BAR = {"forward": 1e-2, "ddpm": 2e-2, "edm": 3e-2, "video": 2e-2}
COND_SCALE = 3.0


def make_launch_list():
    from imagen_pytorch_amd import _abi, engine, engine3d

    engine.UnetEngine = functools.partial(engine.UnetEngine, dry=True)
    engine3d.UnetEngine3D = functools.partial(engine3d.UnetEngine3D, dry=True)
    path = os.path.join(GOLDEN, f"negprompt_parent_launch_list_abi{_abi.ENUMS['IMAGEN_ABI_VERSION']}.json")
    with open(path, "w") as fh:
        json.dump(npf.launch_lists(), fh, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


class negative_prompt:
    """The reference unets of `model` guided against the prompt (neg, neg_mask) instead of their learned null conditioning: the reference's
    forward_with_cond_scale with its second forward given a prompt (a batch-1 prompt is repeated over the batch)."""

    def __init__(self, model, neg, neg_mask):
        self.unets, self.neg, self.mask = list(model.unets), neg, neg_mask

    def __enter__(self):
        for u in self.unets:
            def guided(*args, cond_scale=1., _u=u, **kwargs):
                kwargs.pop("cond_drop_prob", None)
                b = args[0].shape[0]
                pos = _u.forward(*args, **kwargs, cond_drop_prob=0.)
                if cond_scale == 1:
                    return pos
                rep = lambda t: t.expand(b, *t.shape[1:]) if t.shape[0] == 1 else t
                neg = _u.forward(*args, **{**kwargs, "text_embeds": rep(self.neg), "text_mask": rep(self.mask)}, cond_drop_prob=0.)
                return neg + (pos - neg) * cond_scale
            u.forward_with_cond_scale = guided

    def __exit__(self, *exc):
        for u in self.unets:
            del u.forward_with_cond_scale


def mask_of(te):
    return torch.any(te != 0., dim=-1)


def make_forward(ip, base):
    g = torch.Generator().manual_seed(211)
    B, S = 2, 16
    x = torch.randn(B, 3, S, S, generator=g)
    time = torch.tensor([0.6, -1.9])
    cases = {}
    for tag, n_pos, n_neg in (("a", 5, 7), ("b", 7, 3)):
        te = torch.randn(B, n_pos, 32, generator=g)
        tm = torch.ones(B, n_pos, dtype=torch.bool)
        tm[1, n_pos - 2:] = False
        neg = torch.randn(B, n_neg, 32, generator=g)
        nm = torch.ones(B, n_neg, dtype=torch.bool)
        nm[0, n_neg - 1:] = False
        with torch.no_grad():
            rec = dict(text_embeds=te, text_mask=tm, negative_text_embeds=neg, negative_text_mask=nm,
                       out_cond=base(x, time, text_embeds=te, text_mask=tm), out_null=base(x, time, text_embeds=te, text_mask=tm, cond_drop_prob=1.),
                       out_neg=base(x, time, text_embeds=neg, text_mask=nm),
                       out_neg_b1=base(x, time, text_embeds=neg[:1].expand(B, -1, -1), text_mask=nm[:1].expand(B, -1)))
            rec["out_cfg"] = base.forward_with_cond_scale(x, time, text_embeds=te, text_mask=tm, cond_scale=COND_SCALE)
        for k in ("out_neg", "out_neg_b1"):
            gap = npf.nerr(rec["out_null"], rec[k])
            print(f"forward ({tag}) {k}: |learned null - negative| / |negative| = {gap:.3f}")
            assert gap >= DISCRIMINATION * BAR["forward"], (tag, k, gap)
        cases[tag] = rec
    path = os.path.join(GOLDEN, "negprompt_forward.pt")
    torch.save(dict(x=x, time=time, cases=cases, cond_scale=COND_SCALE, weights_from=("linxattn_unet.pt", "twin"), forward_bar_stand_in=BAR["forward"],
                    discrimination=DISCRIMINATION, generator="tools/make_negprompt_golden.py",
                    reference="lucidrains/imagen-pytorch v2.0.0 Unet.forward (imagen_pytorch.py:1524-1725), once per prompt"), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


def record_pair(model, call, neg, neg_mask, seed, bar, what):
    """call() twice from the same seed — guided against the negative prompt, and as the reference stands: the same draws, and outputs
    further apart than DISCRIMINATION * bar at every stage."""
    from oracle.make_golden import _record_draws

    torch.manual_seed(seed)
    with negative_prompt(model, neg, neg_mask):
        outs, draws = _record_draws(call)
    torch.manual_seed(seed)
    outs_plain, draws_plain = _record_draws(call)
    assert len(draws) == len(draws_plain) and all(torch.equal(a, b) for a, b in zip(draws, draws_plain))
    gaps = [npf.nerr(a, b) for a, b in zip(outs_plain, outs)]
    print(f"{what}: outputs {[tuple(o.shape) for o in outs]}, {len(draws)} draws, |without negative - with| / |with| = {['%.3f' % v for v in gaps]}")
    assert min(gaps) >= DISCRIMINATION * bar, (what, gaps, DISCRIMINATION * bar)
    return [o.clone() for o in outs], [o.clone() for o in outs_plain], draws


def ddpm_tags(draws, steps, stages):
    noise, it = {}, iter(draws)
    for stage in range(stages):
        if stage > 0:
            noise[("lowres", stage)] = next(it)
        noise[("init", stage)] = next(it)
        for i in range(steps):
            noise[("step", stage, i)] = next(it)
    assert next(it, None) is None
    return noise


def make_runs(ip, iv, el, base):
    from make_selfcond_golden import edm_tags, pack_unet, round_to_half
    from oracle.make_golden import _derandomise, derandomise_unet3d  # noqa: F401

    torch.manual_seed(223)
    kw_sr = {k: v for k, v in npf.KW_SR.items() if k != "lowres_cond"}
    sr = ip.Unet(**kw_sr, lowres_cond=True).eval()
    _derandomise(sr)
    round_to_half(sr)
    path = os.path.join(GOLDEN, "negprompt_unet_sr.pt")
    torch.save(pack_unet(sr, dict(npf.KW_SR)), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)

    g = torch.Generator().manual_seed(227)
    te = torch.randn(2, 9, 32, generator=g)
    neg = torch.randn(1, 6, 32, generator=g)           # one negative prompt for the whole batch, shorter than the prompts
    neg_b = torch.randn(2, 11, 32, generator=g)        # one per sample, longer than the prompts (the video run)
    common = dict(text_embeds=te, cond_scale=COND_SCALE, use_tqdm=False, return_all_unet_outputs=True)
    runs = {}

    def cascade(klass, **kw):
        model = klass((ip.Unet(**npf.base_kwargs()), ip.Unet(**kw_sr)), image_sizes=npf.IMAGE_SIZES, text_embed_dim=32, cond_drop_prob=0.1, **kw).eval()
        model.unets[0].load_state_dict(base.state_dict())
        model.unets[1].load_state_dict(sr.state_dict())
        return model

    model = cascade(ip.Imagen, timesteps=npf.T)
    outs, plain, draws = record_pair(model, lambda: model.sample(**common), neg, mask_of(neg), 229, BAR["ddpm"], "image DDPM")
    runs["ddpm"] = dict(noise=ddpm_tags(draws, npf.T, 2), outputs=outs, outputs_without_negative=plain, negative_text_embeds=neg, bar=BAR["ddpm"])
    model = cascade(el.ElucidatedImagen, **npf.runs_hparams())
    outs, plain, draws = record_pair(model, lambda: model.sample(**common), neg, mask_of(neg), 233, BAR["edm"], "image Karras")
    runs["edm"] = dict(noise=edm_tags(draws, npf.T, 2), outputs=outs, outputs_without_negative=plain, negative_text_embeds=neg, bar=BAR["edm"])

    spec = torch.load(os.path.join(GOLDEN, "sample_tiny_video.pt"), weights_only=False)["unets"][0]
    model = ip.Imagen((iv.Unet3D(**{k: v for k, v in spec["kwargs"].items() if k != "lowres_cond"}),), image_sizes=(npf.VIDEO_SIZE,), timesteps=npf.T,
                      text_embed_dim=32, cond_drop_prob=0.1).eval()
    model.unets[0].load_state_dict(spec["state_dict"])
    vcommon = dict(common, video_frames=npf.VIDEO_FRAMES)
    outs, plain, draws = record_pair(model, lambda: model.sample(**vcommon), neg_b, mask_of(neg_b), 239, BAR["video"], "video DDPM")
    runs["video"] = dict(noise=ddpm_tags(draws, npf.T, 1), outputs=outs, outputs_without_negative=plain, negative_text_embeds=neg_b, bar=BAR["video"])

    path = os.path.join(GOLDEN, "negprompt_runs.pt")
    torch.save(dict(text_embeds=te, cond_scale=COND_SCALE, image_sizes=npf.IMAGE_SIZES, timesteps=npf.T, hparams=npf.runs_hparams(),
                    frames=npf.VIDEO_FRAMES, video_size=npf.VIDEO_SIZE, runs=runs, discrimination=DISCRIMINATION,
                    weights_from=dict(stage1=("linxattn_unet.pt", "twin"), stage2="negprompt_unet_sr.pt", video=("sample_tiny_video.pt", 0)),
                    generator="tools/make_negprompt_golden.py",
                    reference="lucidrains/imagen-pytorch v2.0.0 Imagen.sample / ElucidatedImagen.sample, image and video stages, the unets' "
                              "forward_with_cond_scale combining two calls of their own forward"), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


def main():
    from oracle.ref_shim import load_reference

    ip, iv, el = load_reference("imagen_pytorch"), load_reference("imagen_video"), load_reference("elucidated_imagen")
    import fixtures_linxattn as lx

    rec, sd = lx.unet_record("twin")
    base = ip.Unet(**rec["kwargs"]).eval()
    base.load_state_dict(sd)
    make_forward(ip, base)
    make_runs(ip, iv, el, base)


if __name__ == "__main__":
    if "--launch-list" in sys.argv[1:]:
        make_launch_list()
    else:
        main()
