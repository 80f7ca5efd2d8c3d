#!/usr/bin/env python
"""tests/golden/selfcond_*.pt: recorded runs of the LIVE REFERENCE on self-conditioning unets (Unet(self_cond=True) under the Karras et al.
sampler, Unet3D(self_cond=True) as a denoiser and under both samplers), every Gaussian draw recorded.

    python tools/make_selfcond_golden.py        # needs the reference's tree (oracle/ref_shim.py); CPU only

  selfcond_image_unet{0,1}.pt  weights of a tiny self-conditioning image cascade (16^2 -> 32^2), one file per stage
  selfcond_image_runs.pt       (b) ElucidatedImagen.sample on it: 4 Karras steps, CFG 3 — plain, skip_steps = 1, inpainting with
                               inpaint_resample_times = 2 — and the plain run once more with `self_cond` forced to None
  selfcond_video_unet.pt       weights of one tiny Unet3D(self_cond=True)
  selfcond_video.pt            that unet at 16^2, 4 frames: (a) its forward with and without a self-conditioning
                               clip, (c) Imagen.sample (3 steps) and ElucidatedImagen.sample (3 steps) over it, each also with `self_cond`
                               forced to None

Only tensors and constructor kwargs are stored.  The weights are rounded to fp16 BEFORE the reference runs and stored as ONE flat fp16 tensor
per unet plus the ordered (key, shape) index (tools/make_video_headdim32_fixture.py): unpack_state_dict() restores them.

A fresh unet's init conv gives the self-conditioning channels the same small weights as every other input, and the recorded outputs would
hardly depend on them: `derandomise_self_cond` scales those columns up until the run with `self_cond` forced to None differs from the real
one by at least DISCRIMINATION times the bar of the tests that compare with these fixtures — asserted here for every run, re-asserted by
tests/test_selfcond_cpu.py::test_fixtures_tell_self_conditioning_from_its_absence from the stored tensors."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from oracle.make_golden import ELUCIDATED_HP, TINY_3D, TINY_BASE, TINY_SR, _derandomise, _record_draws, derandomise_unet3d  # noqa: E402
from oracle.ref_shim import load_reference  # noqa: E402
from fixtures_common import nerr, unpack_state_dict  # noqa: E402  (the fixtures' reader: written and read back by one function)

GOLDEN = os.path.join(ROOT, "tests", "golden")
DISCRIMINATION = 10.0
# the bars of the tests that compare with each run (tests/test_sample_cpu_replay.py, tests/test_model_gpu.py, tests/test_video_gpu.py)
BAR = {"image_edm": 3e-2, "video_forward": 1e-2, "video_ddpm": 2e-2, "video_edm": 5e-2}
SELF_COND_GAIN = 64.0
HP = dict(ELUCIDATED_HP, num_sample_steps=4)
HP_VIDEO = dict(ELUCIDATED_HP, num_sample_steps=3)
T_VIDEO = 3


def pack_unet(u, kwargs):
    sd = u.state_dict()
    assert all(v.is_floating_point() for v in sd.values())
    spec = dict(kwargs=kwargs, flat=torch.cat([v.reshape(-1).half() for v in sd.values()]), index=[(k, tuple(v.shape)) for k, v in sd.items()])
    back = unpack_state_dict(spec)
    assert list(back) == list(sd) and all(torch.equal(back[k], v) for k, v in sd.items())
    return spec


def derandomise_self_cond(unet, channels=3, gain=SELF_COND_GAIN):
    """The init conv's input channels are [x | self_cond | low-res] (no conditioning image here): scale the self_cond columns."""
    for name, prm in unet.named_parameters():
        if name.startswith("init_conv.") and name.endswith("weight"):
            prm.data[:, channels:2 * channels] *= gain


def round_to_half(unet):
    for prm in unet.parameters():
        prm.data.copy_(prm.data.half().float())
    for buf in unet.buffers():
        if buf.is_floating_point():
            buf.data.copy_(buf.data.half().float())


class no_self_cond:
    """The unets of `model` called with self_cond = None whatever the sampler passes."""

    def __init__(self, model):
        self.unets = list(model.unets)

    def __enter__(self):
        for u in self.unets:
            real = u.forward
            u.forward = lambda *a, _real=real, **k: _real(*a, **{**k, "self_cond": None})

    def __exit__(self, *exc):
        for u in self.unets:
            del u.forward


def edm_tags(draws, T, stages, first=0, R=0):
    noise, it = {}, iter(draws)
    for stage in range(stages):
        if stage > 0:
            noise[("lowres", stage)] = next(it)
        noise[("init", stage)] = next(it)
        for i in range(first, T):
            if not R:
                noise[("step", stage, i)] = next(it)
                continue
            for r in reversed(range(R)):
                noise[("step", stage, i, r)] = next(it)
                if r > 0 and i < T - 1:
                    noise[("renoise", stage, i, r)] = next(it)
    assert next(it, None) is None
    return noise


def record_pair(model, call, seed, bar, what):
    """call() twice from the same seed — as is, and with self_cond forced to None: same draws, and outputs further apart than
    DISCRIMINATION * bar at every stage."""
    torch.manual_seed(seed)
    outs, draws = _record_draws(call)
    torch.manual_seed(seed)
    with no_self_cond(model):
        outs_none, draws_none = _record_draws(call)
    assert len(draws) == len(draws_none) and all(torch.equal(a, b) for a, b in zip(draws, draws_none))
    gaps = [nerr(a, b) for a, b in zip(outs_none, outs)]
    print(f"{what}: outputs {[tuple(o.shape) for o in outs]}, {len(draws)} draws, |without self_cond - with| / |with| = {['%.3f' % g for g in gaps]}")
    assert min(gaps) >= DISCRIMINATION * bar, (what, gaps, DISCRIMINATION * bar)
    return [o.clone() for o in outs], [o.clone() for o in outs_none], draws


def make_image(ip, el, seed=43):
    torch.manual_seed(seed)
    kw = [dict(TINY_BASE, self_cond=True), dict({k: v for k, v in TINY_SR.items() if k != "lowres_cond"}, self_cond=True)]
    model = el.ElucidatedImagen((ip.Unet(**kw[0]), ip.Unet(**kw[1])), image_sizes=(16, 32), text_embed_dim=32, cond_drop_prob=0.1, **HP).eval()
    for u in model.unets:
        _derandomise(u)
        derandomise_self_cond(u)
        round_to_half(u)
    for i, u in enumerate(model.unets):
        path = os.path.join(GOLDEN, f"selfcond_image_unet{i}.pt")
        torch.save(pack_unet(u, {**kw[i], "lowres_cond": i > 0}), path)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    text_embeds = torch.randn(2, 9, 32)
    g = torch.Generator().manual_seed(47)
    inpaint_images = torch.rand(2, 3, 32, 32, generator=g)
    inpaint_masks = torch.rand(2, 32, 32, generator=g) > 0.5
    inpaint_masks[:, 8:20, 4:24] = True
    common = dict(text_embeds=text_embeds, cond_scale=3., use_tqdm=False, return_all_unet_outputs=True)
    T = HP["num_sample_steps"]
    runs = {}
    for tag, kwargs, tags in (("plain", {}, dict()), ("skip", dict(skip_steps=1), dict(first=1)),
                              ("inpaint", dict(inpaint_images=inpaint_images, inpaint_masks=inpaint_masks, inpaint_resample_times=2), dict(R=2))):
        outs, outs_none, draws = record_pair(model, lambda: model.sample(**common, **kwargs), 53, BAR["image_edm"], f"image EDM [{tag}]")
        runs[tag] = dict(kwargs=kwargs, noise=edm_tags(draws, T, 2, **tags), outputs=outs, outputs_without_self_cond=outs_none)
    path = os.path.join(GOLDEN, "selfcond_image_runs.pt")
    torch.save(dict(weights_from=["selfcond_image_unet0.pt", "selfcond_image_unet1.pt"], image_sizes=(16, 32), hparams=dict(HP), cond_scale=3.,
                    text_embeds=text_embeds, runs=runs, bar=BAR["image_edm"], discrimination=DISCRIMINATION,
                    generator="tools/make_selfcond_golden.py",
                    reference="lucidrains/imagen-pytorch v2.0.0 ElucidatedImagen.sample over Unet(self_cond=True) stages "
                              "(elucidated_imagen.py:393-545)"), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def make_video(ip, iv, el, seed=59, frames=4, S=16):
    torch.manual_seed(seed)
    kw = dict(TINY_3D, self_cond=True)
    imagen = ip.Imagen((iv.Unet3D(**kw),), image_sizes=(S,), timesteps=T_VIDEO, text_embed_dim=32, cond_drop_prob=0.1).eval()
    unet = imagen.unets[0]
    derandomise_unet3d(unet)
    derandomise_self_cond(unet)
    round_to_half(unet)
    # (a) the denoiser alone
    B = 2
    x = torch.randn(B, 3, frames, S, S)
    clip = torch.randn(B, 3, frames, S, S).clamp(-1., 1.)
    time = torch.tensor([0.7, -2.3])
    text_embeds = torch.randn(B, 11, 32)
    text_mask = torch.ones(B, 11, dtype=torch.bool)
    text_mask[1, 7:] = False
    with torch.no_grad():
        tk = dict(text_embeds=text_embeds, text_mask=text_mask)
        fwd = dict(x=x, time=time, self_cond=clip, **tk,
                   out_cond=unet(x, time, self_cond=clip, **tk), out_null=unet(x, time, self_cond=clip, cond_drop_prob=1., **tk),
                   out_cfg=unet.forward_with_cond_scale(x, time, self_cond=clip, cond_scale=3., **tk),
                   out_cond_no_clip=unet(x, time, **tk), out_cfg_no_clip=unet.forward_with_cond_scale(x, time, cond_scale=3., **tk))
    gap = min(nerr(fwd["out_cond_no_clip"], fwd["out_cond"]), nerr(fwd["out_cfg_no_clip"], fwd["out_cfg"]))
    print(f"video forward: |without clip - with| / |with| = {gap:.3f}")
    assert gap >= DISCRIMINATION * BAR["video_forward"], gap
    # (c) both samplers
    te = torch.randn(2, 9, 32)
    common = dict(text_embeds=te, video_frames=frames, cond_scale=3., use_tqdm=False, return_all_unet_outputs=True)
    outs, outs_none, draws = record_pair(imagen, lambda: imagen.sample(**common), 61, BAR["video_ddpm"], "video DDPM")
    noise, it = {("init", 0): draws[0]}, iter(draws[1:])
    for i in range(T_VIDEO):
        noise[("step", 0, i)] = next(it)
    assert next(it, None) is None
    ddpm = dict(timesteps=T_VIDEO, noise=noise, outputs=outs, outputs_without_self_cond=outs_none, bar=BAR["video_ddpm"])
    edm_model = el.ElucidatedImagen((unet,), image_sizes=(S,), text_embed_dim=32, cond_drop_prob=0.1, **HP_VIDEO).eval()
    assert edm_model.unets[0].self_cond
    edm_model.unets[0].load_state_dict(unet.state_dict())          # (cast_model_parameters may have re-instantiated the unet)
    outs, outs_none, draws = record_pair(edm_model, lambda: edm_model.sample(**common), 67, BAR["video_edm"], "video EDM")
    edm = dict(hparams=dict(HP_VIDEO), noise=edm_tags(draws, HP_VIDEO["num_sample_steps"], 1), outputs=outs, outputs_without_self_cond=outs_none,
               bar=BAR["video_edm"])
    path = os.path.join(GOLDEN, "selfcond_video_unet.pt")
    torch.save(pack_unet(unet, {**kw, "lowres_cond": False}), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    path = os.path.join(GOLDEN, "selfcond_video.pt")
    torch.save(dict(weights_from="selfcond_video_unet.pt", image_sizes=(S,), frames=frames, cond_scale=3., text_embeds=te,
                    forward=fwd, forward_bar=BAR["video_forward"], ddpm=ddpm, edm=edm, discrimination=DISCRIMINATION,
                    generator="tools/make_selfcond_golden.py",
                    reference="lucidrains/imagen-pytorch v2.0.0 Unet3D(self_cond=True).forward (imagen_video.py:1650-1941), Imagen.sample and "
                              "ElucidatedImagen.sample over it"), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    ip, iv, el = load_reference("imagen_pytorch"), load_reference("imagen_video"), load_reference("elucidated_imagen")
    make_image(ip, el)
    make_video(ip, iv, el)
