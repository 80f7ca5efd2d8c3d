#!/usr/bin/env python
"""tests/golden/rect_*.pt: recorded runs of the LIVE REFERENCE on rectangular images (H != W), every Gaussian draw recorded.

    python tools/make_rect_golden.py        # needs the reference's tree (oracle/ref_shim.py); CPU only

  rect_forward_<unet>.pt   Unet.forward on the cond and the null branch, batch 2 (four_sr: 1), in BOTH orientations (an H / W swap passes every square test):
                      tiny, memeff, comb, linx   (two levels)               16x24, 24x16, 32x48
                      four      (four levels, divisor 8; 8 / 16 / 32 / 32 channels)  32x48, 48x32: maps 32x48, 16x24, 8x12, 4x6 (24 attention tokens)
                      four_sr   (its lowres_cond twin)                       64x96, 96x64: maps 64x96, 32x48, 16x24, 8x12 — rows of 96, 48, 24 and 12
                    each with the same unet's forward on the centre-cropped square input (`*_crop`)
  rect_sample_<run>.pt  sampling runs over (tiny, tiny_sr): the reference's own p_sample_loop(unet, shape, ...) per stage — its Imagen.sample is
                    square only, so the stage loop of ip.py:2405-2470 is restated here, its one resize made with
                    F.interpolate(img, (H, W), mode='nearest') (the reference's resize_image_to takes a single int) — as a DDPM cascade
                    16x24 -> 32x48 and its transposed twin, with a negative prompt, with init_images / skip_steps and with inpainting; and
                    the Karras loop through ElucidatedImagen.one_unet_sample.  Every run also from the centre-cropped square start.
  rect_w_<unet>_<k>.pt  the parameters of each unet: one flat fp16 tensor, (dim-8 unets: one part each; cut into parts of at most 0.9 MB if one ever grows), plus the ordered (key, shape) index

Only tensors and constructor kwargs are stored.  The weights are rounded to fp16 BEFORE the reference runs.  Each rectangular record must
lie further than DISCRIMINATION bars from the square one (a run that ignored the extra columns would not): asserted here, re-asserted by
the tests from the stored tensors.  Everything is recorded twice and must come out equal bit for bit."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from make_headdim128_golden import same  # noqa: E402
from make_negprompt_golden import mask_of, negative_prompt  # noqa: E402
from make_selfcond_golden import pack_unet, round_to_half  # noqa: E402
from oracle.make_golden import ELUCIDATED_HP, _derandomise, _record_draws  # noqa: E402
from oracle.ref_shim import load_reference  # noqa: E402
from fixtures_common import nerr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DISCRIMINATION = 10.0
BAR = {"forward": 1e-2, "ddpm": 2e-2, "edm": 3e-2}     # tests/test_plan_interp.py, tests/test_sample_cpu_replay.py
TINY = dict(dim=8, dim_mults=(1, 2), num_resnet_blocks=1, attn_heads=2, layer_attns=(False, True), layer_cross_attns=(False, True), cond_dim=32,
            text_embed_dim=32, attn_pool_num_latents=8, max_text_len=16)
FOUR = dict(TINY, dim_mults=(1, 2, 4, 4), layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True))
MODELS = {"tiny": dict(TINY), "tiny_sr": dict(TINY, lowres_cond=True), "memeff": dict(TINY, memory_efficient=True),
          "comb": dict(TINY, combine_upsample_fmaps=True, pixel_shuffle_upsample=False), "linx": dict(TINY, use_linear_cross_attn=(True, False)),
          "four": dict(FOUR), "four_sr": dict(FOUR, lowres_cond=True)}
SEED = {n: 211 + 6 * i for i, n in enumerate(MODELS)}
SHAPES = {"tiny": ((16, 24), (24, 16), (32, 48)), "memeff": ((16, 24), (24, 16), (32, 48)), "comb": ((16, 24), (24, 16), (32, 48)),
          "linx": ((16, 24), (24, 16), (32, 48)), "four": ((32, 48), (48, 32)), "four_sr": ((64, 96), (96, 64))}
T, R, SKIP, COND_SCALE = 3, 2, 1, 3.
PART_BYTES = 900_000
EDM_COND_SCALE = 3.
HP = dict(ELUCIDATED_HP, num_sample_steps=T, sigma_max=20)
CASCADE = ("tiny", "tiny_sr")


def build(ip, name):
    torch.manual_seed(SEED[name])
    u = ip.Unet(**MODELS[name]).eval()
    _derandomise(u)
    round_to_half(u)
    return u


def crop(t, axes=(-2, -1)):
    """The centre square of the last two axes."""
    H, W = t.shape[-2:]
    s = min(H, W)
    y0, x0 = (H - s) // 2, (W - s) // 2
    return t[..., y0:y0 + s, x0:x0 + s]


def forward_record(u, H, W, seed, B=2):
    g = torch.Generator().manual_seed(seed)
    rec = dict(x=torch.randn(B, 3, H, W, generator=g), time=torch.tensor([0.6, -1.9][:B]), text_embeds=torch.randn(B, 11, 32, generator=g),
               text_mask=torch.ones(B, 11, dtype=torch.bool))
    rec["text_mask"][B - 1, 6:] = False
    kw = dict(text_embeds=rec["text_embeds"], text_mask=rec["text_mask"])
    low = {}
    if u.lowres_cond:
        rec["lowres_cond_img"] = torch.randn(B, 3, H, W, generator=g)
        rec["lowres_noise_times"] = torch.tensor([0.3, 1.1][:B])
        low = dict(lowres_cond_img=rec["lowres_cond_img"], lowres_noise_times=rec["lowres_noise_times"])
    with torch.no_grad():
        for branch, drop in (("out_cond", 0.), ("out_null", 1.)):
            rec[branch] = u(rec["x"], rec["time"], cond_drop_prob=drop, **kw, **low)
            sq = {k: crop(v) for k, v in low.items() if k == "lowres_cond_img"}
            rec[branch + "_crop"] = u(crop(rec["x"]).contiguous(), rec["time"], cond_drop_prob=drop, **kw, **{**low, **sq}).half()   # (only the separation reads it)
            gap = nerr(crop(rec[branch]), rec[branch + "_crop"])
            assert gap >= DISCRIMINATION * BAR["forward"], (H, W, branch, gap)
    return rec


class both_axes_resize:
    """The reference's UpsampleCombiner resizes every feature map with resize_image_to(fmap, x.shape[-1]) (ip.py:1104-1106), which takes a
    single int and would make the map W x W.  For the `comb` records that one call scales BOTH axes by the factor the width asks for — the
    same nearest interpolation, the restatement the stage loop below makes for the cascade's resize."""

    def __init__(self, ip):
        self.ip = ip

    def __enter__(self):
        self.real = self.ip.resize_image_to
        self.ip.resize_image_to = lambda im, size, **kw: im if im.shape[-1] == size else \
            F.interpolate(im, (im.shape[-2] * size // im.shape[-1], size), mode="nearest")

    def __exit__(self, *exc):
        self.ip.resize_image_to = self.real


def forward_file(ip, name):
    """One file per unet (the 64x96 records of four_sr, batch 1, are 0.3 MB each)."""
    u = build(ip, name)
    with both_axes_resize(ip):
        recs = {f"{H}x{W}": forward_record(u, H, W, 300 + H, B=1 if name == "four_sr" else 2) for H, W in SHAPES[name]}
    print(f"forward [{name}]: " + ", ".join(f"{k} |rect - square| {nerr(crop(r['out_cond']), r['out_cond_crop']):.2f}" for k, r in recs.items()))
    return dict(records=recs, forward_bar=BAR["forward"], discrimination=DISCRIMINATION, generator="tools/make_rect_golden.py",
                reference="lucidrains/imagen-pytorch v2.0.0 Unet.forward on H x W inputs (imagen_pytorch.py:1524-1725)")


def weight_files(ip):
    """{file name: record}: the flat fp16 parameters of each unet in parts of at most PART_BYTES, kwargs and index in the first (a committed file holds at most 1 MiB)."""
    files = {}
    for name in MODELS:
        spec = pack_unet(build(ip, name), dict({"lowres_cond": False}, **MODELS[name]))
        n = spec["flat"].numel()
        parts = -(-2 * n // PART_BYTES)
        step = -(-n // parts)
        for k in range(parts):
            head = dict(kwargs=spec["kwargs"], index=spec["index"], parts=parts) if k == 0 else {}
            files[f"rect_w_{name}_{k}.pt"] = dict(head, flat=spec["flat"][k * step:(k + 1) * step].clone())
    return files


def stage_loop(model, shapes, one_stage, te, *, init_images=None, raw_level=False):
    """ip.py:2405-2470 / el.py:668-735 over rectangular stage shapes: the low-res conditioning of a stage is the previous stage's [0, 1]
    output, nearest-resized to (H, W), normalised and augmented with one Gaussian draw."""
    B, img, outs = te.shape[0], None, []
    for i, (unet, (H, W)) in enumerate(zip(model.unets, shapes)):
        kw = {}
        if unet.lowres_cond:
            times = model.lowres_noise_schedule.get_times(B, model.lowres_sample_noise_level, device=te.device)
            low = model.normalize_img(F.interpolate(img, (H, W), mode="nearest"))
            low, *_ = model.lowres_noise_schedule.q_sample(x_start=low, t=times, noise=torch.randn_like(low))
            kw = dict(lowres_cond_img=low, lowres_noise_times=times)
        init = None if init_images is None else model.normalize_img(F.interpolate(init_images, (H, W), mode="nearest"))
        img = one_stage(i, unet, (B, 3, H, W), init, kw)
        outs.append(img.clone())
    return outs


def tags(draws, stages, first=0, inner=0, inpaint=False):
    """Order of the draws (ip.py:2449, 2195, 2244, 2160, 2269; el.py:703, 442, 507, 532): per stage [low-res augmentation], init, then per
    (inner) step [known-image noise (DDPM inpainting),] step [, re-noise unless r == 0 / last timestep]."""
    noise, it = {}, iter(draws)
    for stage in range(stages):
        if stage > 0:
            noise[("lowres", stage)] = next(it)
        noise[("init", stage)] = next(it)
        for i in range(first, T):
            if not inner:
                noise[("step", stage, i)] = next(it)
                continue
            for r in reversed(range(inner)):
                if inpaint:
                    noise[("inpaint", stage, i, r)] = next(it)
                noise[("step", stage, i, r)] = next(it)
                if r > 0 and i < T - 1:
                    noise[("renoise", stage, i, r)] = next(it)
    assert next(it, None) is None
    return noise


RUNS = ("ddpm", "ddpm_tall", "neg", "init_skip", "inpaint", "edm")


def sample_file(ip, el, only):
    """One file per run (the draws of the inpainting run alone are 0.6 MB)."""
    g = torch.Generator().manual_seed(401)
    te = torch.randn(2, 9, 32, generator=g)
    neg = torch.randn(1, 5, 32, generator=g)
    mask = mask_of(te)
    init_images = torch.rand(2, 3, 16, 24, generator=g)
    inpaint_images = torch.rand(2, 3, 32, 48, generator=g)
    inpaint_masks = torch.rand(2, 32, 48, generator=g) > 0.75      # (a quarter of the pixels known, and one block: the known pixels are the same in
    inpaint_masks[:, 8:14, 4:16] = True                            # the square twin, so more of them would pull the two runs together)

    def models():
        us = [build(ip, n) for n in CASCADE]
        ddpm = ip.Imagen((ip.Unet(**TINY), ip.Unet(**TINY)), image_sizes=(16, 32), timesteps=T, text_embed_dim=32, cond_drop_prob=0.1).eval()
        edm = el.ElucidatedImagen((ip.Unet(**TINY), ip.Unet(**TINY)), image_sizes=(16, 32), text_embed_dim=32, cond_drop_prob=0.1, **HP).eval()
        for m in (ddpm, edm):
            for u, src in zip(m.unets, us):
                u.load_state_dict(src.state_dict())      # (cast_model_parameters re-instantiated the second unet with lowres_cond)
        return ddpm, edm

    ddpm, edm = models()

    def ddpm_run(shapes, inpaint=None, init=None, skip=None):
        def one(i, unet, shape, init_i, kw):
            ik = {}
            if inpaint is not None:      # (given at each stage's own size: resize_to(image, shape[-1]) is then the identity, ip.py:2221)
                ik = dict(inpaint_images=F.interpolate(inpaint[0], shape[-2:], mode="nearest"),
                          inpaint_masks=F.interpolate(inpaint[1][:, None].float(), shape[-2:], mode="nearest")[:, 0].bool(), inpaint_resample_times=R)
            return ddpm.p_sample_loop(unet, shape, noise_scheduler=ddpm.noise_schedulers[i], text_embeds=te, text_mask=mask, cond_scale=COND_SCALE,
                                      pred_objective=ddpm.pred_objectives[i], dynamic_threshold=ddpm.dynamic_thresholding[i], init_images=init_i,
                                      skip_steps=skip, use_tqdm=False, **ik, **kw)
        return stage_loop(ddpm, shapes, one, te, init_images=init)

    def edm_run(shapes):
        def one(i, unet, shape, init_i, kw):
            return edm.one_unet_sample(unet, shape, unet_number=i + 1, text_embeds=te, text_mask=mask, cond_scale=EDM_COND_SCALE,
                                       dynamic_threshold=edm.dynamic_thresholding[i], use_tqdm=False, **kw)
        return stage_loop(edm, shapes, one, te)

    wide, tall, square = ((16, 24), (32, 48)), ((24, 16), (48, 32)), ((16, 16), (32, 32))
    jobs = {
        "ddpm": (lambda s: ddpm_run(s), wide, {}, {}, "ddpm"),
        "ddpm_tall": (lambda s: ddpm_run(s), tall, {}, {}, "ddpm"),
        "neg": (lambda s: ddpm_run(s), wide, {}, dict(negative_text_embeds=neg, negative_text_masks=mask_of(neg)), "ddpm"),
        "init_skip": (lambda s: ddpm_run(s, init=init_images if s[0][1] == 24 else crop(init_images), skip=SKIP), wide, dict(first=SKIP),
                      dict(init_images=init_images, skip_steps=SKIP), "ddpm"),
        "inpaint": (lambda s: ddpm_run(s, inpaint=(inpaint_images, inpaint_masks) if s[0][1] == 24 else (crop(inpaint_images), crop(inpaint_masks))),
                    wide, dict(inner=R, inpaint=True), dict(inpaint_images=inpaint_images, inpaint_masks=inpaint_masks, inpaint_resample_times=R), "ddpm"),
        "edm": (lambda s: edm_run(s), wide, {}, dict(cond_scale=EDM_COND_SCALE), "edm"),
    }
    runs = {}
    for name, (fn, shapes, tag_kw, extra, kind) in jobs.items():
        if name != only:
            continue
        import contextlib
        ctx = (lambda: negative_prompt(ddpm, neg, mask_of(neg))) if name == "neg" else contextlib.nullcontext
        torch.manual_seed(409)
        with ctx(), torch.no_grad():
            outs, draws = _record_draws(lambda: fn(shapes))
        torch.manual_seed(409)
        with ctx(), torch.no_grad():
            far = fn(square)
        gaps = [nerr(crop(a), b) for a, b in zip(outs, far)]
        print(f"{name}: {len(draws)} draws, |rect - square start| per stage = {['%.3f' % v for v in gaps]}")
        assert min(gaps) >= DISCRIMINATION * BAR[kind], (name, gaps)
        runs[name] = dict(noise=tags(draws, 2, **tag_kw), outputs=outs, outputs_square=[o.half() for o in far], image_shapes=shapes, bar=BAR[kind],
                          kind=kind, **extra)
    return dict(unets=CASCADE, image_sizes=(16, 32), timesteps=T, hparams=dict(HP), cond_scale=COND_SCALE, text_embeds=te, run=runs[only],
                discrimination=DISCRIMINATION, generator="tools/make_rect_golden.py",
                reference="lucidrains/imagen-pytorch v2.0.0 Imagen.p_sample_loop / ElucidatedImagen.one_unet_sample at H x W shapes, stage loop restated")


def main():
    ip, el = load_reference("imagen_pytorch"), load_reference("elucidated_imagen")
    w, w2 = weight_files(ip), weight_files(ip)
    jobs = [(f"rect_forward_{name}.pt", lambda name=name: forward_file(ip, name)) for name in SHAPES] + [(f"rect_sample_{r}.pt", lambda r=r: sample_file(ip, el, r)) for r in RUNS]
    jobs += [(name, (lambda name=name, it=iter((w, w2)): next(it)[name])) for name in w]
    for fname, make in jobs:
        rec, again = make(), make()
        assert same(rec, again), f"{fname}: two recordings differ"
        blobs = []
        for r in (rec, again):
            buf = io.BytesIO()
            torch.save(r, buf)
            blobs.append(buf.getvalue())
        assert blobs[0] == blobs[1], f"{fname}: two recordings serialise to different bytes"
        path = os.path.join(GOLDEN, fname)
        with open(path, "wb") as f:
            f.write(blobs[0])
        print(f"wrote {path} ({os.path.getsize(path)} bytes), recorded twice: identical")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
