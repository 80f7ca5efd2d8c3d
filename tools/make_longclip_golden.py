#!/usr/bin/env python
"""tests/golden/longclip_*.pt: recorded runs of the LIVE REFERENCE on clips longer than 32 frames (Unet3D stages of 33 .. 128 frames:
TEMPORAL_ATTENTION's tiled kernel, ABI 15), and the launch list of an existing short-clip config as it is before that change.

    python tools/make_longclip_golden.py                 # needs the reference's tree (oracle/ref_shim.py); CPU only
    python tools/make_longclip_golden.py --sample        # only longclip_sample.pt, over the recorded weights of `long`
    python tools/make_longclip_golden.py --launch-list   # only tests/golden/longclip_short_launch_list_abi14.json, from THIS tree (run it
                                                         # on the commit before the feature; no reference needed)

  longclip_unet.pt        weights of `long`: Unet3D(dim=16, dim_mults=(1, 2), attn_heads=2, attn_dim_head=64, temporal_strides=(2, 1), ...);
                          the second half of the flat tensor is in longclip_unet_part2.pt (1.1 MB in one file)
  longclip_unet_hd32.pt   weights of `long32`: the same model with attn_heads=4, attn_dim_head=32 (and longclip_unet_hd32_part2.pt)
  longclip_long.pt        `long` on 36 frames of 16 x 16: x (stored once, fp16-exact), time, text_embeds, text_mask, out_cond, out_null.
                          Level 0 attends over 36 frames (one full key tile and a 4-frame partial one), level 1 over 18
  longclip_long32.pt      `long32` on the same input
  longclip_twin.pt        `long`'s weights on the first 16 frames of the same input: the short-clip path, which anchors the tests' bar
  longclip_sample.pt      Imagen.sample (2 DDPM steps) and ElucidatedImagen.sample (2 Karras steps) over `long` at 36 frames of 8 x 8, CFG 3,
                          every Gaussian draw recorded; and the same runs on 16 frames with the first 16 frames of every draw

Only tensors and constructor kwargs are stored; weights are rounded to fp16 BEFORE the reference runs and stored as one flat fp16 tensor per
unet plus the ordered (key, shape) index (tools/make_selfcond_golden.py).  The 16-frame sampling runs must lie at least DISCRIMINATION bars
from the first 16 frames of the 36-frame ones for a test to tell a driver that sampled the short clip and repeated it; the gap of every
run is printed, stored with the run and asserted here, on the reference alone.  With the constructor defaults no seed reaches it (0.10 ..
0.14 under DDPM, 0.20 .. 0.24 under Karras over twenty seeds, against 0.2 and 0.5): a normwise figure on outputs in [0, 1] is diluted by
their mean of 0.4 .. 0.6, and a threshold at the clip's 95th percentile scales all frames of a run alike.  So the models are built with
SAMPLE_KW: auto_normalize_img=False (outputs in [-1, 1], no offset: 0.27 .. 0.37 under DDPM, 0.38 .. 0.49 under Karras) and, under
Karras, dynamic_thresholding_percentile=0.7 (the clip-wide quantile, the one statistic of the sampler that sees every frame, clamps 30 %
of x0's values: 0.50 .. 0.57).  Lower percentiles or a static clamp give 0.6 .. 0.75 but saturate half the output and more, and the
two-step run becomes ill-conditioned on the reference itself; the mildest setting that reaches the gap with a tenth of margin is used.
The parity tests measure against the same centred outputs, so their figures are about twice what outputs in [0, 1] would give."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LONG = dict(dim=16, cond_dim=32, text_embed_dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True),
            layer_cross_attns=(False, True), attn_heads=2, attn_dim_head=64, max_text_len=16, attn_pool_num_latents=8, temporal_strides=(2, 1))
LONG32 = dict(LONG, attn_heads=4, attn_dim_head=32)
FRAMES, TWIN_FRAMES, S, S_SAMPLE = 36, 16, 16, 8
BAR = {"ddpm": 2e-2, "edm": 5e-2}          # the video bars of tests/test_selfcond_gpu.py
DISCRIMINATION = 10.0
T_DDPM = 2
SAMPLE_KW = {"ddpm": dict(auto_normalize_img=False), "edm": dict(auto_normalize_img=False, dynamic_thresholding_percentile=0.7)}
WEIGHTS = {"long": ("longclip_unet.pt", "longclip_unet_part2.pt"), "long32": ("longclip_unet_hd32.pt", "longclip_unet_hd32_part2.pt")}


def _save(obj, name):
    path = os.path.join(GOLDEN, name)
    torch.save(obj, path)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size} bytes)")
    assert size < 1 << 20, "a committed file stays under 1 MiB"


def make_launch_list():
    """The 'base' clip of tests/golden/unet3d_tiny.pt (4 frames at 16 x 16): op kinds and labels of its static and step plans."""
    from imagen_pytorch_amd import Unet3D, _abi
    from imagen_pytorch_amd.engine3d import UnetEngine3D

    g = torch.load(os.path.join(GOLDEN, "unet3d_tiny.pt"), weights_only=False)["runs"]["base"]
    u = Unet3D(**g["kwargs"]).eval()
    u.load_state_dict(g["state_dict"])
    B, _, Fr, size, _ = g["x"].shape
    eng = UnetEngine3D(u, 2 * B, B, Fr, size, "cpu", dry=True)
    eng.set_conditioning(text_embeds=g["text_embeds"], text_mask=g["text_mask"], keep=torch.tensor([True] * B + [False] * B), lowres_noise_times=None)
    n = g["text_embeds"].shape[1]
    got = {"static": [[int(k), l] for k, _, l in eng._static_plans[n][0].ops], "step": [[int(k), l] for k, _, l in eng.step_plan.ops]}
    path = os.path.join(GOLDEN, f"longclip_short_launch_list_abi{_abi.ENUMS['IMAGEN_ABI_VERSION']}.json")
    with open(path, "w") as f:
        json.dump(got, f)
    print(f"wrote {path}: {len(got['static'])} static + {len(got['step'])} step launches")


def _replay_draws(fn, draws, frames):
    """fn() with torch.randn / randn_like returning the first `frames` frames of the recorded draws, in order."""
    it = iter(draws)
    real_randn, real_randn_like = torch.randn, torch.randn_like

    def take(shape):
        t = next(it)[:, :, :frames].contiguous()
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t

    torch.randn = lambda *a, **k: take(a[0] if len(a) == 1 and not isinstance(a[0], int) else a)
    torch.randn_like = lambda x, **k: take(x.shape)
    try:
        with torch.no_grad():
            out = fn()
    finally:
        torch.randn, torch.randn_like = real_randn, real_randn_like
    assert next(it, None) is None
    return out


def make_models(iv):
    from make_selfcond_golden import pack_unet, round_to_half
    from oracle.make_golden import derandomise_unet3d

    unets = {}
    for name, kw, seed, path in (("long", LONG, 71, WEIGHTS["long"]), ("long32", LONG32, 73, WEIGHTS["long32"])):
        torch.manual_seed(seed)
        u = iv.Unet3D(**kw).eval()
        derandomise_unet3d(u)
        round_to_half(u)
        spec = pack_unet(u, {**kw, "lowres_cond": False})
        half = spec["flat"].numel() // 2              # (the whole unet is 1.1 MB in fp16: two files, each under the limit)
        _save(dict(spec, flat=spec["flat"][:half].clone()), path[0])
        _save(dict(flat=spec["flat"][half:].clone()), path[1])
        unets[name] = u
    return unets


def make_forwards(unets):
    from fixtures_common import nerr

    torch.manual_seed(79)
    B = 2
    x = torch.randn(B, 3, FRAMES, S, S).half().float()
    time = torch.tensor([0.7, -2.3])
    text_embeds = torch.randn(B, 11, 32)
    text_mask = torch.ones(B, 11, dtype=torch.bool)
    text_mask[1, 7:] = False
    tk = dict(text_embeds=text_embeds, text_mask=text_mask)
    common = dict(time=time, generator="tools/make_longclip_golden.py",
                  reference="lucidrains/imagen-pytorch v2.0.0 Unet3D.forward (imagen_video.py:1650-1941)", **tk)
    outs = {}
    for name, u, xs, weights, path in (("long", unets["long"], x, WEIGHTS["long"], "longclip_long.pt"),
                                       ("long32", unets["long32"], x, WEIGHTS["long32"], "longclip_long32.pt"),
                                       ("twin", unets["long"], x[:, :, :TWIN_FRAMES].contiguous(), WEIGHTS["long"], "longclip_twin.pt")):
        with torch.no_grad():
            f = dict(common, frames=xs.shape[2], out_cond=u(xs, time, **tk), out_null=u(xs, time, cond_drop_prob=1., **tk))
        if name == "long":
            f["x"] = x.half()
        outs[name] = f
        print(f"{name}: {xs.shape[2]} frames, out_cond std {f['out_cond'].std():.3f}, out_null std {f['out_null'].std():.3f}")
        _save(dict(weights_from=weights, forward=f), path)
    gap = nerr(outs["long"]["out_cond"][:, :, :TWIN_FRAMES], outs["twin"]["out_cond"])
    print(f"first {TWIN_FRAMES} frames of the long forward vs the twin's: {gap:.3f}")


def make_sample(ip, el, unet):
    from make_selfcond_golden import edm_tags
    from oracle.make_golden import ELUCIDATED_HP, _record_draws
    from fixtures_common import nerr

    torch.manual_seed(83)
    te = torch.randn(2, 9, 32)
    hp = dict(ELUCIDATED_HP, num_sample_steps=2)
    imagen = ip.Imagen((unet,), image_sizes=(S_SAMPLE,), timesteps=T_DDPM, text_embed_dim=32, cond_drop_prob=0.1, **SAMPLE_KW["ddpm"]).eval()
    edm_model = el.ElucidatedImagen((unet,), image_sizes=(S_SAMPLE,), text_embed_dim=32, cond_drop_prob=0.1, **hp, **SAMPLE_KW["edm"]).eval()
    edm_model.unets[0].load_state_dict(unet.state_dict())
    rec = {}
    for kind, model, seed in (("ddpm", imagen, 89), ("edm", edm_model, 97)):
        call = lambda frames: model.sample(text_embeds=te, video_frames=frames, cond_scale=3., use_tqdm=False, return_all_unet_outputs=True)
        for seed in range(seed, seed + 4):   # the first seed whose two runs are DISCRIMINATION bars apart
            torch.manual_seed(seed)
            outs, draws = _record_draws(lambda: call(FRAMES))
            short = _replay_draws(lambda: call(TWIN_FRAMES), draws, TWIN_FRAMES)
            gap = nerr(outs[0][:, :, :TWIN_FRAMES], short[0])
            print(f"{kind} seed {seed}: output {tuple(outs[0].shape)}, {len(draws)} draws; first {TWIN_FRAMES} frames vs the {TWIN_FRAMES}-frame "
                  f"run: {gap:.3f} (needs >= {DISCRIMINATION * BAR[kind]:.2f})")
            if gap >= 1.1 * DISCRIMINATION * BAR[kind]:   # a tenth of margin: the code under test may differ from the reference by a bar
                break
        assert gap >= 1.1 * DISCRIMINATION * BAR[kind], f"{kind}: no seed of {seed - 3} .. {seed} separates the two runs by {DISCRIMINATION:.0f} bars and a margin"
        if kind == "ddpm":
            noise, it = {("init", 0): draws[0]}, iter(draws[1:])
            for i in range(T_DDPM):
                noise[("step", 0, i)] = next(it)
            assert next(it, None) is None
            rec[kind] = dict(timesteps=T_DDPM, noise=noise)
        else:
            rec[kind] = dict(hparams=hp, noise=edm_tags(draws, hp["num_sample_steps"], 1))
        rec[kind].update(outputs=[o.clone() for o in outs], outputs_short=[o.clone() for o in short], bar=BAR[kind], gap=gap, seed=seed)
    _save(dict(weights_from=WEIGHTS["long"], image_sizes=(S_SAMPLE,), frames=FRAMES, short_frames=TWIN_FRAMES, cond_scale=3., text_embeds=te, model_kwargs=SAMPLE_KW,
               discrimination=DISCRIMINATION, generator="tools/make_longclip_golden.py",
               reference="lucidrains/imagen-pytorch v2.0.0 Imagen.sample and ElucidatedImagen.sample over one Unet3D", **rec), "longclip_sample.pt")


if __name__ == "__main__":
    if "--launch-list" in sys.argv:
        make_launch_list()
        sys.exit(0)
    from oracle.ref_shim import load_reference

    ip, iv, el = load_reference("imagen_pytorch"), load_reference("imagen_video"), load_reference("elucidated_imagen")
    if "--sample" in sys.argv:
        import fixtures_longclip as lc

        _, kw, sd = lc.unet_record("long")
        u = iv.Unet3D(**kw).eval()
        u.load_state_dict(sd)
        make_sample(ip, el, u)
        sys.exit(0)
    unets = make_models(iv)
    make_forwards(unets)
    make_sample(ip, el, unets["long"])
