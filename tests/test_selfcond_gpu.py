"""MI355X: self-conditioning unets under the Karras et al. sampler, and Unet3D(self_cond=True) as a denoiser and under both samplers,
against recorded runs of the live reference with identical Gaussian draws (tests/golden/selfcond_*.pt, tools/make_selfcond_golden.py; the
same runs recorded with `self_cond` forced to None lie >= 10 bars away, tests/test_selfcond_cpu.py).

Bars are those of the existing tests of the same kind: 3e-2 for the Elucidated fixture runs and their options
(tests/test_model_gpu.py::test_elucidated_sample_options_vs_reference_fixture), 1e-2 / 2e-2 (CFG) for the tiny Unet3D forwards, 2e-2 for the
video DDPM cascade and 5e-2 for the video Elucidated run (tests/test_video_gpu.py).

Every test prints its measured figures before it asserts (and records them through conftest.record_parity).  Measured on MI355X (normwise):
  * Elucidated, image, stage 1 / stage 2 alone: plain 3.82e-3 / 7.46e-3, skip_steps = 1 1.23e-3 / 7.58e-3, inpainting with two resamples
    1.81e-3 / 3.45e-3, under the bar of 3e-2; the yardstick, the same sampler on the cascade without self_cond, 7.95e-3 / 8.91e-3; the runs
    recorded with self_cond forced to None lie 0.54 / 0.47 / 0.38 away;
  * Unet3D(self_cond=True).forward: cond 6.70e-4, null 6.54e-4, without a clip 2.32e-3 (bar 1e-2); CFG 1.89e-3, CFG without a clip 2.48e-3
    (bar 2e-2);
  * video samples: DDPM 1.20e-3 (bar 2e-2), Elucidated 2.80e-3 (bar 5e-2); without self_cond 0.62 / 0.71 away."""
import os
import sys

import pytest
import torch

from conftest import gpu_device, record_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_selfcond as sc  # noqa: E402
from fixtures_selfcond import nerr  # noqa: E402

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def image_model():
    return sc.image_model(gpu_device())


def _common(g, run, dev):
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in run["kwargs"].items()}
    return dict(text_embeds=g["text_embeds"].to(dev), cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=lambda t, shape: run["noise"][t].to(dev), **kw)


@pytest.mark.parametrize("tag", ["plain", "skip", "inpaint"])
def test_elucidated_self_cond_sample_vs_reference_fixture(image_model, tag):
    """ElucidatedImagen.sample over two Unet(self_cond=True) stages (16^2 -> 32^2, 4 Karras steps, CFG 3, injected draws): the plain run,
    skip_steps = 1 (the first evaluation self-conditions on zeros) and inpainting with inpaint_resample_times = 2 (the value carries over
    from one resample to the next, the last timestep's too) against fixture (b); hipGraph replay == eager bit for bit; a second sample() on
    the cached stage == the first (self_cond_in is zeroed again).  Beside the error, the one of the same sampler on the cascade WITHOUT
    self_cond (tests/golden/sample_tiny_elucidated.pt) as the yardstick."""
    dev = gpu_device()
    g, _ = sc.image_fixture()
    run = g["runs"][tag]
    common = _common(g, run, dev)
    outs = image_model.sample(return_all_unet_outputs=True, **common)
    eager = image_model.sample(return_all_unet_outputs=True, use_graph=False, **common)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "graph replay != eager"
    again = image_model.sample(return_all_unet_outputs=True, **common)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "second sample() on the cached stage differs: self_cond_in not re-zeroed"
    e0 = nerr(outs[0], run["outputs"][0])
    alone = image_model.sample(start_at_unet_number=2, start_image_or_video=run["outputs"][0].to(dev), **common)
    e1 = nerr(alone, run["outputs"][1])
    far = nerr(outs[0], run["outputs_without_self_cond"][0])
    print(f"self-conditioning EDM [{tag}] vs reference: stage 1 {e0:.2e}, stage 2 alone {e1:.2e}; from the run without self_cond {far:.2e}")
    if tag == "plain":
        y0, y1 = _yardstick(dev)
        print(f"    yardstick, the cascade without self_cond (sample_tiny_elucidated.pt): stage 1 {y0:.2e}, stage 2 alone {y1:.2e}")
    record_parity(f"selfcond_edm[{tag}]", stage1=e0, stage2_alone=e1)
    assert e0 < 3e-2 and e1 < 3e-2, (tag, e0, e1)
    assert far > 10 * 3e-2, far
    if tag == "inpaint":
        m = run["kwargs"]["inpaint_masks"][:, None].expand(-1, 3, -1, -1)
        assert torch.allclose(alone.cpu()[m], run["kwargs"]["inpaint_images"][m], atol=1e-6)


def _yardstick(dev):
    from imagen_pytorch_amd import ElucidatedImagen, Unet

    g = torch.load(os.path.join(sc.GOLDEN, "sample_tiny_elucidated.pt"), weights_only=False)
    model = ElucidatedImagen(tuple(Unet(**u["kwargs"]).eval() for u in g["unets"]), image_sizes=g["image_sizes"], text_embed_dim=32,
                             cond_drop_prob=0.1, **g["hparams"]).to(dev).eval()
    for m, u in zip(model.unets, g["unets"]):
        m.load_state_dict(u["state_dict"])
    common = dict(text_embeds=g["text_embeds"].to(dev), cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=lambda t, shape: g["noise"][t].to(dev))
    outs = model.sample(return_all_unet_outputs=True, **common)
    alone = model.sample(start_at_unet_number=2, start_image_or_video=g["outputs"][0].to(dev), **common)
    return nerr(outs[0], g["outputs"][0]), nerr(alone, g["outputs"][1])


def test_unet3d_self_cond_forward_vs_reference_fixture():
    """Unet3D(self_cond=True).forward, 4 frames at 16^2, with a self-conditioning clip and without (zeros), and under CFG: fixture (a)."""
    dev = gpu_device()
    g, _ = sc.video_fixture()
    f = g["forward"]
    u = sc.video_unet().to(dev)
    kw = dict(text_embeds=f["text_embeds"].to(dev), text_mask=f["text_mask"].to(dev))
    x, t, clip = f["x"].to(dev), f["time"].to(dev), f["self_cond"].to(dev)
    e_c = nerr(u(x, t, self_cond=clip, **kw), f["out_cond"])
    e_n = nerr(u(x, t, self_cond=clip, cond_drop_prob=1.0, **kw), f["out_null"])
    e_z = nerr(u(x, t, **kw), f["out_cond_no_clip"])
    e_g = nerr(u.forward_with_cond_scale(x, t, self_cond=clip, cond_scale=3.0, **kw), f["out_cfg"])
    e_gz = nerr(u.forward_with_cond_scale(x, t, cond_scale=3.0, **kw), f["out_cfg_no_clip"])
    print(f"Unet3D(self_cond=True) vs reference: cond {e_c:.2e} null {e_n:.2e} no clip {e_z:.2e} cfg {e_g:.2e} cfg, no clip {e_gz:.2e}")
    record_parity("selfcond_unet3d_forward", cond=e_c, null=e_n, no_clip=e_z, cfg=e_g, cfg_no_clip=e_gz)
    assert max(e_c, e_n, e_z) < 1e-2 and max(e_g, e_gz) < 2e-2


@pytest.mark.parametrize("kind,bar", [("ddpm", 2e-2), ("edm", 5e-2)])
def test_video_self_cond_sample_vs_reference_fixture(kind, bar):
    """Imagen.sample (3 steps) and ElucidatedImagen.sample (3 Karras steps) over one Unet3D(self_cond=True) stage, 4 frames at 16^2, CFG 3:
    fixture (c); graph == eager; the second call on the cached stage == the first."""
    dev = gpu_device()
    g, _ = sc.video_fixture()
    run = g[kind]
    model = sc.video_model(kind, dev)
    common = dict(text_embeds=g["text_embeds"].to(dev), video_frames=g["frames"], cond_scale=g["cond_scale"], use_tqdm=False,
                  noise_fn=lambda t, shape: run["noise"][t].to(dev))
    out = model.sample(**common)
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    assert torch.equal(out, model.sample(use_graph=False, **common)) and torch.equal(out, model.sample(**common))
    e = nerr(out, run["outputs"][0])
    far = nerr(out, run["outputs_without_self_cond"][0])
    print(f"self-conditioning video {kind} vs reference: {e:.2e}; from the run without self_cond {far:.2e}")
    record_parity(f"selfcond_video[{kind}]", out=e)
    assert e < bar and far > 10 * bar, (kind, e, far)
