"""MI355X: the few-step solvers of Imagen.sample (sampler='dpmpp_2m' | 'ddim') on the HIP path.  No kernel is new: a
solver step is the denoiser plan, CFG_X0, QUANTILE and one (ddim) or two (dpmpp_2m: update + history copy) LINCOMB launches.

The restatement the samples are compared with is tests/fixtures_solver.py (the formulas in decimal arithmetic, applied in a plain fp32
loop over the oracle's guided forward), recorded once in tests/golden/solver_runs.pt; tests/test_solver_cpu.py recomputes it.

Bars are those of the existing tests of the same kind: 2e-2 for a DDPM sample of the tiny cascade and of the tiny Unet3D / self_cond stages
(tests/test_model_gpu.py::test_sample_vs_reference_fixture, tests/test_video_gpu.py, tests/test_selfcond_gpu.py), 2e-3 for merged
requests against their own calls (tests/test_model_gpu.py).  Every test prints its figures before it asserts and records them through
conftest.record_parity.  Measured on MI355X: see the docstrings (profiles/solver_parity_mi355x.json)."""
import os
import sys

import pytest
import torch

from conftest import gpu_device, record_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_solver as fs  # noqa: E402
from fixtures_solver import nerr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 2e-2


@pytest.fixture(scope="module")
def cascade():
    return fs.cascade_model(gpu_device())


def _common(g, noise, dev, **kw):
    return dict(text_embeds=g["text_embeds"].to(dev), cond_scale=fs.COND_SCALE, use_tqdm=False, noise_fn=noise, **kw)


@pytest.mark.parametrize("sampler", ["dpmpp_2m", "ddim"])
def test_solver_samples_vs_restatement(cascade, sampler):
    """8 + 10: the tiny cascade (16^2 -> 32^2, low-res conditioning, CFG 3, dynamic thresholding) at 6 solver steps against the
    restatement, bar 2e-2; hipGraph replay == eager launches bit for bit; a second call on the cached stages == the first.
    Measured on MI355X, stage 1 / stage 2: dpmpp_2m 6.7e-4 / 4.3e-4, ddim 8.5e-4 / 4.1e-4."""
    dev = gpu_device()
    g, run = fs.cascade_fixture(), fs.runs_fixture()["runs"][f"cascade.{sampler}"]
    kw = _common(g, fs.fixed_noise(run["noise"], dev), dev, sampler=sampler, sample_steps=fs.STEPS, return_all_unet_outputs=True)
    outs = cascade.sample(**kw)
    errs = [nerr(o, w) for o, w in zip(outs, run["outputs"])]
    print(f"{sampler} at {fs.STEPS} steps vs the restatement: stage 1 {errs[0]:.2e}, stage 2 {errs[1]:.2e}")
    record_parity(f"solver_sample[{sampler}]", stage1=errs[0], stage2=errs[1])
    assert max(errs) < BAR, errs
    eager = cascade.sample(use_graph=False, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "graph replay != eager"
    again = cascade.sample(**kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "second sample() on the cached stages differs"


def test_ddim_eta_1_reproduces_the_references_ddpm_run(cascade):
    """9: sample(sampler='ddim', eta=1, sample_steps=T) with the recorded draws of the reference's DDPM run injected (the step draw
    as LINCOMB's t2) against that run, under the bar of the DDPM fixture test (2e-2); no DDPM_UPDATE in the launch lists.
    Measured on MI355X: 1.08e-3 / 5.1e-4 (the DDPM sampler on the same draws: 1.08e-3 / 5.2e-4)."""
    from imagen_pytorch_amd import ops

    dev = gpu_device()
    g = fs.cascade_fixture()
    kw = dict(text_embeds=g["text_embeds"].to(dev), cond_scale=g["cond_scale"], use_tqdm=False, return_all_unet_outputs=True,
              noise_fn=fs.fixed_noise(g["noise"], dev))
    outs = cascade.sample(sampler="ddim", eta=1.0, sample_steps=g["timesteps"], **kw)
    errs = [nerr(o, r) for o, r in zip(outs, g["outputs"])]
    ddpm = [nerr(o, r) for o, r in zip(cascade.sample(**kw), g["outputs"])]
    print(f"ddim(eta = 1, T = {g['timesteps']}) vs the reference's DDPM run: {errs}; the DDPM sampler: {ddpm}")
    record_parity("solver_anchor_ddim_eta1", stage1=errs[0], stage2=errs[1], ddpm_stage1=ddpm[0], ddpm_stage2=ddpm[1])
    assert max(errs) < BAR, errs
    for key, st in cascade._stages.items():
        if key[-1] is not None and key[-1][2] == 1.0:
            assert ops.ENUMS["IMAGEN_OP_DDPM_UPDATE"] not in {int(k) for k, _, _ in st["plan"].ops}


@pytest.mark.parametrize("sampler,eta", [("dpmpp_2m", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_seeds(cascade, sampler, eta):
    """10: without noise_fn the initial image, the low-res augmentation and — 'ddim' at eta > 0 — LINCOMB's own Philox draw are keyed
    by the call's seed: the same seed twice gives identical images, another seed other ones; graph == eager."""
    dev = gpu_device()
    te = fs.cascade_fixture()["text_embeds"].to(dev)
    kw = dict(text_embeds=te, cond_scale=fs.COND_SCALE, use_tqdm=False, sampler=sampler, sample_steps=4, eta=eta)
    a = cascade.sample(seed=5, **kw)
    assert torch.equal(a, cascade.sample(seed=5, **kw)) and torch.equal(a, cascade.sample(seed=5, use_graph=False, **kw))
    assert nerr(cascade.sample(seed=6, **kw), a) > 0.05
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    if eta > 0:
        assert nerr(cascade.sample(seed=5, **{**kw, "eta": 0.0}), a) > 1e-2, "eta must matter"


def test_entry_points(cascade):
    """11: sample_pipelined is bit-identical to sample; sample_requests under dpmpp_2m — each request within the merged-request bar
    (2e-3) of its own sample() call, and not another seed's images.  Measured on MI355X: 0 / 0 / 0 (bit-identical at these sizes)."""
    dev = gpu_device()
    te = fs.cascade_fixture()["text_embeds"].to(dev)
    common = dict(cond_scale=fs.COND_SCALE, sampler="dpmpp_2m", sample_steps=4)
    batches = [dict(text_embeds=te * s, seed=31 + i) for i, s in enumerate((1.0, 0.9, 1.1))]
    seq = [cascade.sample(use_tqdm=False, **common, **b) for b in batches]
    pipe = cascade.sample_pipelined(batches, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(pipe[0], pipe[1])
    with cascade.lane(2):
        assert torch.equal(cascade.sample(use_tqdm=False, **common, **batches[0]), seq[0])
    reqs = [dict(text_embeds=te[:1], seed=41), dict(text_embeds=te, seed=42), dict(text_embeds=te[1:], seed=43)]
    own = [cascade.sample(use_tqdm=False, **common, **r) for r in reqs]
    merged = cascade.sample_requests(reqs, **common)
    errs = [nerr(m, o) for m, o in zip(merged, own)]
    print(f"merged requests under dpmpp_2m vs their own calls: {errs}")
    record_parity("solver_merged_requests", **{f"request{i}": e for i, e in enumerate(errs)})
    assert [tuple(m.shape) for m in merged] == [tuple(o.shape) for o in own] and max(errs) < 2e-3, errs
    swapped = cascade.sample_requests([dict(reqs[0], seed=43), reqs[1], dict(reqs[2], seed=41)], **common)
    assert nerr(swapped[1], own[1]) < 2e-3 and nerr(swapped[0], own[0]) > 0.05 and nerr(swapped[2], own[2]) > 0.05
    with pytest.raises(ValueError):
        cascade.sample_requests(reqs, cond_scale=fs.COND_SCALE, sampler="ddim", eta=0.5)


@pytest.mark.parametrize("tag", ["selfcond", "video", "rect"])
def test_unet_variants_and_shapes(tag):
    """12: dpmpp_2m at 4 steps on one Unet(self_cond=True) stage (its next input is the thr1_out of the step), one Unet3D stage
    (4 frames) and the cascade's first unet at 16 x 24 (image_shapes), against the restatement, under the 2e-2 of their DDPM
    counterparts; graph == eager; the second call == the first (history and self-conditioning buffers are reset).
    Measured on MI355X: self_cond 1.93e-3, Unet3D 1.24e-3, 16 x 24 8.2e-4."""
    dev = gpu_device()
    run = fs.runs_fixture()["runs"][f"{tag}.dpmpp_2m"]
    g, kw = fs.cascade_fixture(), {}
    if tag == "selfcond":
        model = fs.single_stage_model(fs.selfcond_spec(), 16, dev)
    elif tag == "video":
        g = fs.load("sample_tiny_video.pt")
        model, kw = fs.video_model(dev), dict(video_frames=g["frames"])
    else:
        model, kw = fs.single_stage_model(fs.cascade_specs()[0], 16, dev), dict(image_shapes=((16, 24),))
    common = _common(g, fs.fixed_noise(run["noise"], dev), dev, sampler="dpmpp_2m", sample_steps=4, **kw)
    out = model.sample(**common)
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    err = nerr(out, run["outputs"][0])
    print(f"dpmpp_2m, {tag}, vs the restatement: {err:.2e}")
    record_parity(f"solver_variant[{tag}]", out=err)
    assert err < BAR
    assert torch.equal(out, model.sample(use_graph=False, **common)) and torch.equal(out, model.sample(**common))


def test_init_images_and_skip_steps(cascade):
    """init_images / skip_steps count solver steps: the run starts at row 2 of 5 (first order there: the weight row is rewritten in
    place before the cached graph replays), then the same stage runs from row 0 again.  Bar 2e-2.  Measured on MI355X: 8.4e-4 / 4.2e-4."""
    dev = gpu_device()
    g = fs.cascade_fixture()
    noise = fs.memo_noise(7)
    init = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(8))
    want = fs.solver_sample(fs.cascade_specs(), g["image_sizes"], g["text_embeds"], steps=5, sampler="dpmpp_2m", noise_fn=noise, return_all=True,
                            init_images=(init, None), skip_steps=(2, None))
    kw = _common(g, fs.fixed_noise(noise.draws, dev), dev, sampler="dpmpp_2m", sample_steps=5, return_all_unet_outputs=True)
    plain = cascade.sample(**kw)
    outs = cascade.sample(init_images=(init.to(dev), None), skip_steps=(2, None), **kw)
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"dpmpp_2m, init_images + skip_steps = 2 of 5: {errs}")
    record_parity("solver_skip_steps", stage1=errs[0], stage2=errs[1])
    assert max(errs) < BAR
    assert all(torch.equal(a, b) for a, b in zip(plain, cascade.sample(**kw))), "the weight row of the skipped start must be restored"
