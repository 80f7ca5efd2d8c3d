"""MI355X: negative prompts (a second text prompt on the null rows of guidance) on the HIP path, against the recordings of the live
reference in tests/golden/negprompt_*.pt (tools/make_negprompt_golden.py; each recorded run lies >= 10 bars from its twin without the
negative prompt, tests/test_negative_prompt_cpu.py).  The bars are those of the CPU file:

  * forwards (a) prompt 5 / negative 7 tokens, (b) 7 / 3, batch-2 and batch-1 negatives, cond and negative rows separately: 1.5 x the
    larger figure the ordinary pair (learned null rows) of the same unet and prompt measures against its recording in the same run;
  * Imagen.sample 16 -> 32 and the video DDPM run: 2e-2; ElucidatedImagen.sample: 3e-2 (tests/test_sample_cpu_replay.py's bars for such
    runs without a negative prompt); hipGraph replay == eager, bit for bit;
  * sample(conditioning=handle) == the keywords, bit for bit; a merged sample_requests call, one request with a negative prompt and one
    without, each within 2e-3 of its own sample() call (tests/test_model_gpu.py::test_merged_requests_match_separate_calls's bar);
  * sampling without a negative prompt gives the same bits before and after a call with one on the same model (no stale src_idx /
    keep_u8 / staging rows);
  * sample_pipelined on a cascade with one stage at cond_scale 1 == sample(), bit for bit.

Every test prints its measured figures before it asserts (and records them through conftest.record_parity).  Measured on MI355X (normwise):
  * forwards: (a) ordinary pair cond 1.21e-3 / null 1.26e-3 (bar 1.89e-3); batch-2 negative cond 1.21e-3 / negative rows 1.21e-3, batch-1
    negative rows 1.26e-3; (b) ordinary pair 1.22e-3 / 1.26e-3 (bar 1.89e-3); negative rows 1.13e-3 (batch 2) / 1.44e-3 (batch 1); the guided
    forward at cond_scale 3: 3.2e-3 / 3.3e-3;
  * samples, stage 1 / stage 2 alone: DDPM 2.46e-3 / 6.5e-4 (bar 2e-2), Karras 9.5e-3 / 1.10e-2 (bar 3e-2), video DDPM 1.56e-3 (bar 2e-2); the
    same models without a negative prompt 1.99e-3, 1.03e-2, 1.75e-3; the twins recorded without one lie 0.33 / 0.39 / 0.46 away;
  * merged requests against their own sample() calls: 8.1e-4 (with a negative prompt) / 9.6e-4 (without), bar 2e-3."""
import os
import sys

import pytest
import torch

from conftest import gpu_device, record_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_negprompt as npf  # noqa: E402
from fixtures_negprompt import nerr  # noqa: E402

pytestmark = pytest.mark.gpu
BARS = {"ddpm": 2e-2, "edm": 3e-2, "video": 2e-2}


@pytest.fixture(scope="module")
def base_unet():
    return npf.base_unet(gpu_device())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_negative_prompt_forward_vs_reference_fixture(base_unet, tag):
    dev = gpu_device()
    f = npf.forward_fixture()
    c = f["cases"][tag]
    u = base_unet
    x, t = f["x"].to(dev), f["time"].to(dev)
    tk = dict(text_embeds=c["text_embeds"].to(dev), text_mask=c["text_mask"].to(dev))
    neg, nm = c["negative_text_embeds"].to(dev), c["negative_text_mask"].to(dev)
    B = x.shape[0]
    both = u._run(x, t, cfg=True, **tk)
    o_c, o_n = nerr(both[:B], c["out_cond"]), nerr(both[B:], c["out_null"])
    bar = 1.5 * max(o_c, o_n)
    pair = u._run(x, t, cfg=True, negative_text_embeds=neg, negative_text_mask=nm, **tk)
    e_c, e_n = nerr(pair[:B], c["out_cond"]), nerr(pair[B:], c["out_neg"])
    one = u._run(x, t, cfg=True, negative_text_embeds=neg[:1], negative_text_mask=nm[:1], **tk)
    e1_c, e1_n = nerr(one[:B], c["out_cond"]), nerr(one[B:], c["out_neg_b1"])
    far = min(nerr(pair[B:], c["out_null"]), nerr(one[B:], c["out_null"]))
    guided = u.forward_with_cond_scale(x, t, cond_scale=f["cond_scale"], negative_text_embeds=neg, negative_text_masks=nm, **tk)
    e_g = nerr(guided, c["out_neg"] + (c["out_cond"] - c["out_neg"]) * f["cond_scale"])
    print(f"negative prompt forward ({tag}) on the HIP path: ordinary pair cond {o_c:.3e} null {o_n:.3e}, bar {bar:.3e}; batch-2 negative cond {e_c:.3e} "
          f"negative rows {e_n:.3e}; batch-1 cond {e1_c:.3e} negative rows {e1_n:.3e}; guided {e_g:.3e}; from the learned-null recording {far:.3e}")
    record_parity(f"negprompt_forward[{tag}]", ordinary_cond=o_c, ordinary_null=o_n, cond=e_c, negative=e_n, cond_b1=e1_c, negative_b1=e1_n,
                  guided=e_g, bar=bar)
    assert max(e_c, e_n, e1_c, e1_n) < bar, (e_c, e_n, e1_c, e1_n, bar)
    assert far > 10 * 1e-2, far
    assert torch.equal(guided, pair[B:] + (pair[:B] - pair[B:]) * f["cond_scale"])
    # the ordinary pair afterwards, on the same engine: the bits of before
    assert torch.equal(u._run(x, t, cfg=True, **tk), both) and len(u._engines) == 1


def _common(g, run, dev, **extra):
    return dict(text_embeds=g["text_embeds"].to(dev), cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=lambda t, shape: run["noise"][t].to(dev), **extra)


@pytest.mark.parametrize("kind", ["ddpm", "edm"])
def test_image_sample_with_negative_prompt_vs_reference_fixture(kind):
    """(c) Imagen.sample / (d) ElucidatedImagen.sample, 16^2 -> 32^2, 4 steps, cond_scale 3, one negative prompt for the batch."""
    dev = gpu_device()
    g = npf.runs_fixture()
    run = g["runs"][kind]
    model = npf.image_model(kind, dev)
    common = _common(g, run, dev)
    neg = dict(negative_text_embeds=run["negative_text_embeds"].to(dev))
    plain_before = model.sample(return_all_unet_outputs=True, **common)
    outs = model.sample(return_all_unet_outputs=True, **common, **neg)
    eager = model.sample(return_all_unet_outputs=True, use_graph=False, **common, **neg)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "graph replay != eager"
    e0 = nerr(outs[0], run["outputs"][0])
    alone = model.sample(start_at_unet_number=2, start_image_or_video=run["outputs"][0].to(dev), **common, **neg)
    e1 = nerr(alone, run["outputs"][1])
    p0 = nerr(plain_before[0], run["outputs_without_negative"][0])
    far = min(nerr(a, b) for a, b in zip(outs, run["outputs_without_negative"]))
    print(f"negative prompt {kind} vs reference: stage 1 {e0:.2e}, stage 2 alone {e1:.2e}; without a negative prompt, stage 1 {p0:.2e}; "
          f"from the twin without one {far:.2e}")
    record_parity(f"negprompt_sample[{kind}]", stage1=e0, stage2_alone=e1, plain_stage1=p0)
    bar = BARS[kind]
    assert e0 < bar and e1 < bar, (kind, e0, e1)
    assert p0 < bar and far > 10 * bar
    handle = model.prepare_conditioning(text_embeds=common["text_embeds"], **neg)
    by_handle = model.sample(return_all_unet_outputs=True, conditioning=handle, **{k: v for k, v in common.items() if k != "text_embeds"})
    assert all(torch.equal(a, b) for a, b in zip(outs, by_handle)), "sample(conditioning=handle) != the keywords"
    after = model.sample(return_all_unet_outputs=True, **common)
    assert all(torch.equal(a, b) for a, b in zip(after, plain_before)), "sampling without a negative prompt changed after a call with one"
    assert len(model._stages) == 2


def test_video_sample_with_negative_prompt_vs_reference_fixture():
    """(e) a video DDPM run of 4 frames at 16^2, one negative prompt per sample, longer than the prompts."""
    dev = gpu_device()
    g = npf.runs_fixture()
    run = g["runs"]["video"]
    model = npf.video_model(dev)
    common = _common(g, run, dev, video_frames=g["frames"])
    neg = dict(negative_text_embeds=run["negative_text_embeds"].to(dev))
    plain_before = model.sample(**common)
    out = model.sample(**common, **neg)
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    assert torch.equal(out, model.sample(use_graph=False, **common, **neg)), "graph replay != eager"
    e, p, far = nerr(out, run["outputs"][0]), nerr(plain_before, run["outputs_without_negative"][0]), nerr(out, run["outputs_without_negative"][0])
    print(f"negative prompt video DDPM vs reference: {e:.2e}; without a negative prompt {p:.2e}; from the twin without one {far:.2e}")
    record_parity("negprompt_sample[video]", out=e, plain=p)
    assert e < BARS["video"] and p < BARS["video"] and far > 10 * BARS["video"]
    assert torch.equal(model.sample(**common), plain_before), "sampling without a negative prompt changed after a call with one"
    assert len(model._stages) == 1


def test_merged_requests_with_and_without_a_negative_prompt_match_separate_calls():
    """One request with a negative prompt and one without, merged: each gets the images of its own sample() call (in-kernel Philox noise)."""
    dev = gpu_device()
    g = npf.runs_fixture()
    model = npf.image_model("ddpm", dev)
    te = g["text_embeds"].to(dev)
    neg = g["runs"]["ddpm"]["negative_text_embeds"].to(dev)
    reqs = [dict(text_embeds=te, negative_text_embeds=neg, seed=41), dict(text_embeds=te[:1, :7].contiguous(), seed=42)]
    alone = [model.sample(cond_scale=3.0, use_tqdm=False, **r) for r in reqs]
    merged = model.sample_requests(reqs, cond_scale=3.0)
    errs = [nerr(m, a) for m, a in zip(merged, alone)]
    other = nerr(merged[0], model.sample(cond_scale=3.0, use_tqdm=False, text_embeds=te, seed=41))
    print(f"merged requests, with / without a negative prompt, vs their own sample() calls: {errs[0]:.2e} / {errs[1]:.2e}; "
          f"the first from its call without the negative prompt {other:.2e}")
    record_parity("negprompt_merged_requests", with_negative=errs[0], without=errs[1])
    assert [tuple(m.shape) for m in merged] == [tuple(a.shape) for a in alone]
    assert max(errs) < 2e-3, errs
    assert other > 0.05


def test_pipelined_cascade_with_an_unguided_stage_matches_sample():
    """sample_pipelined with a negative prompt on a cascade whose second stage runs at cond_scale 1 (it has no null rows): bit-identical,
    per batch, to sample() with the same keywords and seeds — with one batch that has a negative prompt and one that has none."""
    dev = gpu_device()
    g = npf.runs_fixture()
    model = npf.image_model("ddpm", dev)
    te = g["text_embeds"].to(dev)
    neg = g["runs"]["ddpm"]["negative_text_embeds"].to(dev)
    batches = [dict(text_embeds=te, negative_text_embeds=neg, seed=61), dict(text_embeds=te, seed=62)]
    seq = [model.sample(cond_scale=(3.0, 1.0), use_tqdm=False, **b) for b in batches]
    pipe = model.sample_pipelined(batches, cond_scale=(3.0, 1.0))
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq))
    assert not torch.equal(seq[0], model.sample(cond_scale=(3.0, 1.0), use_tqdm=False, text_embeds=te, seed=61))
