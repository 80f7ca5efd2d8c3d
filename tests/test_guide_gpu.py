"""MI355X (-m gpu): guidance rescale and adaptive projected guidance of Imagen.sample on the HIP path — GUIDE_X0 (csrc/sampler.hip) in place of
CFG_X0 on the guided steps.  The kernel itself is checked per element by tests/test_guide_kernel_gpu.py; here the sampled images:

  the recorded runs of the restatement (tests/fixtures_guide.py, tests/golden/guide_runs.pt), bar 2e-2 (the project's bar of a sampled stage),
  each more than 2 bars from its plain-CFG twin; hipGraph replay == eager launches, bit for bit; a second call on the cached stages == the
  first (the running average is reset by the stage's head); merged requests with a common keyword against each request's own call, bar 2e-3
  (the merged-requests bar of tests/test_negative_prompt_gpu.py); lanes == sequential, bit-exact."""
import os
import sys
import threading

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_guide as fgd  # noqa: E402
import fixtures_solver as fs  # noqa: E402
from conftest import gpu_device, record_parity  # noqa: E402
from fixtures_guide import nerr  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 2e-2
MERGED_BAR = 2e-3


def _common(te, noise, dev, **kw):
    return dict(text_embeds=te.to(dev), cond_scale=fgd.COND_SCALE, use_tqdm=False, noise_fn=noise, **kw)


@pytest.mark.parametrize("which", ["rescale", "apg"])
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m", "ddim"])
def test_cascade_vs_restatement(sampler, which):
    dev = gpu_device()
    g = fs.cascade_fixture()
    grp = fgd.runs_fixture()["groups"][f"cascade.{sampler}"]
    steps, want, twin = grp["steps"], grp["runs"][which], grp["twin"]
    model = fs.cascade_model(dev, timesteps=steps) if sampler == "ddpm" else fs.cascade_model(dev)
    solver = {} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=steps)
    kw = _common(g["text_embeds"], fs.fixed_noise(grp["noise"], dev), dev, return_all_unet_outputs=True, **solver)
    outs = [o.cpu() for o in model.sample(**kw, **fgd.KEYWORDS[which])]
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    gaps = [nerr(o, t) for o, t in zip(outs, twin)]
    print(f"{sampler}, {which} at {steps} steps vs the restatement: stage 1 {errs[0]:.2e}, stage 2 {errs[1]:.2e}; from the plain-CFG twin {gaps[0]:.2e}, {gaps[1]:.2e}")
    record_parity(f"guide_sample[{sampler}-{which}]", stage1=errs[0], stage2=errs[1], gap_stage1=gaps[0], gap_stage2=gaps[1])
    assert max(errs) < BAR, errs
    assert gaps[-1] > 2 * BAR, gaps
    eager = model.sample(use_graph=False, **kw, **fgd.KEYWORDS[which])
    assert all(torch.equal(a, b.cpu()) for a, b in zip(outs, eager)), "graph replay != eager"
    again = model.sample(**kw, **fgd.KEYWORDS[which])
    assert all(torch.equal(a, b.cpu()) for a, b in zip(outs, again)), "second sample() on the cached stages differs"


@pytest.mark.parametrize("name", ["v.rescale", "selfcond.apg", "video.apg", "rect.rescale", "negative_interval.apg"])
def test_variants_vs_restatement(name):
    dev = gpu_device()
    v = fgd.variants()[name]
    grp = fgd.runs_fixture()["groups"][name]
    want, twin, steps = grp["runs"][v["which"]][0], grp["twin"][0], grp["steps"]
    model = v["model"](dev, steps)
    extra = {k: (t.to(dev) if isinstance(t, torch.Tensor) else t) for k, t in v.get("sample", {}).items()}
    kw = dict(fgd.KEYWORDS[v["which"]], **extra, **({} if v["sampler"] == "ddpm" else dict(sampler=v["sampler"], sample_steps=steps)))
    call = _common(v["te"], fs.fixed_noise(grp["noise"], dev), dev, **kw)
    out = model.sample(**call)
    err, gap = nerr(out.cpu(), want), nerr(out.cpu(), twin)
    print(f"{name}: {err:.2e} from the restatement, {gap:.2e} from the plain-CFG twin")
    record_parity(f"guide_variant[{name}]", err=err, gap=gap)
    assert tuple(out.shape) == tuple(want.shape) and err < BAR and gap > 2 * BAR
    assert torch.equal(out, model.sample(**call))


@pytest.mark.parametrize("which", ["rescale", "apg"])
def test_merged_requests_and_lanes(which):
    """sample_requests with the keyword as a common one: the statistics are per row, so every request's images are those of its own
    sample() call (bar 2e-3: another batch size may pick another tile configuration).  Two lanes from two threads == the same calls in turn."""
    dev = gpu_device()
    g = fs.cascade_fixture()
    model = fs.cascade_model(dev)
    te = g["text_embeds"].to(dev)
    common = dict(cond_scale=fgd.COND_SCALE, sampler="dpmpp_2m", sample_steps=4, **fgd.KEYWORDS[which])
    reqs = [dict(text_embeds=te[:1], seed=21), dict(text_embeds=te, seed=22)]
    merged = model.sample_requests(reqs, **common)
    own = [model.sample(use_tqdm=False, **common, **r) for r in reqs]
    plain = model.sample(use_tqdm=False, **{k: v for k, v in common.items() if not k.startswith("guidance_")}, **reqs[1])
    errs = [nerr(a, b) for a, b in zip(merged, own)]
    print(f"merged requests with {which} vs their own calls: {errs}; the keyword moves request 2 by {nerr(own[1], plain):.2e}")
    record_parity(f"guide_merged[{which}]", worst=max(errs))
    assert max(errs) < MERGED_BAR and nerr(own[1], plain) > 2 * BAR
    calls = [dict(text_embeds=te, seed=31, use_tqdm=False, **common), dict(text_embeds=te * 0.9, seed=32, use_tqdm=False, **common)]
    seq = [model.sample(**c) for c in calls]
    got = [None, None]

    def work(i):
        with model.lane(i + 1), torch.cuda.device(dev):
            got[i] = model.sample(**calls[i])
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(o is not None and torch.equal(o, s) for o, s in zip(got, seq)), "lanes != sequential"
