"""MI355X (-m gpu): composed prompts of Imagen.sample on the HIP path — (K + 1) B denoiser rows and COMPOSE_X0 (csrc/sampler.hip) in place of
CFG_X0.  The kernel itself is checked per element by tests/test_compose_kernel_gpu.py; here:

  * the recorded runs of the restatement (tests/fixtures_compose.py, tests/golden/compose_runs.pt), bar 2e-2 (the sample bar of
    tests/test_guide_gpu.py and tests/test_solver_gpu.py), each more than 2 bars from its plain-CFG twin; hipGraph replay == eager launches
    and a second call on the cached stages == the first, bit for bit;
  * Unet forwards at (K + 1) B rows: every branch's rows against the oracle's forward on that prompt alone, under the bar
    tests/test_negative_prompt_gpu.py uses for its forward rows — 1.5 x the larger error of the ordinary 2 B-row pair, measured here;
  * lanes == sequential and sample_pipelined == own calls, bit-exact."""
import os
import sys
import threading

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_compose as fc  # noqa: E402
import fixtures_solver as fs  # noqa: E402
from conftest import gpu_device, record_parity  # noqa: E402
from fixtures_compose import nerr  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 2e-2


@pytest.mark.parametrize("name,which", [(n, w) for n, grp in fc.groups().items() for w in grp["which"]])
def test_recorded_runs_vs_restatement(name, which):
    dev = gpu_device()
    g = fs.cascade_fixture()
    grp, rec = fc.groups()[name], fc.runs_fixture()["groups"][name]
    steps, want, twin = rec["steps"], rec["runs"][which], rec["twin"]
    model = fc.group_model(grp, dev, steps)
    kw = dict(fc.keywords(which, grp["stages"], dev), **fc.to_device(grp.get("sample", {}), dev),
              **({} if grp["sampler"] == "ddpm" else dict(sampler=grp["sampler"], sample_steps=steps)))
    call = dict(text_embeds=g["text_embeds"].to(dev), cond_scale=fc.COND_SCALE, use_tqdm=False, noise_fn=fs.fixed_noise(rec["noise"], dev),
                return_all_unet_outputs=True, **kw)
    outs = [o.cpu() for o in model.sample(**call)]
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    gaps = [nerr(o, t) for o, t in zip(outs, twin)]
    print(f"{name}, {which} at {steps} steps vs the restatement: {errs}; from the plain-CFG twin {gaps}")
    record_parity(f"compose_sample[{name}-{which}]", **{f"stage{i + 1}": e for i, e in enumerate(errs)}, **{f"gap_stage{i + 1}": e for i, e in enumerate(gaps)})
    assert [tuple(o.shape) for o in outs] == [tuple(w.shape) for w in want]
    assert max(errs) < BAR, errs
    assert gaps[-1] > 2 * BAR, gaps
    eager = model.sample(**{**call, "use_graph": False})
    assert all(torch.equal(a, b.cpu()) for a, b in zip(outs, eager)), "graph replay != eager"
    again = model.sample(**call)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(outs, again)), "second sample() on the cached stages differs"


@pytest.mark.parametrize("K", [2, 4])
def test_forward_branch_rows_vs_oracle(K):
    """The cascade's first unet at (K + 1) B rows: branch k's rows against the oracle's forward on prompt k alone, the null rows against its
    null forward, and with a negative prompt the null rows against its forward on that prompt."""
    from imagen_pytorch_amd import Unet
    from oracle.unet_oracle import unet_forward

    dev = gpu_device()
    sd, kw = fs.cascade_specs()[0]
    unet = Unet(**kw).eval()
    unet.load_state_dict(sd)
    unet = unet.to(dev)
    B, size = 2, 16
    g = torch.Generator().manual_seed(9)
    x, t = torch.randn(B, 3, size, size, generator=g), torch.tensor([0.3, -1.2])
    te = fs.cascade_fixture()["text_embeds"]
    extra = [(fc.prompt(51, batch=1, tokens=5), None), (fc.prompt(52, tokens=11), torch.rand(2, 11, generator=g) > 0.3), (fc.prompt(53, tokens=9), None)][:K - 1]
    prompts = [(te, torch.any(te != 0.0, dim=-1))] + [(e.expand(B, -1, -1), torch.any(e != 0.0, dim=-1).expand(B, -1) if m is None else m) for e, m in extra]
    with torch.no_grad():
        refs = [unet_forward(sd, kw, x, t, text_embeds=e, text_mask=m) for e, m in prompts]
        ref_null = unet_forward(sd, kw, x, t, text_embeds=te, text_mask=prompts[0][1], cond_drop_prob=1.0)
        neg = fc.NEGATIVE
        ref_neg = unet_forward(sd, kw, x, t, text_embeds=neg[0].expand(B, -1, -1), text_mask=neg[1].expand(B, -1))

    def rows(n_rows, **cond):
        eng = unet.engine(n_rows, B, size, dev)
        keep = torch.ones(n_rows, dtype=torch.bool)
        keep[n_rows - B:] = False
        eng.set_conditioning(text_embeds=te.to(dev), text_mask=prompts[0][1].to(dev), keep=keep, lowres_noise_times=None, **cond)
        return eng.forward(x.to(dev), t.to(dev)).float().cpu().reshape(n_rows, 3, size, size).clone()

    pair = rows(2 * B)
    o_c, o_n = nerr(pair[:B], refs[0]), nerr(pair[B:], ref_null)
    bar = 1.5 * max(o_c, o_n)
    on_dev = [(e.to(dev), None if m is None else m.to(dev)) for e, m in extra]
    out = rows((K + 1) * B, extra_prompts=on_dev)
    errs = [nerr(out[k * B:(k + 1) * B], refs[k]) for k in range(K)] + [nerr(out[K * B:], ref_null)]
    outn = rows((K + 1) * B, extra_prompts=on_dev, negative_text_embeds=neg[0].to(dev), negative_text_mask=neg[1].to(dev))
    errs_n = [nerr(outn[k * B:(k + 1) * B], refs[k]) for k in range(K)] + [nerr(outn[K * B:], ref_neg)]
    print(f"K = {K}: ordinary pair cond {o_c:.3e} null {o_n:.3e}, bar {bar:.3e}; branch rows {errs}; with a negative prompt {errs_n}")
    record_parity(f"compose_forward[K{K}]", ordinary_cond=o_c, ordinary_null=o_n, bar=bar, branches=max(errs[:-1]), null=errs[-1], negative=errs_n[-1])
    assert max(errs + errs_n) < bar, (errs, errs_n, bar)
    assert min(nerr(refs[k], ref_null) for k in range(K)) > 10 * bar, "the prompts must move the rows for this test to say anything"


def test_lanes_and_pipelined():
    """Two lanes from two threads == the same calls in turn; sample_pipelined with compose as a per-batch key == each batch's own call."""
    dev = gpu_device()
    g = fs.cascade_fixture()
    model = fs.cascade_model(dev)
    te = g["text_embeds"].to(dev)
    common = dict(cond_scale=fc.COND_SCALE, sampler="dpmpp_2m", sample_steps=4, use_tqdm=False)
    comps = [fc.to_device(dict(compose=[dict(text_embeds=fc.prompt(71, scale=4.0), weight=torch.tensor([20.0, -4.0]), mask=fc.half_mask("left", batch=2))]), dev),
             fc.to_device(dict(compose=[dict(text_embeds=fc.prompt(72, batch=1, scale=4.0), weight=(10.0, 20.0))]), dev)]
    calls = [dict(text_embeds=te, seed=31, **comps[0]), dict(text_embeds=te * 0.9, seed=32, **comps[1])]
    seq = [model.sample(**common, **c) for c in calls]
    plain = model.sample(**common, text_embeds=te, seed=31)
    assert nerr(seq[0], plain) > 2 * BAR
    got = [None, None]

    def work(i):
        with model.lane(i + 1), torch.cuda.device(dev):
            got[i] = model.sample(**common, **calls[i])
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert all(o is not None and torch.equal(o, s) for o, s in zip(got, seq)), "lanes != sequential"
    pipe = model.sample_pipelined(calls, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)), "sample_pipelined != own calls"
