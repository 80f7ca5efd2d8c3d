"""MI355X: guidance schedules of Imagen.sample (guidance_schedule= / guidance_interval=) on the HIP path.  The one kernel
change is CFG_X0's cfg == 2, which reads the guidance scale from column 7 of the step's table row; an interval's unguided steps replay the
B-row plan of a sibling stage on the same sampler state.

Bars are those of the existing tests of the same kind: 1e-6 normwise against fp64 for CFG_X0 (tests/test_sampler_kernels_gpu.py, every
objective at cfg == 1), 2e-2 for a sampled stage against its restatement (tests/test_solver_gpu.py, tests/test_model_gpu.py); everything
that is the same arithmetic on the same inputs is bit-equal.  The restatement is tests/fixtures_guidance.py, recorded in
tests/golden/guidance_runs.pt; tests/golden/guidance_cfg_x0_parent.pt holds what the parent commit's kernel library gave on an MI355X
(tools/make_guidance_golden.py --kernel).  Every test prints its figures before it asserts and records them through
conftest.record_parity (profiles/guidance_parity_mi355x.json)."""
import os
import sys

import pytest
import torch

from conftest import EMULATED, gpu_device, record_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import fixtures_guidance as fg  # noqa: E402
import fixtures_solver as fs  # noqa: E402
import make_guidance_golden as mg  # noqa: E402
from fixtures_guidance import nerr  # noqa: E402
from plan_interp_guidance import cfg_x0_contract  # noqa: E402

pytestmark = pytest.mark.gpu

BAR, TOL = 2e-2, 1e-6
SCALES = (0.0, 1.0, 3.0, 7.5, -1.0)
DECOY = 123.0           # the immediate cond_scale of every cfg == 2 launch: it must not be read


def _nerr64(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).norm() / ref.norm().clamp(min=1e-300)).item()


def _table(steps):
    """A real cosine step table with the scales in column 7, cycled so that steps 0 / middle / last meet different ones."""
    from imagen_pytorch_amd.schedules import GaussianDiffusionContinuousTimes

    coef = GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=steps).step_coefficients()
    coef[:, 7] = torch.tensor([SCALES[i % len(SCALES)] for i in range(steps)])
    return coef


@pytest.mark.parametrize("objective", ["noise", "x_start", "v"])
def test_cfg_x0_scale_from_the_table_row(objective):
    """cfg == 2 against fp64, per element: the three objectives, steps 0 / middle / last of a 5-row table and, at each of them, every
    scale of {0, 1, 3, 7.5, -1} in column 7, the immediate set to a decoy.  2 x 1540 elements: several blocks, the last one partial."""
    dev = gpu_device()
    inp = mg.kernel_inputs()
    steps, worst = inp["steps"], 0.0
    for step in (0, steps // 2, steps - 1):
        for shift in range(len(SCALES)):
            coef = _table(steps)
            coef[:, 7] = coef[:, 7].roll(shift)
            x0, ab = mg.run_cfg_x0(inp, cfg=2, objective=objective, cond_scale=DECOY, step=step, coef=coef, device=dev)
            ref = cfg_x0_contract(inp["x"].reshape(-1), inp["pred"].reshape(-1), coef[step], cfg=2, cond_scale=DECOY,
                                  objective={"noise": 0, "x_start": 1, "v": 2}[objective], dtype=torch.float64)
            e = _nerr64(x0.reshape(-1), ref)
            worst = max(worst, e)
            assert e <= TOL, (objective, step, float(coef[step, 7]), e)
            # per element: at most five fp32 roundings (cond - nul, the guidance combine, sigma * eps, the difference, the quotient), each
            # of relative size u = 2^-24 on an intermediate no larger than M, the same expression over absolute values: |err| <= 6 u M
            n = inp["x"].numel()
            c, nu, xa = inp["pred"].reshape(-1)[:n].double().abs(), inp["pred"].reshape(-1)[n:].double().abs(), inp["x"].reshape(-1).double().abs()
            a, sg, s = float(coef[step, 0]), float(coef[step, 1]), abs(float(coef[step, 7]))
            m_eps = nu + s * (c + nu)
            M = {"noise": (xa + sg * m_eps) / max(a, 1e-8), "x_start": m_eps, "v": a * xa + sg * m_eps}[objective]
            assert bool(((x0.reshape(-1).double() - ref).abs() <= 6 * 2.0 ** -24 * M).all()), (objective, step, s)
            assert torch.equal(ab, x0.abs()), "absx0 must be |x0| bit for bit"
    print(f"cfg_x0 cfg == 2 [{objective}]: worst normwise error vs fp64 {worst:.2e}")
    record_parity(f"guidance_cfg_x0[{objective}]", worst=worst)


@pytest.mark.parametrize("objective", ["noise", "x_start", "v"])
def test_cfg_x0_constant_column_is_the_immediate(objective):
    """cfg == 2 with s in column 7 is bit-equal to cfg == 1 with the immediate s: one expression serves both."""
    dev = gpu_device()
    inp = mg.kernel_inputs()
    for s in SCALES + (2.3,):
        coef = _table(inp["steps"])
        coef[:, 7] = s
        for step in (0, inp["steps"] - 1):
            a = mg.run_cfg_x0(inp, cfg=2, objective=objective, cond_scale=DECOY, step=step, coef=coef, device=dev)
            b = mg.run_cfg_x0(inp, cfg=1, objective=objective, cond_scale=s, step=step, coef=coef, device=dev)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (objective, s, step)


def test_cfg_0_and_1_give_the_parent_commits_bits():
    """cfg == 0 and cfg == 1 on the inputs of tools/make_guidance_golden.py --kernel: the bits the parent commit's library gave on MI355X."""
    if EMULATED:
        pytest.skip("the recorded bits are the GPU's; the host compiler of the emulation may contract differently")
    rec = fs.load("guidance_cfg_x0_parent.pt")["outputs"]
    inp = mg.kernel_inputs()
    for (objective, cfg), (x0, ab) in rec.items():
        got = mg.run_cfg_x0(inp, cfg=cfg, objective=objective, cond_scale=inp["cond_scale"], step=inp["step"], device=gpu_device())
        assert torch.equal(got[0], x0) and torch.equal(got[1], ab), (objective, cfg)


@pytest.fixture(scope="module")
def cascade():
    return fs.cascade_model(gpu_device())


def _common(te, noise, dev, **kw):
    return dict(text_embeds=te.to(dev), cond_scale=fg.COND_SCALE, use_tqdm=False, noise_fn=noise, **kw)


def test_constant_schedule_equals_the_scalar_call(cascade):
    dev = gpu_device()
    g = fs.cascade_fixture()
    kw = _common(g["text_embeds"], fs.memo_noise(3, dev), dev, return_all_unet_outputs=True)
    want = cascade.sample(**kw)
    n = len(cascade._stages)
    for extra in (dict(guidance_schedule=lambda t: fg.COND_SCALE), dict(guidance_interval=(0.0, 1.0)), dict(guidance_schedule=[fg.COND_SCALE] * g["timesteps"])):
        assert all(torch.equal(a, b) for a, b in zip(cascade.sample(**kw, **extra), want))
    assert len(cascade._stages) == n, "a constant schedule builds no stage of its own"


@pytest.mark.parametrize("which", ["ramp", "interval"])
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m", "ddim"])
def test_scheduled_samples_vs_restatement(sampler, which):
    """The tiny cascade with a ramp / an interval on both stages against the recorded restatement, bar 2e-2; hipGraph replay == eager
    launches bit for bit; a second call on the cached stages == the first.  The constant-scale twin is printed beside it."""
    dev = gpu_device()
    g = fs.cascade_fixture()
    grp = fg.runs_fixture()["groups"][f"cascade.{sampler}"]
    steps, want = grp["steps"], grp["runs"][which]
    model = fs.cascade_model(dev, timesteps=steps) if sampler == "ddpm" else fs.cascade_model(dev)
    solver = {} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=steps)
    kw = _common(g["text_embeds"], fs.fixed_noise(grp["noise"], dev), dev, return_all_unet_outputs=True, **solver)
    outs = model.sample(**kw, **fg.schedule_kwargs(which))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    twin = [nerr(o, w) for o, w in zip(model.sample(**kw), grp["twin"])]
    print(f"{sampler}, {which} at {steps} steps vs the restatement: stage 1 {errs[0]:.2e}, stage 2 {errs[1]:.2e}; "
          f"the constant-scale call vs its restatement: {twin[0]:.2e}, {twin[1]:.2e}")
    record_parity(f"guidance_sample[{sampler}-{which}]", stage1=errs[0], stage2=errs[1], twin_stage1=twin[0], twin_stage2=twin[1])
    assert max(errs) < BAR, errs
    eager = model.sample(use_graph=False, **kw, **fg.schedule_kwargs(which))
    assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "graph replay != eager"
    again = model.sample(**kw, **fg.schedule_kwargs(which))
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "second sample() on the cached stages differs"
    if which == "interval":
        assert sum(st["sibling"] is not None for st in model._stages.values()) == 2


@pytest.mark.parametrize("tag", ["selfcond.ddpm.steep", "selfcond.ddpm.interval", "selfcond.dpmpp_2m.switch", "video.ddpm.interval", "rect.dpmpp_2m.interval"])
def test_scheduled_variants_vs_restatement(tag):
    """A Unet(self_cond=True) stage, one Unet3D stage and the cascade's first unet at 16 x 24 with schedules that switch plans."""
    dev = gpu_device()
    name, sampler, which = tag.split(".")
    grp = fg.runs_fixture()["groups"][f"{name}.{sampler}"]
    want, steps = grp["runs"][which][0], grp["steps"]
    te, kw = fs.cascade_fixture()["text_embeds"], {}
    if name == "selfcond":
        model = fs.single_stage_model(fs.selfcond_spec(), 16, dev, timesteps=steps)
    elif name == "video":
        v = fs.load("sample_tiny_video.pt")
        model, te, kw = fs.video_model(dev, timesteps=steps), v["text_embeds"], dict(video_frames=v["frames"])
    else:
        model, kw = fs.single_stage_model(fs.cascade_specs()[0], 16, dev, timesteps=steps), dict(image_shapes=((16, 24),))
    kw.update(fg.schedule_kwargs(which), **({} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=steps)))
    call = _common(te, fs.fixed_noise(grp["noise"], dev), dev, **kw)
    out = model.sample(**call)
    err = nerr(out, want)
    print(f"{tag}: {err:.2e}")
    record_parity(f"guidance_variant[{tag}]", err=err)
    assert tuple(out.shape) == tuple(want.shape) and err < BAR
    assert torch.equal(out, model.sample(**call))


def test_negative_prompt_with_an_interval(cascade):
    """The negative prompt sits on the null rows of the guided steps; the unguided steps have none.  Against the restatement, computed here."""
    dev = gpu_device()
    g = fs.cascade_fixture()
    te, T = g["text_embeds"], g["timesteps"]
    neg = torch.randn(1, 6, 32, generator=torch.Generator().manual_seed(5))
    noise = fs.memo_noise(13)
    scales = fg.scales_of("interval", T)
    want = fg.guided_sample(fs.cascade_specs(), g["image_sizes"], te, sampler="ddpm", steps=T, scales=[scales] * 2, noise_fn=noise,
                            negative=(neg, torch.ones(1, 6, dtype=torch.bool)))
    kw = _common(te, fs.fixed_noise(noise.draws, dev), dev, guidance_interval=fg.INTERVAL)
    out = cascade.sample(negative_text_embeds=neg.to(dev), **kw)
    err, gap = nerr(out, want), nerr(out, cascade.sample(**kw))
    print(f"negative prompt with an interval: {err:.2e} from the restatement, {gap:.2e} from the call without it")
    record_parity("guidance_negative_interval", err=err, gap=gap)
    assert err < BAR and gap > 2 * BAR
