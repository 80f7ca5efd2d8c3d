"""CPU: the few-step solvers of Imagen.sample — sampler='dpmpp_2m' (DPM-Solver++ 2M, data prediction) and 'ddim' (its first-order
case, 0 <= eta <= 1) on the continuous-time schedules of a DDPM-trained cascade.  No kernel is new: a solver step is the
denoiser plan, CFG_X0, QUANTILE and one or two LINCOMB launches.

  1. tables: GaussianDiffusionContinuousTimes.solver_coefficients against the issue's formulas restated literally in 60-digit decimal
     arithmetic (tests/fixtures_solver.py), both schedules, steps 2 / 5 / 32, to 1e-6 relative (fp32 storage); measured <= 5.7e-8;
  2. anchor, algebraic: 'ddim' at eta = 1 on the training grid IS the reference's ancestral posterior (ip.py:252-270, 2160-2164): its rows
     equal alpha_n (1 - c) / alpha, alpha_n c and sqrt(sigma_n^2 c) evaluated exactly from step_coefficients()'s own log-SNR column, the
     final row (nonzero = 0) included, to 1e-6 relative; measured <= 6e-8;
  3. order of convergence on an analytic denoiser, independent of the driver (figures in the test's docstring);
  4. the real driver through the plan interpreter against a plain fp32 loop over the oracle's guided forward; the bar is the 2e-2 of
     tests/test_sample_cpu_replay.py::test_cascade_sample_driver.  Measured (stage 1 / stage 2 of the cascade): dpmpp_2m 7.4e-4 / 4.0e-4,
     ddim 6.8e-4 / 3.7e-4; one self_cond stage 1.04e-3, one Unet3D stage 1.45e-3, 16 x 24 8.4e-4;
  5. anchor, end to end: sample(sampler='ddim', eta=1, sample_steps=T) with the recorded draws of the reference's DDPM run injected
     reproduces that run (tests/golden/sample_tiny_cascade.pt) under the same 2e-2; measured 9.2e-4 / 4.8e-4; no DDPM_UPDATE is launched;
  6. no regression: ABI 15, the default call's launch lists are the parent commit's (tests/golden/solver_parent_launch_list_abi15.json);
  7. driver properties: refusals before any launch, the stage cache, the per-request time table, skip_steps / init_images,
     start_at_unet_number, sample_pipelined and sample_requests.

On the commit before the solvers every test that passes `sampler=` fails with `TypeError: ... unexpected keyword argument`, and sections
1 - 3 with `AttributeError: ... solver_coefficients`; the launch-list test passes on both."""
import functools
import json
import os
import sys
from decimal import Decimal

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_solver as fs  # noqa: E402
from fixtures_solver import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401

BAR = 2e-2     # tests/test_sample_cpu_replay.py: the DDPM replay of the same fixture cascade


def _sched(schedule, timesteps=1000):
    from imagen_pytorch_amd.schedules import GaussianDiffusionContinuousTimes

    return GaussianDiffusionContinuousTimes(noise_schedule=schedule, timesteps=timesteps)


def _rel(got, want):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    return float(torch.where(want != 0, (got - want).abs() / want.abs().clamp(min=1e-300), (got - want).abs()).max())


# ------------------------------------------------------------------------------------------------ 1. tables

@pytest.mark.parametrize("steps", [2, 5, 32])
@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m", 0.0)])
@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_tables_against_the_restated_formulas(schedule, sampler, eta, steps):
    sched = _sched(schedule)
    rows = fs.restated_rows(schedule, sampler, steps, eta)
    for philox in (True, False):
        step, w = sched.solver_coefficients(sampler, steps, eta, philox=philox)
        assert step.dtype == w.dtype == torch.float32 and tuple(step.shape) == tuple(w.shape) == (steps, 8)
        e_step = _rel(step[:, :7], [[r.alpha, r.sigma, r.alpha_next, r.sigma_next, r.c, r.nonzero, r.log_snr] for r in rows])
        noise_col, other = (4, 2) if philox else (2, 4)
        e_w = _rel(w[:, [0, 1, 3, noise_col]], [[r.on_x, r.on_x0, r.on_prev, r.on_noise] for r in rows])
        print(f"{schedule} {sampler} eta {eta} steps {steps}: step table {e_step:.2e}, weights {e_w:.2e}")
        assert e_step < 1e-6 and e_w < 1e-6
        assert not w[:, [other, 5, 6, 7]].any() and not step[:, 7].any()
    if sampler == "dpmpp_2m":      # first order on the first and the last row, second order between
        w = sched.solver_coefficients(sampler, steps)[1]
        assert w[0, 3] == 0 and w[-1, 3] == 0 and (steps < 3 or bool((w[1:-1, 3] != 0).all()))


def test_first_row_of_a_run_is_first_order():
    """skip_steps starts a dpmpp_2m run at row `start`: that row has no history and is the first-order one; the others are unchanged."""
    sched = _sched("cosine")
    full, part = sched.solver_coefficients("dpmpp_2m", 6)[1], sched.solver_coefficients("dpmpp_2m", 6, start=2)[1]
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(full[keep], part[keep]) and part[2, 3] == 0 and full[2, 3] != 0
    rows = fs.restated_rows("cosine", "dpmpp_2m", 6, start=2)
    assert _rel(part[:, [0, 1, 3]], [[r.on_x, r.on_x0, r.on_prev] for r in rows]) < 1e-6


def test_table_refusals():
    sched = _sched("cosine")
    for args in (("euler", 4), ("dpmpp_2m", 1), ("ddim", 0), ("ddim", 4, 1.5), ("ddim", 4, -0.1), ("dpmpp_2m", 4, 0.5)):
        with pytest.raises(ValueError):
            sched.solver_coefficients(*args)
    assert sched.solver_coefficients("ddim", 1)[0].shape == (1, 8)


# ------------------------------------------------------------------------------------------------ 2. anchor, algebraic

@pytest.mark.parametrize("timesteps", [3, 50, 1000])
@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_ddim_eta_1_on_the_training_grid_is_the_ancestral_posterior(schedule, timesteps):
    sched = _sched(schedule, timesteps)
    table = sched.step_coefficients()
    step, w = sched.solver_coefficients("ddim", timesteps, eta=1.0)
    # the reference's posterior from the table's own log-SNR column, exactly (decimal): mean = alpha_n ((1 - c) / alpha x + c x0),
    # std = sqrt(sigma_n^2 c), times nonzero
    ls = [Decimal(float(v)) for v in table[:, 6]] + [Decimal(float(sched.log_snr(torch.tensor(0.0))))]
    one = Decimal(1)
    sig = lambda v: one / (one + (-v).exp())
    want = []
    for i in range(timesteps):
        l, ln = ls[i], ls[i + 1]
        a, an, sn = sig(l).sqrt(), sig(ln).sqrt(), sig(-ln).sqrt()
        c = one - (l - ln).exp()
        want.append([float(an * (one - c) / a), float(an * c), float((sn * sn * c).sqrt()) * float(table[i, 5])])
    err = _rel(w[:, [0, 1, 4]], want)
    print(f"{schedule} T = {timesteps}: ddim(eta = 1) rows vs the posterior of step_coefficients(): {err:.2e}")
    assert err < 1e-6
    assert table[-1, 5] == 0 and w[-1, 4] == 0 and bool((w[:-1, 4] > 0).all())
    # and the table CFG_X0 / the time embedding read is step_coefficients()'s, to fp32 rounding of its own fp32 evaluation
    assert torch.equal(step[:, 6], table[:, 6]) and torch.equal(step[:, 5], table[:, 5])
    assert _rel(step[:, :5], table[:, :5].double()) < 2e-6


# ------------------------------------------------------------------------------------------------ 3. order of convergence

def _analytic_error(schedule, sampler, S, v=0.04):
    """|x_0 - exact| of the product's tables applied by LINCOMB's documented formula (fp64, thr_mode 2) to the linear ODE of Gaussian
    data N(0, v I): x0 = alpha v / (alpha^2 v + sigma^2) x_t, solved by x_t = x_1 sqrt((alpha_t^2 v + sigma_t^2) / (alpha_1^2 v + sigma_1^2))."""
    step, w = (t.double() for t in _sched(schedule).solver_coefficients(sampler, S))
    x1 = torch.linspace(-1.0, 1.0, 9, dtype=torch.float64)
    x, prev = x1.clone(), torch.zeros_like(x1)
    for i in range(S):
        a, s = step[i, 0], step[i, 1]
        x0 = a * v / (a * a * v + s * s) * x
        thr = x0.clamp(-1.0, 1.0)
        assert torch.equal(thr, x0), "the clamp must never bind in this test"
        x, prev = w[i, 0] * x + w[i, 1] * thr + w[i, 3] * prev, thr    # out = w0 t0 + w1 thr(t1) + w3 thr(t3)
    a1, s1, a0, s0 = step[0, 0], step[0, 1], step[-1, 2], step[-1, 3]
    exact = x1 * torch.sqrt((a0 * a0 * v + s0 * s0) / (a1 * a1 * v + s1 * s1))
    return float((x - exact).abs().max())


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_order_of_convergence_on_an_analytic_denoiser(schedule):
    """Measured max |error| at t = 0 over x_1 in [-1, 1], v = 0.04:
        cosine  S = 16 / 32 / 64   ddim 3.40e-2 / 1.76e-2 / 9.00e-3 (ratios 1.93, 1.96)   dpmpp_2m 1.95e-2 / 2.99e-3 / 3.89e-4 (6.51, 7.68)
        linear  S = 16 / 32 / 64   ddim 6.25e-2 / 3.29e-2 / 1.71e-2 (ratios 1.90, 1.93)   dpmpp_2m 5.46e-2 / 1.63e-2 / 1.30e-4 (3.34, 125)
    2M's ratios at these S are NOT the asymptotic ones: its signed error changes sign between S = 64 and 128 (the first-order first and
    last steps against the second-order interior), so it falls faster than 4x per doubling before that and the pairs 16 -> 32 and
    32 -> 64 are both pre-asymptotic.  The assertion the issue asks for is made on 32 -> 64; the asymptotic regime is asserted too, on
    512 -> 1024, where the ratio is that of a second-order method: cosine 3.71, linear 4.05 (ddim there: 2.00 / 1.99)."""
    S = (16, 32, 64)
    ddim = [_analytic_error(schedule, "ddim", s) for s in S]
    two = [_analytic_error(schedule, "dpmpp_2m", s) for s in S]
    r1 = [ddim[i] / ddim[i + 1] for i in range(2)]
    r2 = [two[i] / two[i + 1] for i in range(2)]
    print(f"{schedule}: ddim {ddim} ratios {r1}; dpmpp_2m {two} ratios {r2}")
    assert all(b < a for a, b in zip(ddim, two)), "2M must beat DDIM at every S"
    assert all(1.7 < r < 2.3 for r in r1), r1
    assert r2[1] >= 3.0, r2
    far1 = _analytic_error(schedule, "ddim", 512) / _analytic_error(schedule, "ddim", 1024)
    far2 = _analytic_error(schedule, "dpmpp_2m", 512) / _analytic_error(schedule, "dpmpp_2m", 1024)
    print(f"{schedule}: 512 -> 1024 ddim {far1:.2f}, dpmpp_2m {far2:.2f}")
    assert 1.9 < far1 < 2.1 and 3.0 <= far2 < 5.0, (far1, far2)


# ------------------------------------------------------------------------------------------------ 4. the driver through the interpreter

def _common(g, noise, **kw):
    return dict(text_embeds=g["text_embeds"], cond_scale=fs.COND_SCALE, use_tqdm=False, noise_fn=noise, device="cpu", **kw)


@pytest.mark.parametrize("sampler", ["dpmpp_2m", "ddim"])
def test_solver_cascade_through_the_interpreter(cpu_backend, sampler):
    """The tiny cascade (16^2 -> 32^2, low-res conditioning, CFG 3) at 6 solver steps through the real driver, graph path and eager,
    against the restatement — recomputed here and equal to the recorded one the GPU tests read.  Measured, stage 1 / stage 2:
    dpmpp_2m 7.4e-4 / 4.0e-4, ddim 6.8e-4 / 3.7e-4 (bar 2e-2)."""
    g, run = fs.cascade_fixture(), fs.runs_fixture()["runs"][f"cascade.{sampler}"]
    noise = fs.fixed_noise(run["noise"])
    want = fs.solver_sample(fs.cascade_specs(), g["image_sizes"], g["text_embeds"], sampler=sampler, steps=fs.STEPS, noise_fn=noise, return_all=True)
    assert all(torch.allclose(a, b, atol=1e-5) for a, b in zip(want, run["outputs"])), "tests/golden/solver_runs.pt is stale"
    model = fs.cascade_model()
    outs = model.sample(sampler=sampler, sample_steps=fs.STEPS, return_all_unet_outputs=True, **_common(g, noise))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"{sampler} at {fs.STEPS} steps vs the restatement: {errs}")
    assert max(errs) < BAR, errs
    eager = model.sample(sampler=sampler, sample_steps=fs.STEPS, return_all_unet_outputs=True, use_graph=False, **_common(g, noise))
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    kinds = {int(k) for st in model._stages.values() for k, _, _ in st["plan"].ops}
    from imagen_pytorch_amd import ops
    assert ops.ENUMS["IMAGEN_OP_DDPM_UPDATE"] not in kinds and ops.ENUMS["IMAGEN_OP_LINCOMB"] in kinds
    labels = [l for st in model._stages.values() for _, _, l in st["plan"].ops if l.startswith(sampler)]
    assert labels == ([f"{sampler}.update", f"{sampler}.history"] * 2 if sampler == "dpmpp_2m" else [f"{sampler}.update"] * 2)
    # the two solvers are different samplers: the other one's restatement is far
    other = fs.runs_fixture()["runs"]["cascade.ddim" if sampler == "dpmpp_2m" else "cascade.dpmpp_2m"]
    assert run["noise"].keys() == other["noise"].keys()


@pytest.mark.parametrize("tag", ["selfcond", "video", "rect"])
def test_solver_variants_through_the_interpreter(cpu_backend, tag):
    """dpmpp_2m at 4 steps on one Unet(self_cond=True) stage (its next input is the thr1_out of the step), one Unet3D stage and the
    cascade's first unet at 16 x 24 (image_shapes), against the recorded restatement.  Measured 1.04e-3 / 1.45e-3 / 8.4e-4 (bar 2e-2)."""
    run = fs.runs_fixture()["runs"][f"{tag}.dpmpp_2m"]
    noise = fs.fixed_noise(run["noise"])
    g = fs.cascade_fixture()
    kw = {}
    if tag == "selfcond":
        model = fs.single_stage_model(fs.selfcond_spec(), 16)
    elif tag == "video":
        v = fs.load("sample_tiny_video.pt")
        model, g, kw = fs.video_model(), v, dict(video_frames=v["frames"])
    else:
        model, kw = fs.single_stage_model(fs.cascade_specs()[0], 16), dict(image_shapes=((16, 24),))
    out = model.sample(sampler="dpmpp_2m", sample_steps=4, **_common(g, noise, **kw))
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    err = nerr(out, run["outputs"][0])
    print(f"dpmpp_2m, {tag}: {err:.2e}")
    assert err < BAR
    assert torch.equal(out, model.sample(sampler="dpmpp_2m", sample_steps=4, **_common(g, noise, **kw))), "history / self_cond buffers are reset per call"


# ------------------------------------------------------------------------------------------------ 5. anchor, end to end

def test_ddim_eta_1_reproduces_the_references_ddpm_run(cpu_backend):
    """sample(sampler='ddim', eta=1, sample_steps=T) with the draws of the reference's recorded DDPM run injected (the step draw as
    LINCOMB's t2) against that run: the bar of its DDPM replay, 2e-2.  Measured 9.2e-4 / 4.8e-4 (the DDPM replay itself: 9.4e-4 / 4.8e-4)."""
    from imagen_pytorch_amd import ops

    g = fs.cascade_fixture()
    model = fs.cascade_model()
    T = g["timesteps"]
    kw = dict(text_embeds=g["text_embeds"], cond_scale=g["cond_scale"], use_tqdm=False, return_all_unet_outputs=True,
              noise_fn=lambda tag, shape: g["noise"][tag], device="cpu")
    outs = model.sample(sampler="ddim", eta=1.0, sample_steps=T, **kw)
    errs = [nerr(o, r) for o, r in zip(outs, g["outputs"])]
    plans = [st["plan"] for st in model._stages.values()]
    assert len(plans) == 2 and all(ops.ENUMS["IMAGEN_OP_DDPM_UPDATE"] not in {int(k) for k, _, _ in p.ops} for p in plans)
    ddpm = model.sample(**kw)
    errs_ddpm = [nerr(o, r) for o, r in zip(ddpm, g["outputs"])]
    print(f"ddim(eta = 1, T = {T}) vs the reference's DDPM run: {errs}; the DDPM replay itself: {errs_ddpm}")
    assert max(errs) < BAR, errs
    # sample_steps=None under a solver means the unet's timesteps
    assert all(torch.equal(a, b) for a, b in zip(outs, model.sample(sampler="ddim", eta=1.0, **kw)))


# ------------------------------------------------------------------------------------------------ 6. no regression

def test_default_call_launch_lists_are_the_parent_commits(monkeypatch):
    from imagen_pytorch_amd import _abi, engine

    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))
    assert _abi.ENUMS["IMAGEN_ABI_VERSION"] == 15, "no ABI change: the solver update is LINCOMB"
    want = json.load(open(os.path.join(fs.GOLDEN, "solver_parent_launch_list_abi15.json")))
    got = fs.launch_lists()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


# ------------------------------------------------------------------------------------------------ 7. driver properties

@pytest.fixture()
def no_launch(cpu_backend, monkeypatch):
    """cpu_backend in which running any plan is an error: what is refused must be refused before the first launch."""
    from imagen_pytorch_amd import ops

    def launched(self, stream=None):
        raise AssertionError(f"plan '{self.name}' was launched")
    monkeypatch.setattr(ops.Plan, "run", launched)


def test_refusals_come_before_any_launch(no_launch):
    from imagen_pytorch_amd import ElucidatedImagen, Unet
    from imagen_pytorch_amd.distributed import sample_sharded

    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False)
    te = g["text_embeds"]
    base = dict(text_embeds=te, cond_scale=3.0, use_tqdm=False, device="cpu")
    known, keep = torch.rand(2, 3, 32, 32), torch.rand(2, 32, 32) > 0.5
    for kw in (dict(sampler="euler"), dict(sampler="dpmpp_2m", eta=0.5), dict(sampler="ddim", eta=1.5), dict(sampler="ddim", eta=-0.1),
               dict(sampler="dpmpp_2m", inpaint_images=known, inpaint_masks=keep), dict(sampler="ddim", inpaint_images=known, inpaint_masks=keep),
               dict(sample_steps=8), dict(eta=0.5), dict(sampler="ddpm", sample_steps=8), dict(sampler="ddpm", eta=1.0),
               dict(sampler="dpmpp_2m", sample_steps=1), dict(sampler="dpmpp_2m", sample_steps=(6, 1)), dict(sampler="ddim", sample_steps=0),
               dict(sampler="ddim", sample_steps=(4, 4, 4))):
        with pytest.raises(ValueError):
            model.sample(**base, **kw)
        with pytest.raises(ValueError):
            model.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", **kw)
        with pytest.raises(ValueError):
            sample_sharded(model.sample, te, cond_scale=3.0, use_tqdm=False, device="cpu", **kw)
    with pytest.raises(ValueError, match="eta"):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", sampler="ddim", eta=0.5)
    with pytest.raises(ValueError):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", sampler="euler")
    from oracle.make_golden import ELUCIDATED_HP
    edm = ElucidatedImagen([Unet(**u["kwargs"]).eval() for u in g["unets"]], image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1,
                           **ELUCIDATED_HP)
    for kw in (dict(sampler="dpmpp_2m"), dict(sampler="ddpm"), dict(sample_steps=8), dict(eta=0.0)):
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            edm.sample(**base, **kw)
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            edm.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", **kw)
    assert not model._stages and not edm._stages


def test_stage_cache_and_time_table(cpu_backend):
    """The stage key includes (sampler, steps, eta): different sample_steps build different stages, a repeated call reuses its own; the
    default call's stages are untouched.  The per-request time table has `steps` rows, not num_timesteps."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(5)
    kw = _common(g, noise, stop_at_unet_number=1)
    a = model.sample(sampler="dpmpp_2m", sample_steps=4, **kw)
    assert len(model._stages) == 1
    b = model.sample(sampler="dpmpp_2m", sample_steps=5, **kw)
    assert len(model._stages) == 2 and not torch.equal(a, b)
    ids = {k: id(v) for k, v in model._stages.items()}
    assert torch.equal(a, model.sample(sampler="dpmpp_2m", sample_steps=4, **kw))
    assert {k: id(v) for k, v in model._stages.items()} == ids
    model.sample(sampler="ddim", sample_steps=4, **kw)
    model.sample(sampler="ddim", sample_steps=4, eta=0.5, **kw)
    model.sample(**kw)
    assert len(model._stages) == 5
    for key, st in model._stages.items():
        solver = key[-1]
        steps = g["timesteps"] if solver is None else solver[1]
        assert st["T"] == steps and tuple(st["coef"].shape) == (steps, 8)
        eng = st["eng"]
        assert eng._tt_plan is not None, "the tiny stage fits the time table"
        assert eng.time_table_layout["chunks"] * eng.time_table_layout["steps_per_chunk"] >= steps
        rows = [seg for seg in eng._tt_plan.keep if torch.is_tensor(seg) and seg.ndim == 1 and seg.numel() == steps * eng.R]
        assert rows, "the table's log-SNR column has steps x rows entries"


def test_skip_steps_init_images_and_start_at_unet(cpu_backend):
    """init_images / skip_steps count solver steps (the run's first row is first order), and stage 2 alone from stage 1's image equals
    stage 2 of the whole cascade."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(7)
    init = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(8))
    kw = dict(sampler="dpmpp_2m", sample_steps=5)
    want = fs.solver_sample(fs.cascade_specs(), g["image_sizes"], g["text_embeds"], steps=5, sampler="dpmpp_2m", noise_fn=noise, return_all=True,
                            init_images=(init, None), skip_steps=(2, None))
    outs = model.sample(init_images=(init, None), skip_steps=(2, None), return_all_unet_outputs=True, **kw, **_common(g, noise))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"dpmpp_2m, init_images + skip_steps = 2 of 5: {errs}")
    assert max(errs) < BAR
    plain = model.sample(return_all_unet_outputs=True, **kw, **_common(g, noise))       # the same cached stage, back at row 0
    assert nerr(plain[0], outs[0]) > 10 * BAR
    want_plain = fs.solver_sample(fs.cascade_specs(), g["image_sizes"], g["text_embeds"], steps=5, sampler="dpmpp_2m", noise_fn=noise, return_all=True)
    assert max(nerr(o, w) for o, w in zip(plain, want_plain)) < BAR
    alone = model.sample(start_at_unet_number=2, start_image_or_video=plain[0], **kw, **_common(g, noise))
    assert torch.equal(alone, plain[1])
    short = model.sample(max_steps=3, stop_at_unet_number=1, **kw, **_common(g, noise))
    assert tuple(short.shape) == tuple(plain[0].shape) and not torch.equal(short, plain[0])


def test_pipelined_lanes_and_merged_requests(cpu_backend):
    """sample_pipelined is bit-identical to sample; a lane gives the same images; sample_requests under dpmpp_2m (the deterministic
    solvers draw nothing after the initial image, which carries each request's key) equals each request's own call."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    te = g["text_embeds"]
    fns = [fs.memo_noise(11), fs.memo_noise(12)]
    common = dict(cond_scale=fs.COND_SCALE, device="cpu", sampler="dpmpp_2m", sample_steps=4)
    batches = [dict(text_embeds=te * s, noise_fn=fn) for s, fn in zip((1.0, 0.9), fns)]
    seq = [model.sample(use_tqdm=False, **common, **b) for b in batches]
    pipe = model.sample_pipelined(batches, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(pipe[0], pipe[1])
    with model.lane(3):
        assert torch.equal(model.sample(use_tqdm=False, **common, **batches[0]), seq[0])
    reqs = [dict(text_embeds=te[:1], seed=21), dict(text_embeds=te, seed=22)]
    merged = model.sample_requests(reqs, **common)
    own = [model.sample(use_tqdm=False, **common, **r) for r in reqs]
    errs = [nerr(a, b) for a, b in zip(merged, own)]
    print(f"merged requests under dpmpp_2m vs their own calls (interpreter): {errs}")
    assert [tuple(m.shape) for m in merged] == [tuple(o.shape) for o in own] and max(errs) < 2e-3
