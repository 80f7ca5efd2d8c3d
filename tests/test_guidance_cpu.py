"""CPU: guidance schedules of Imagen.sample — `guidance_schedule=` (a scale per step) and `guidance_interval=` (guidance inside a band of
noise levels, the B-row plan outside it) — on the real driver with the plan interpreter as launcher (tests/plan_interp_guidance.py, whose
CFG_X0 contract knows cfg == 2), in the style of tests/test_sample_cpu_replay.py.

  1. how the keywords resolve to one scale per step (callable, sequence, per-unet tuple, the interval's closed ends, the solver grids);
  2. a constant schedule, and a call without the keywords, build the parent commit's launch lists and cache keys; ABI 15, no new op kind;
  3. the ramp and the interval runs of the three samplers, a self_cond stage, a Unet3D stage and a 16 x 24 stage against the recorded
     restatement (tests/fixtures_guidance.py, tests/golden/guidance_runs.pt), each of which lies >= 10 bars from its constant-scale twin;
  4. an interval call launches the B-row plan on exactly the steps outside the interval;
  5. the state the two plans share, across guided -> unguided -> guided: self-conditioning, the 2M history, skip_steps / init_images;
  6. every refusal, before anything is launched;
  7. the keywords through sample_pipelined, sample_sharded and sample_requests, with a negative prompt, on a lane."""
import functools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_guidance as fg  # noqa: E402
import fixtures_solver as fs  # noqa: E402
from fixtures_guidance import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend as _replay_backend  # noqa: E402,F401

BAR = 2e-2      # the project's bar of a sampled stage against its restatement (tests/test_sample_cpu_replay.py, tests/test_solver_cpu.py)


@pytest.fixture()
def cpu_backend(_replay_backend, monkeypatch):  # noqa: F811
    """The replay backend of tests/test_sample_cpu_replay.py with the interpreter that knows cfg == 2 behind ops.Plan.run."""
    from imagen_pytorch_amd import ops
    from plan_interp_guidance import GuidanceInterpreter

    it = GuidanceInterpreter()
    monkeypatch.setattr(ops.Plan, "run", lambda self, stream=None: it.run(self))
    return it


def _common(te, noise, **kw):
    return dict(text_embeds=te, cond_scale=fg.COND_SCALE, use_tqdm=False, noise_fn=noise, device="cpu", **kw)


# ------------------------------------------------------------------------------------------------ 1. resolution

@pytest.mark.parametrize("steps", [1, 4, 5, 6, 10, 32])
def test_scales_against_the_restatement(steps):
    from imagen_pytorch_amd.schedules import guidance_scales, step_times

    assert step_times(steps) == [float(t) for t in fg.restated_times(steps)]
    seq = [0.5 * i - 1.0 for i in range(steps)]
    for sched in (None, fg.RAMP, seq):
        for interval in (None, fg.INTERVAL, (0.2, 0.8), (0.0, 1.0), (0.5, 1.0), (0.0, 0.1)):
            got = guidance_scales(steps, 3.0, sched, interval)
            assert got.dtype == torch.float32 and got.tolist() == fg.restated_scales(steps, 3.0, sched, interval), (steps, sched, interval)


def test_interval_ends_are_inside():
    from imagen_pytorch_amd.schedules import guidance_scales

    # 5 steps: t = 1, 0.8, 0.6, 0.4, 0.2.  0.8 and 0.2 are no binary fractions; a bound written as 0.2 meets the row at 1 / 5
    assert guidance_scales(5, 3.0, None, (0.2, 0.8)).tolist() == [1.0, 3.0, 3.0, 3.0, 3.0]
    assert guidance_scales(5, 3.0, None, (0.21, 0.79)).tolist() == [1.0, 1.0, 3.0, 3.0, 1.0]
    assert guidance_scales(4, 3.0, None, (0.25, 0.75)).tolist() == [1.0, 3.0, 3.0, 3.0]
    assert guidance_scales(4, 3.0, lambda t: 8.0 * t, (0.5, 1.0)).tolist() == [8.0, 6.0, 4.0, 1.0]
    assert guidance_scales(10, 2.0, None, (0.3, 0.7)).tolist() == [1.0] * 3 + [2.0] * 5 + [1.0] * 2


def test_per_unet_values_and_the_solver_grids(cpu_backend):
    """_resolve: one value serves every unet, a tuple holds one per unet (None: the stage is left alone); the vector has the stage's own
    number of denoiser evaluations — timesteps under 'ddpm', sample_steps under a solver; a constant vector becomes the stage's cond_scale."""
    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False, timesteps=(4, 5))
    resolve = lambda **kw: model._resolve(model._call(text_embeds=g["text_embeds"], device="cpu", **kw))
    c = resolve(cond_scale=3.0, guidance_schedule=fg.RAMP)
    assert [v.tolist() for v in c.guidance] == [fg.restated_scales(4, 3.0, fg.RAMP), fg.restated_scales(5, 3.0, fg.RAMP)]
    c = resolve(cond_scale=(3.0, 2.0), guidance_schedule=(None, [1.0, 2.0, 3.0, 4.0, 5.0]), guidance_interval=((0.3, 0.8), None))
    assert c.guidance[0].tolist() == [1.0, 3.0, 3.0, 1.0] and c.guidance[1].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] and c.cond_scale == (3.0, 2.0)
    c = resolve(cond_scale=3.0, guidance_interval=(None, (0.0, 0.5)), sampler="dpmpp_2m", sample_steps=(3, 6))
    assert c.guidance[0] is None and c.guidance[1].tolist() == [1.0, 1.0, 1.0, 3.0, 3.0, 3.0]
    c = resolve(cond_scale=3.0, guidance_schedule=[5.0, 4.0, 3.0, 2.0], stop_at_unet_number=1)       # one sequence, and only the stage that runs
    assert c.guidance[0].tolist() == [5.0, 4.0, 3.0, 2.0] and c.guidance[1] is None
    # constant vectors: the stage is the scalar one
    c = resolve(cond_scale=(3.0, 7.1), guidance_schedule=(lambda t: 5.0, lambda t: 7.1), guidance_interval=(0.0, 1.0))
    assert c.guidance == (None, None) and c.cond_scale == (5.0, 7.1)
    c = resolve(cond_scale=3.0, guidance_interval=(0.0, 0.01))                # nothing inside: every step unguided
    assert c.guidance == (None, None) and c.cond_scale == (1.0, 1.0)
    assert resolve(cond_scale=3.0).guidance == (None, None)
    assert not model._stages


# ------------------------------------------------------------------------------------------------ 2. no regression

def test_abi_and_default_launch_lists(monkeypatch):
    from imagen_pytorch_amd import _abi, engine
    from plan_interp import Interpreter
    from plan_interp_guidance import GuidanceInterpreter

    assert _abi.ENUMS["IMAGEN_ABI_VERSION"] == 15
    assert len(_abi.OP_STRUCT) == len(Interpreter.DISPATCH) == len(GuidanceInterpreter.DISPATCH) == 32
    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))
    want = json.load(open(os.path.join(fs.GOLDEN, "solver_parent_launch_list_abi15.json")))
    assert fs.launch_lists() == want


def test_constant_schedule_is_the_scalar_call(cpu_backend):
    """A schedule that resolves to the stage's cond_scale on every step meets the scalar call's stages: same keys, same objects, cfg = 1
    with the immediate; so does a call without the keywords.  A schedule that varies gets a key of its own that ends in its bytes."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(3)
    kw = _common(g["text_embeds"], noise)
    T = g["timesteps"]
    a = model.sample(**kw)
    keys = {k: id(v) for k, v in model._stages.items()}
    assert len(keys) == 2 and all(len(k) == 16 for k in keys), "the parent's key: 16 entries"
    for extra in (dict(guidance_schedule=lambda t: fg.COND_SCALE), dict(guidance_schedule=[fg.COND_SCALE] * T), dict(guidance_interval=(0.0, 1.0)),
                  dict(guidance_schedule=(None, lambda t: fg.COND_SCALE))):
        assert torch.equal(model.sample(**kw, **extra), a)
        assert {k: id(v) for k, v in model._stages.items()} == keys
    for st in model._stages.values():
        p = [s for k, s, l in st["plan"].ops if l == "cfg_x0"][0]
        assert p.cfg == 1 and p.cond_scale == fg.COND_SCALE and st["scales"] is None and st["sibling"] is None
        assert float(st["coef"][:, 7].abs().max()) == 0.0
    b = model.sample(**kw, guidance_schedule=fg.RAMP, stop_at_unet_number=1)
    new = [k for k in model._stages if k not in keys]
    assert len(new) == 1 and new[0][:16] == [k for k in keys if k[0] == 0][0] and new[0][16][0] == "guidance"
    st = model._stages[new[0]]
    p = [s for k, s, l in st["plan"].ops if l == "cfg_x0"][0]
    assert p.cfg == 2 and st["coef"][:, 7].tolist() == fg.restated_scales(T, fg.COND_SCALE, fg.RAMP) and st["eng"].R == 4
    assert not torch.equal(b, model.sample(**kw, stop_at_unet_number=1))
    assert [[int(k), l] for k, _, l in st["plan"].ops] == [[int(k), l] for k, _, l in model._stages[new[0][:16]]["plan"].ops], "the same launch list"


# ------------------------------------------------------------------------------------------------ 3. / 4. the recorded runs

def _plans(it, n_before=0):
    """'G' / 'U' per CFG_X0 launch since `n_before`: the guided (cfg 2, 2B rows) or the unguided (cfg 0, B rows) plan."""
    out = []
    for cfg, rows in it.launches[n_before:]:
        assert (cfg, rows) in ((2, 4), (0, 2), (1, 4)), (cfg, rows)
        out.append("U" if cfg == 0 else "G")
    return "".join(out)


@pytest.mark.parametrize("which", ["ramp", "interval"])
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m", "ddim"])
def test_cascade_runs_through_the_interpreter(cpu_backend, sampler, which):
    """The tiny cascade with a ramp / an interval on both stages, graph path and eager, against the restatement — recomputed here and equal
    to the recorded one the GPU tests read — and >= 10 bars from the constant-scale twin.  Which plan every step replayed is counted.
    Measured (stage 1 / stage 2): see the printed figures; bar 2e-2."""
    g = fs.cascade_fixture()
    grp = fg.runs_fixture()["groups"][f"cascade.{sampler}"]
    steps, want, twin = grp["steps"], grp["runs"][which], grp["twin"]
    assert nerr(want[-1], twin[-1]) > 10 * BAR, "the schedule must matter for this test to say anything"
    noise = fs.fixed_noise(grp["noise"])
    scales = fg.scales_of(which, steps)
    again = fg.guided_sample(fs.cascade_specs(), g["image_sizes"], g["text_embeds"], sampler=sampler, steps=steps, scales=[scales] * 2, noise_fn=noise,
                             return_all=True)
    assert all(torch.allclose(a, b, atol=1e-5) for a, b in zip(again, want)), "tests/golden/guidance_runs.pt is stale"
    model = fs.cascade_model(timesteps=steps) if sampler == "ddpm" else fs.cascade_model()
    kw = dict(return_all_unet_outputs=True, **fg.schedule_kwargs(which), **({} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=steps)))
    outs = model.sample(**kw, **_common(g["text_embeds"], noise))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"{sampler}, {which} at {steps} steps vs the restatement: {errs}; vs the constant twin {[nerr(o, t) for o, t in zip(outs, twin)]}")
    assert max(errs) < BAR, errs
    pattern = "".join("U" if s == 1.0 else "G" for s in scales)
    launched = _plans(cpu_backend)
    # per stage: the warm-up launch of each captured plan (guided first), then one launch per step
    warm = "G" + ("U" if "U" in pattern else "")
    assert launched == (warm + pattern) * 2, (launched, pattern)
    n = len(cpu_backend.launches)
    eager = model.sample(use_graph=False, **kw, **_common(g["text_embeds"], noise))
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    assert _plans(cpu_backend, n) == pattern * 2
    siblings = [st["sibling"] for st in model._stages.values() if st["sibling"] is not None]
    assert len(siblings) == (2 if which == "interval" else 0) and len(model._stages) == (4 if which == "interval" else 2)
    for sib in siblings:
        owner = [st for st in model._stages.values() if st["sibling"] is sib][0]
        assert sib["eng"].R == 2 and owner["eng"].R == 4 and sib["eng"].x_in is owner["eng"].x_in and sib["step_ptr"] is owner["step_ptr"]
        assert sib["coef"] is owner["coef"] and sib["seed_dev"] is owner["seed_dev"] and sib["final"] is owner["final"]
        assert sib["eng"].lowres_in is owner["eng"].lowres_in and sib["x0_prev"] is owner["x0_prev"] and sib["x0_thr"] is owner["x0_thr"]
        # the whole sampler state, from the one list the driver keeps: the sibling holds the owner's very objects
        assert {"step_ptr", "seed_dev", "row_keys", "noise", "final", "x0_thr", "x0_prev", "tables"} <= set(model.SHARED_STATE)
        assert all(sib[k] is owner[k] for k in model.SHARED_STATE), [k for k in model.SHARED_STATE if sib[k] is not owner[k]]
        assert all(owner[k] is not None for k in ("step_ptr", "seed_dev", "row_keys", "noise", "final", "tables"))
        assert (owner["x0_prev"] is not None) == (owner["x0_thr"] is not None) == (sampler == "dpmpp_2m")
        assert sib["weights"] is owner["weights"] and all(a is b for a, b in zip(sib["tables"], owner["tables"]))
        assert [l for _, s, l in sib["plan"].ops if l == "cfg_x0" and s.cfg == 0], "the sibling is the stage cond_scale = 1 builds"


@pytest.mark.parametrize("tag", ["selfcond.ddpm.steep", "selfcond.ddpm.interval", "selfcond.dpmpp_2m.switch", "video.ddpm.interval", "rect.dpmpp_2m.interval"])
def test_variants_through_the_interpreter(cpu_backend, tag):
    """One Unet(self_cond=True) stage (its next input is the previous step's thresholded x0, whichever plan wrote it; under 2M also the
    history), one Unet3D stage and the cascade's first unet at 16 x 24, with schedules that switch plans, against the recorded restatement."""
    name, sampler, which = tag.split(".")
    grp = fg.runs_fixture()["groups"][f"{name}.{sampler}"]
    want, twin, steps = grp["runs"][which][0], grp["twin"][0], grp["steps"]
    assert nerr(want, twin) > 10 * BAR
    noise = fs.fixed_noise(grp["noise"])
    te, kw = fs.cascade_fixture()["text_embeds"], {}
    if name == "selfcond":
        model = fs.single_stage_model(fs.selfcond_spec(), 16, timesteps=steps)
    elif name == "video":
        v = fs.load("sample_tiny_video.pt")
        model, te, kw = fs.video_model(timesteps=steps), v["text_embeds"], dict(video_frames=v["frames"])
    else:
        model, kw = fs.single_stage_model(fs.cascade_specs()[0], 16, timesteps=steps), dict(image_shapes=((16, 24),))
    kw.update(fg.schedule_kwargs(which), **({} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=steps)))
    out = model.sample(**_common(te, noise, **kw))
    assert tuple(out.shape) == tuple(want.shape)
    err = nerr(out, want)
    print(f"{tag}: {err:.2e} (vs the constant twin {nerr(out, twin):.2e})")
    assert err < BAR
    pattern = "".join("U" if s == 1.0 else "G" for s in fg.scales_of(which, steps))
    assert _plans(cpu_backend).endswith(pattern) and ("U" in pattern or which == "steep")
    assert torch.equal(out, model.sample(**_common(te, noise, **kw))), "history / self_cond buffers are reset per call"


def test_skip_steps_and_init_images_across_a_switch(cpu_backend):
    """init_images + skip_steps = 1 of 5 under dpmpp_2m with a schedule that runs guided -> unguided -> guided -> guided from the first row
    of the run: the step counter, the history and the run's first-order row are the one state of both plans."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(7)
    init = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(8))
    seq = [9.0, 6.0, 1.0, 4.0, 2.0]
    scales = fg.restated_scales(5, fg.COND_SCALE, seq)
    want = fg.guided_sample(fs.cascade_specs()[:1], g["image_sizes"][:1], g["text_embeds"], sampler="dpmpp_2m", steps=5, scales=[scales], noise_fn=noise,
                            init_images=(init,), skip_steps=(1,))
    kw = dict(sampler="dpmpp_2m", sample_steps=5, guidance_schedule=(seq, None), stop_at_unet_number=1)
    out = model.sample(init_images=(init, None), skip_steps=(1, None), **kw, **_common(g["text_embeds"], noise))
    err = nerr(out, want)
    print(f"dpmpp_2m, skip 1 of 5 across a plan switch: {err:.2e}")
    assert err < BAR
    assert _plans(cpu_backend).endswith("GUGG")
    full = model.sample(**kw, **_common(g["text_embeds"], noise))                       # the same cached stages, back at row 0
    want_full = fg.guided_sample(fs.cascade_specs()[:1], g["image_sizes"][:1], g["text_embeds"], sampler="dpmpp_2m", steps=5, scales=[scales], noise_fn=noise)
    assert nerr(full, want_full) < BAR and nerr(full, out) > 10 * BAR and _plans(cpu_backend).endswith("GGUGG")


# ------------------------------------------------------------------------------------------------ 6. refusals

@pytest.fixture()
def no_launch(cpu_backend, monkeypatch):
    from imagen_pytorch_amd import ops

    def launched(self, stream=None):
        raise AssertionError(f"plan '{self.name}' was launched")
    monkeypatch.setattr(ops.Plan, "run", launched)


def test_refusals_come_before_any_launch(no_launch):
    from imagen_pytorch_amd import ElucidatedImagen, Imagen, Unet, ops
    from imagen_pytorch_amd.distributed import sample_sharded
    from oracle.make_golden import ELUCIDATED_HP

    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False, timesteps=4)
    te = g["text_embeds"]
    base = dict(text_embeds=te, cond_scale=3.0, use_tqdm=False, device="cpu")
    known, keep = torch.rand(2, 3, 32, 32), torch.rand(2, 32, 32) > 0.5
    nan, inf = float("nan"), float("inf")
    bad = (dict(guidance_schedule=[1.0, 2.0, 3.0]), dict(guidance_schedule=[1.0] * 5), dict(guidance_schedule=([3.0] * 4, [3.0] * 3)),
           dict(guidance_schedule=[3.0] * 6, sampler="dpmpp_2m", sample_steps=5),
           dict(guidance_interval=(0.5, 0.5)), dict(guidance_interval=(0.8, 0.2)), dict(guidance_interval=(-0.1, 0.5)), dict(guidance_interval=(0.2, 1.5)),
           dict(guidance_interval=(nan, 0.5)), dict(guidance_interval=0.5), dict(guidance_interval=((0.2, 0.8), (0.9, 0.1))),
           dict(guidance_interval=((0.2, 0.8),) * 3), dict(guidance_schedule=(fg.RAMP,) * 3),
           dict(guidance_schedule=lambda t: nan), dict(guidance_schedule=[1.0, inf, 2.0, 3.0]), dict(guidance_schedule=lambda t: 1e39 * t + 1.0),
           dict(guidance_schedule="ramp"), dict(guidance_schedule=3.0),
           dict(guidance_schedule=fg.RAMP, inpaint_images=known, inpaint_masks=keep), dict(guidance_interval=(0.2, 0.8), inpaint_images=known, inpaint_masks=keep))
    for kw in bad:
        with pytest.raises(ValueError):
            model.sample(**base, **kw)
        with pytest.raises(ValueError):
            model.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", **kw)
        with pytest.raises(ValueError):
            sample_sharded(model.sample, te, cond_scale=3.0, use_tqdm=False, device="cpu", **kw)
    for kw in (dict(guidance_schedule=fg.RAMP), dict(guidance_interval=(0.2, 0.8))):
        with pytest.raises(ValueError, match="common keyword"):
            model.sample_requests([dict(text_embeds=te, **kw)], cond_scale=3.0, device="cpu")
        with pytest.raises(ValueError):
            model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", guidance_interval=(0.9, 0.1))
    # a model that cannot be guided: trained without conditional dropout; without a text branch; a stage whose unet has none
    unets = lambda **kw: [Unet(**{**u["kwargs"], **kw}).eval() for u in g["unets"]]
    plain = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.0).eval()
    uncond = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, condition_on_text=False).eval()
    mixed = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.1).eval()
    mixed.unets[1].cond_on_text = False
    for kw in (dict(guidance_schedule=fg.RAMP), dict(guidance_interval=(0.2, 0.8))):
        with pytest.raises(ValueError, match="conditional dropout"):
            plain.sample(text_embeds=te, use_tqdm=False, device="cpu", **kw)
        with pytest.raises(ValueError, match="text branch"):
            uncond.sample(batch_size=2, use_tqdm=False, device="cpu", **kw)
        with pytest.raises(ValueError, match="unet 2 has no text branch"):
            mixed.sample(**base, **kw)
    edm = ElucidatedImagen(unets(), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **ELUCIDATED_HP)
    for kw in (dict(guidance_schedule=fg.RAMP), dict(guidance_interval=(0.2, 0.8)), dict(guidance_schedule=[3.0] * 4)):
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            edm.sample(**base, **kw)
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            edm.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", **kw)
    assert not model._stages and not edm._stages and not plain._stages and not uncond._stages and not mixed._stages
    # the op validates its field
    t = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="cfg"):
        ops.cfg_x0(ops.Plan(), t, t, t, torch.zeros(1, dtype=torch.int32), t, t, B=1, n_per_sample=4, cfg=3, cond_scale=1.0)
    with pytest.raises(ValueError, match="table"):
        ops.cfg_x0(ops.Plan(), t, t, torch.zeros(4, 7), torch.zeros(1, dtype=torch.int32), t, t, B=1, n_per_sample=4, cfg=2, cond_scale=1.0)


# ------------------------------------------------------------------------------------------------ 7. the other entry points

def test_pipelined_sharded_requests_negative_prompt_and_lanes(cpu_backend):
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    te = g["text_embeds"]
    from imagen_pytorch_amd.distributed import sample_sharded

    sched = dict(guidance_schedule=fg.RAMP, guidance_interval=fg.INTERVAL)
    common = dict(cond_scale=fg.COND_SCALE, device="cpu", **sched)
    fns = [fs.memo_noise(11), fs.memo_noise(12)]
    batches = [dict(text_embeds=te * s, noise_fn=fn) for s, fn in zip((1.0, 0.9), fns)]
    seq = [model.sample(use_tqdm=False, **common, **b) for b in batches]
    plain = model.sample(use_tqdm=False, cond_scale=fg.COND_SCALE, device="cpu", **batches[0])
    assert nerr(seq[0], plain) > 10 * BAR
    pipe = model.sample_pipelined(batches, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(pipe[0], pipe[1])
    with model.lane(3):
        assert torch.equal(model.sample(use_tqdm=False, **common, **batches[0]), seq[0])
    assert torch.equal(sample_sharded(model.sample, te, use_tqdm=False, noise_fn=fns[0], **common), seq[0])
    # merged requests under a deterministic solver: each equals its own call
    solver = dict(sampler="dpmpp_2m", sample_steps=4, cond_scale=fg.COND_SCALE, device="cpu", guidance_interval=fg.INTERVAL)
    reqs = [dict(text_embeds=te[:1], seed=21), dict(text_embeds=te, seed=22)]
    merged = model.sample_requests(reqs, **solver)
    own = [model.sample(use_tqdm=False, **solver, **r) for r in reqs]
    errs = [nerr(a, b) for a, b in zip(merged, own)]
    print(f"merged requests with an interval vs their own calls (interpreter): {errs}")
    assert max(errs) < BAR
    # a negative prompt acts on the guided steps only (the unguided plan has no null rows), also through a conditioning handle
    neg = torch.randn(1, 6, 32, generator=torch.Generator().manual_seed(5))
    negm = torch.ones(1, 6, dtype=torch.bool)
    noise = fs.memo_noise(13)
    T = g["timesteps"]
    scales = fg.scales_of("interval", T)
    assert 1.0 in scales and fg.COND_SCALE in scales
    want = fg.guided_sample(fs.cascade_specs(), g["image_sizes"], te, sampler="ddpm", steps=T, scales=[scales] * 2, noise_fn=noise, negative=(neg, negm))
    kw = dict(cond_scale=fg.COND_SCALE, use_tqdm=False, noise_fn=noise, device="cpu", guidance_interval=fg.INTERVAL)
    out = model.sample(text_embeds=te, negative_text_embeds=neg, **kw)
    err, gap = nerr(out, want), nerr(out, model.sample(text_embeds=te, **kw))
    print(f"negative prompt with an interval: {err:.2e} from the restatement, {gap:.2e} from the call without it")
    assert err < BAR and gap > 2 * BAR
    handle = model.prepare_conditioning(text_embeds=te, negative_text_embeds=neg, device="cpu")
    assert torch.equal(model.sample(conditioning=handle, **kw), out)
    # stage 2 alone from stage 1's image
    outs = model.sample(text_embeds=te, return_all_unet_outputs=True, **kw)
    assert torch.equal(model.sample(text_embeds=te, start_at_unet_number=2, start_image_or_video=outs[0], **kw), outs[1])


def test_sample_and_sample_pipelined_agree_on_a_negative_prompt_beside_a_schedule(cpu_backend):
    """Both entries check a negative prompt against the scales the schedule resolves to, through the one `_resolve`: a schedule that guides
    (varying, or constant and not 1) beside cond_scale = 1 is sampled, bit-equal; a schedule of ones beside cond_scale = 3 is refused by both,
    and so is cond_scale = 1 with no schedule."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    te = g["text_embeds"]
    T = g["timesteps"]
    neg = dict(negative_text_embeds=torch.randn(1, 6, 32, generator=torch.Generator().manual_seed(5)))
    ramp = [3.0 - i / T for i in range(T)]
    for sched in (ramp, [3.0] * T):
        kw = dict(cond_scale=1.0, guidance_schedule=sched, device="cpu", **neg)
        batch = dict(text_embeds=te, noise_fn=fs.memo_noise(31))
        seq = model.sample(use_tqdm=False, **kw, **batch)
        assert torch.equal(model.sample_pipelined([batch], **kw)[0], seq)
        assert not torch.equal(seq, model.sample(use_tqdm=False, **{k: v for k, v in kw.items() if k not in neg}, **batch))
    stages = len(model._stages)
    for kw in (dict(cond_scale=3.0, guidance_schedule=[1.0] * T), dict(cond_scale=1.0)):
        with pytest.raises(ValueError, match="cond_scale is 1 on every stage"):
            model.sample(text_embeds=te, use_tqdm=False, device="cpu", **kw, **neg)
        with pytest.raises(ValueError, match="cond_scale is 1 on every stage"):
            model.sample_pipelined([dict(text_embeds=te)], device="cpu", **kw, **neg)
    assert len(model._stages) == stages
