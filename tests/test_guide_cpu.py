"""CPU: guidance rescale and adaptive projected guidance of Imagen.sample — `guidance_rescale=phi`, `guidance_apg=dict(eta=, norm_threshold=,
momentum=)` — on the real driver with the plan interpreter as launcher (tests/plan_interp_guide.py, which states GUIDE_X0's contract), in the
style of tests/test_guidance_cpu.py.

  1. how the keywords resolve per unet, and every refusal, before anything is launched;
  2. which op every step launches (counted); a call without the keywords builds the parent commit's launch lists and cache keys; ABI 15, the new
     kind in the extension range, its struct mirror against imagen_sizeof;
  3. the recorded runs (tests/fixtures_guide.py, tests/golden/guide_runs.pt) of the three samplers and of the variants against the driver,
     bar 2e-2, each >= 10 bars from its plain-CFG twin;
  4. the running average is reset between two calls on one cached stage;
  5. the keywords through sample_pipelined, sample_sharded, sample_requests and on a lane;
  6. the kernel cases of tests/test_guide_kernel_gpu.py on the CPU emulation of the kernel library when IMAGEN_EMUL_TESTS=1."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_guidance as fg  # noqa: E402
import fixtures_guide as fgd  # noqa: E402
import fixtures_solver as fs  # noqa: E402
from fixtures_guide import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend as _replay_backend  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-2      # the project's bar of a sampled stage against its restatement (tests/test_sample_cpu_replay.py, tests/test_solver_cpu.py)


@pytest.fixture()
def cpu_backend(_replay_backend, monkeypatch):  # noqa: F811
    """The replay backend of tests/test_sample_cpu_replay.py with the interpreter that knows GUIDE_X0 behind ops.Plan.run."""
    from imagen_pytorch_amd import ops
    from plan_interp_guide import GuideInterpreter

    it = GuideInterpreter()
    monkeypatch.setattr(ops.Plan, "run", lambda self, stream=None: it.run(self))
    return it


def _common(te, noise, **kw):
    return dict(text_embeds=te, cond_scale=fgd.COND_SCALE, use_tqdm=False, noise_fn=noise, device="cpu", **kw)


# ------------------------------------------------------------------------------------------------ 1. resolution and refusals

def test_keywords_resolve_per_unet(cpu_backend):
    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False, timesteps=(4, 5))
    resolve = lambda **kw: model._resolve(model._call(text_embeds=g["text_embeds"], device="cpu", cond_scale=3.0, **kw))
    assert resolve().guide is None
    assert resolve(guidance_rescale=0.7).guide == (("rescale", 0.7),) * 2
    assert resolve(guidance_rescale=(None, 1)).guide == (None, ("rescale", 1.0))
    assert resolve(guidance_apg=dict(eta=0.5)).guide == (("apg", 0.5, 0.0, 0.0),) * 2
    assert resolve(guidance_apg=dict(norm_threshold=2.5, momentum=-0.5)).guide == (("apg", 0.0, 2.5, -0.5),) * 2
    assert resolve(guidance_apg=dict(norm_threshold=-1.0)).guide == (("apg", 0.0, 0.0, 0.0),) * 2, "a threshold <= 0 is no threshold"
    assert resolve(guidance_rescale=(0.3, None), guidance_apg=(None, {})).guide == (("rescale", 0.3), ("apg", 0.0, 0.0, 0.0))
    # a stage at cond_scale 1 beside a guided one is no error: it stays the plain stage
    c = model._resolve(model._call(text_embeds=g["text_embeds"], device="cpu", cond_scale=(1.0, 3.0), guidance_rescale=0.7))
    assert c.guide == (("rescale", 0.7),) * 2
    assert not model._stages


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
    bad = (dict(guidance_rescale=0.5, guidance_apg={}), dict(guidance_rescale=(0.5, None), guidance_apg=({}, None)),      # both on one stage
           dict(guidance_rescale=-0.1), dict(guidance_rescale=1.5), dict(guidance_rescale=nan), dict(guidance_rescale="0.7"), dict(guidance_rescale=True),
           dict(guidance_rescale=(0.5, 0.5, 0.5)), dict(guidance_rescale=[0.5]), dict(guidance_rescale=(0.5, "x")),
           dict(guidance_apg=0.5), dict(guidance_apg=dict(beta=1.0)), dict(guidance_apg=dict(eta=nan)), dict(guidance_apg=dict(eta=inf)),
           dict(guidance_apg=dict(norm_threshold=inf)), dict(guidance_apg=dict(momentum=nan)), dict(guidance_apg=dict(momentum="a")),
           dict(guidance_apg=({}, {}, {})), dict(guidance_apg=({}, 3)),
           dict(guidance_rescale=0.5, inpaint_images=known, inpaint_masks=keep), dict(guidance_apg={}, inpaint_images=known, inpaint_masks=keep),
           dict(guidance_rescale=0.5, cond_scale=1.0), dict(guidance_apg={}, cond_scale=(1.0, 1.0)),                       # nothing is guided
           dict(guidance_rescale=(0.5, None), cond_scale=(1.0, 3.0)))                                                        # ... where the setting is
    for kw in bad:
        kw = {**base, **kw}
        with pytest.raises(ValueError):
            model.sample(**kw)
        rest = {k: v for k, v in kw.items() if k not in ("text_embeds", "use_tqdm")}
        with pytest.raises(ValueError):
            model.sample_pipelined([dict(text_embeds=te)], **rest)
        with pytest.raises(ValueError):
            sample_sharded(model.sample, te, **{k: v for k, v in kw.items() if k != "text_embeds"})
    for kw in (dict(guidance_rescale=0.5), dict(guidance_apg={})):
        with pytest.raises(ValueError, match="common keyword"):
            model.sample_requests([dict(text_embeds=te, **kw)], cond_scale=3.0, device="cpu")
    with pytest.raises(ValueError):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", guidance_rescale=2.0)
    # a constant schedule at 1 is "no schedule"; a schedule that varies is guidance
    with pytest.raises(ValueError, match="silently ignored"):
        model.sample(**{**base, "cond_scale": 1.0}, guidance_rescale=0.5, guidance_schedule=lambda t: 1.0)
    # a model that cannot be guided: trained without conditional dropout; without a text branch; a stage whose unet has none
    unets = lambda **kw: [Unet(**{**u["kwargs"], **kw}).eval() for u in g["unets"]]
    plain = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.0).eval()
    uncond = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, condition_on_text=False).eval()
    mixed = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.1).eval()
    mixed.unets[1].cond_on_text = False
    for kw in (dict(guidance_rescale=0.5), dict(guidance_apg={})):
        with pytest.raises(ValueError, match="conditional dropout"):
            plain.sample(text_embeds=te, use_tqdm=False, device="cpu", **kw)
        with pytest.raises(ValueError, match="text branch"):
            uncond.sample(batch_size=2, use_tqdm=False, device="cpu", **kw)
        with pytest.raises(ValueError, match="unet 2 has no text branch"):
            mixed.sample(**base, **kw)
    edm = ElucidatedImagen(unets(), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **ELUCIDATED_HP)
    for kw in (dict(guidance_rescale=0.5), dict(guidance_apg={}), dict(guidance_apg=dict(eta=1.0))):
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            edm.sample(**base, **kw)
        with pytest.raises(ValueError, match="ElucidatedImagen"):
            edm.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", **kw)
    assert not model._stages and not edm._stages and not plain._stages and not uncond._stages and not mixed._stages
    # the op validates its fields
    t, z = torch.zeros(4, 8), torch.zeros(1, dtype=torch.int32)
    kw = dict(B=1, n_per_sample=4, cfg=1, cond_scale=1.0)
    with pytest.raises(ValueError, match="mode"):
        ops.guide_x0(ops.Plan(), t, t, t, z, t, t, mode="cads", **kw)
    for phi in (-0.1, 1.1, nan):
        with pytest.raises(ValueError, match="phi"):
            ops.guide_x0(ops.Plan(), t, t, t, z, t, t, mode="rescale", phi=phi, **kw)
    for bad_kw in (dict(eta=inf), dict(norm_threshold=nan), dict(momentum=inf)):
        with pytest.raises(ValueError, match="finite"):
            ops.guide_x0(ops.Plan(), t, t, t, z, t, t, mode="apg", **bad_kw, **kw)
    with pytest.raises(ValueError, match="cfg"):
        ops.guide_x0(ops.Plan(), t, t, t, z, t, t, mode="rescale", **{**kw, "cfg": 0})
    with pytest.raises(ValueError, match="avg"):
        ops.guide_x0(ops.Plan(), t, t, t, z, t, t, mode="apg", momentum=-0.5, **kw)
    with pytest.raises(ValueError, match="cfg"):
        ops.cfg_x0(ops.Plan(), t, t, t, z, t, t, B=1, n_per_sample=4, cfg=3, cond_scale=1.0)      # CFG_X0 itself is as it was


# ------------------------------------------------------------------------------------------------ 2. ABI, launch lists, keys

def test_abi_is_15_and_the_new_kind_is_an_extension(monkeypatch):
    from imagen_pytorch_amd import _abi, engine
    from plan_interp_guide import GuideInterpreter

    assert _abi.ENUMS["IMAGEN_ABI_VERSION"] == 15
    kind = _abi.ENUMS["IMAGEN_OP_GUIDE_X0"]
    assert kind == 33 and kind not in _abi.OP_STRUCT and _abi.EXT_OP_STRUCT[kind] is _abi.STRUCTS["ImagenGuideX0Params"]
    assert _abi.STRUCT_KIND[_abi.STRUCTS["ImagenGuideX0Params"]] == kind and _abi.STRUCT_KIND[_abi.STRUCTS["ImagenCfgX0Params"]] == 13
    assert set(GuideInterpreter.DISPATCH) == set(_abi.OP_STRUCT) | {kind}
    lib = _abi.load_library()
    assert lib.imagen_sizeof(kind) == ctypes.sizeof(_abi.STRUCTS["ImagenGuideX0Params"]) > 0
    _abi.require_ext_op(kind, "test")
    # a library from before the kind: refused with a message that says what to do, not a crash
    monkeypatch.setitem(_abi.EXT_OP_STRUCT, 9999, _abi.STRUCTS["ImagenGuideX0Params"])
    with pytest.raises(_abi.ImagenHipError, match="rebuild"):
        _abi.require_ext_op(9999, "guide_x0")
    # launch validation on the host, no GPU needed
    p = _abi.STRUCTS["ImagenGuideX0Params"]()
    assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p), None) != 0 and b"guide_x0" in lib.imagen_last_error()
    assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p) - 4, None) != 0 and b"params struct" in lib.imagen_last_error()
    # the default call's launch lists are the parent commit's
    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))
    want = json.load(open(os.path.join(fs.GOLDEN, "solver_parent_launch_list_abi15.json")))
    assert fs.launch_lists() == want


def _labels(st):
    return [l for _, _, l in st["plan"].ops]


def test_which_op_each_step_launches(cpu_backend):
    """A call without the keywords keeps its stages (keys of 16 entries, CFG_X0); a setting is a stage of its own whose key ends in it and
    whose plan has GUIDE_X0's two launches where CFG_X0 stood, everything else the same; with an interval the unguided steps replay the
    B-row sibling's CFG_X0 and no GUIDE_X0."""
    from imagen_pytorch_amd import _abi

    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(3)
    kw = _common(g["text_embeds"], noise)
    a = model.sample(**kw)
    keys = dict(model._stages)
    assert len(keys) == 2 and all(len(k) == 16 for k in keys) and not cpu_backend.guides
    assert all("cfg_x0" in _labels(st) and st["guide"] is None and st["avg"] is None and st["head"] is None for st in keys.values())
    T = g["timesteps"]
    for which, setting in fgd.SETTINGS.items():
        n0, c0 = len(cpu_backend.guides), len(cpu_backend.launches)
        b = model.sample(**kw, **fgd.KEYWORDS[which])
        new = {k: v for k, v in model._stages.items() if k not in keys}
        assert len(new) == 2 and all(k[:16] in keys and k[16] == ("guide", setting) for k in new), list(new)
        assert nerr(b, a) > 10 * BAR
        mode = _abi.ENUMS["IMAGEN_GUIDE_RESCALE" if which == "rescale" else "IMAGEN_GUIDE_APG"]
        # per stage: one warm-up launch before capture, then T steps; reduce then apply, cfg 1 (the immediate)
        assert cpu_backend.guides[n0:] == [(mode, 0, 1), (mode, 1, 1)] * (2 * (T + 1)) and len(cpu_backend.launches) == c0, "no CFG_X0 on a guided step"
        for k, st in new.items():
            plain = _labels(keys[k[:16]])
            i = plain.index("cfg_x0")
            assert _labels(st) == plain[:i] + ["guide_x0.reduce", "guide_x0.apply"] + plain[i + 1:]
            assert (st["avg"] is not None) == (st["head"] is not None) == (which == "apg")
            if which == "apg":
                assert [l for _, _, l in st["head"].ops] == ["memset32"] and tuple(st["avg"].shape) == (2, st["n"])
        keys.update(new)
        assert torch.equal(model.sample(**kw, **fgd.KEYWORDS[which]), b) and len(model._stages) == len(keys), "the stages are cached"
    assert torch.equal(model.sample(**kw), a), "the call without the keywords still meets its own stages"
    # an interval: 4 steps, guided on the middle two; the sibling is CFG_X0 at cfg 0 and shares no GUIDE_X0
    n0, c0 = len(cpu_backend.guides), len(cpu_backend.launches)
    model.sample(**kw, **fgd.KEYWORDS["apg"], guidance_interval=fg.INTERVAL, stop_at_unet_number=1)
    scales = fg.scales_of("interval", T)
    guided, unguided = sum(s != 1.0 for s in scales), sum(s == 1.0 for s in scales)
    assert guided and unguided
    # (the warm-up launch + the steps of each plan)
    assert len(cpu_backend.guides) - n0 == 2 * (1 + guided) and [c for c, _ in cpu_backend.launches[c0:]] == [0] * (1 + unguided)
    st = [v for k, v in model._stages.items() if k not in keys and v["sibling"] is not None][0]
    assert "cfg_x0" in _labels(st["sibling"]) and st["sibling"]["guide"] is None and st["guide"] == fgd.APG
    assert [p.cfg for _, p, l in st["plan"].ops if l.startswith("guide_x0")] == [2, 2]


# ------------------------------------------------------------------------------------------------ 3. the recorded runs

@pytest.mark.parametrize("which", ["rescale", "apg"])
@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m", "ddim"])
def test_cascade_runs_through_the_interpreter(cpu_backend, sampler, which):
    """The tiny cascade with the setting on both stages, graph path and eager, against the restatement — recomputed here and equal to the
    recorded one the GPU tests read — and >= 10 bars from the plain-CFG twin."""
    g = fs.cascade_fixture()
    grp = fgd.runs_fixture()["groups"][f"cascade.{sampler}"]
    steps, want, twin = grp["steps"], grp["runs"][which], grp["twin"]
    assert nerr(want[-1], twin[-1]) > 10 * BAR, "the keyword must matter for this test to say anything"
    noise = fs.fixed_noise(grp["noise"])
    again = fgd.guide_sample(fs.cascade_specs(), g["image_sizes"], g["text_embeds"], sampler=sampler, steps=steps, scales=[[fgd.COND_SCALE] * steps] * 2,
                             guides=[fgd.SETTINGS[which]] * 2, noise_fn=noise, return_all=True)
    assert all(torch.allclose(a, b, atol=1e-5) for a, b in zip(again, want)), "tests/golden/guide_runs.pt is stale"
    model = fs.cascade_model(timesteps=steps) if sampler == "ddpm" else fs.cascade_model()
    kw = dict(return_all_unet_outputs=True, **fgd.KEYWORDS[which], **({} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=steps)))
    outs = model.sample(**kw, **_common(g["text_embeds"], noise))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"{sampler}, {which} at {steps} steps vs the restatement: {errs}; vs the plain-CFG twin {[nerr(o, t) for o, t in zip(outs, twin)]}")
    assert max(errs) < BAR, errs
    eager = model.sample(use_graph=False, **kw, **_common(g["text_embeds"], noise))
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))


@pytest.mark.parametrize("name", ["v.rescale", "selfcond.apg", "video.apg", "rect.rescale", "negative_interval.apg"])
def test_variants_through_the_interpreter(cpu_backend, name):
    """A v-objective stage, a Unet(self_cond=True) stage, a Unet3D stage, the cascade's first unet at 16 x 24, and a negative prompt with a
    guidance interval (the running average lives through the guided steps only), against the recorded restatement.  The second call on the
    same cached stage equals the first: the running average is reset at the start of every run."""
    v = fgd.variants()[name]
    grp = fgd.runs_fixture()["groups"][name]
    want, twin, steps = grp["runs"][v["which"]][0], grp["twin"][0], grp["steps"]
    assert nerr(want, twin) > 10 * BAR
    noise = fs.fixed_noise(grp["noise"])
    model = v["model"]("cpu", steps)
    kw = dict(fgd.KEYWORDS[v["which"]], **v.get("sample", {}), **({} if v["sampler"] == "ddpm" else dict(sampler=v["sampler"], sample_steps=steps)))
    out = model.sample(**_common(v["te"], noise, **kw))
    assert tuple(out.shape) == tuple(want.shape)
    err = nerr(out, want)
    print(f"{name}: {err:.2e} (vs the plain-CFG twin {nerr(out, twin):.2e})")
    assert err < BAR
    assert cpu_backend.guides and len(model._stages) == (2 if v.get("interval") else 1)
    n = len(model._stages)
    assert torch.equal(out, model.sample(**_common(v["te"], noise, **kw))) and len(model._stages) == n, "avg / history / self_cond buffers are reset per call"


def test_running_average_is_reset_between_calls(cpu_backend):
    """Two calls on one cached stage with momentum: the second equals the first although the first left its running average behind; a
    call with max_steps = 1 in between (another run of the same stage, stopped early) changes nothing either."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(31)
    kw = dict(_common(g["text_embeds"], noise), guidance_apg=dict(eta=0.0, momentum=-0.75), stop_at_unet_number=1)
    a = model.sample(**kw)
    (st,) = model._stages.values()
    left = st["avg"].clone()
    assert float(left.abs().max()) > 0
    model.sample(**kw, max_steps=1)
    assert not torch.equal(st["avg"], left)
    assert torch.equal(model.sample(**kw), a) and torch.equal(st["avg"], left) and len(model._stages) == 1
    assert nerr(model.sample(**{**kw, "guidance_apg": dict(eta=0.0)}), a) > BAR, "the momentum matters"


# ------------------------------------------------------------------------------------------------ 5. the other entry points

def test_pipelined_sharded_requests_and_lanes(cpu_backend):
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    te = g["text_embeds"]
    from imagen_pytorch_amd.distributed import sample_sharded

    for which in ("rescale", "apg"):
        common = dict(cond_scale=fgd.COND_SCALE, device="cpu", **fgd.KEYWORDS[which])
        fns = [fs.memo_noise(11), fs.memo_noise(12)]
        batches = [dict(text_embeds=te * s, noise_fn=fn) for s, fn in zip((1.0, 0.9), fns)]
        seq = [model.sample(use_tqdm=False, **common, **b) for b in batches]
        plain = model.sample(use_tqdm=False, cond_scale=fgd.COND_SCALE, device="cpu", **batches[0])
        assert nerr(seq[0], plain) > 10 * BAR
        pipe = model.sample_pipelined(batches, **common)
        assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(pipe[0], pipe[1])
        with model.lane(3):
            assert torch.equal(model.sample(use_tqdm=False, **common, **batches[0]), seq[0])
        assert torch.equal(sample_sharded(model.sample, te, use_tqdm=False, noise_fn=fns[0], **common), seq[0])
        # merged requests under a deterministic solver: per-row statistics, so each equals its own call
        solver = dict(sampler="dpmpp_2m", sample_steps=4, **common)
        reqs = [dict(text_embeds=te[:1], seed=21), dict(text_embeds=te, seed=22)]
        merged = model.sample_requests(reqs, **solver)
        own = [model.sample(use_tqdm=False, **solver, **r) for r in reqs]
        errs = [nerr(a, b) for a, b in zip(merged, own)]
        print(f"merged requests with {which} vs their own calls (interpreter): {errs}")
        assert max(errs) < BAR
        # a pipelined cascade whose first stage runs at cond_scale 1: that stage is the plain one, the call is no error
        mixed = dict(common, cond_scale=(1.0, fgd.COND_SCALE))
        assert torch.equal(model.sample_pipelined(batches[:1], **mixed)[0], model.sample(use_tqdm=False, **mixed, **batches[0]))
    # a conditioning handle and stage 2 alone from stage 1's image
    kw = dict(cond_scale=fgd.COND_SCALE, use_tqdm=False, noise_fn=fs.memo_noise(13), device="cpu", **fgd.KEYWORDS["apg"])
    outs = model.sample(text_embeds=te, return_all_unet_outputs=True, **kw)
    handle = model.prepare_conditioning(text_embeds=te, device="cpu")
    assert torch.equal(model.sample(conditioning=handle, **kw), outs[1])
    assert torch.equal(model.sample(text_embeds=te, start_at_unet_number=2, start_image_or_video=outs[0], **kw), outs[1])


# ------------------------------------------------------------------------------------------------ 6. the kernel on the CPU emulation

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_kernel_cases_on_the_emulation():
    """csrc/sampler.hip compiled by tools/emul: every case of tests/test_guide_kernel_gpu.py in a child pytest on the emulated library
    (IMAGEN_EMUL_TESTS=1, as cfg_x0's cases run there)."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_guide_kernel_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
