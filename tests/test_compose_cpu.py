"""CPU: composed prompts of Imagen.sample — `compose=[dict(text_embeds= | texts=, text_masks=, weight=, mask=), ...]`, `compose_mask=` — on the
real driver with the plan interpreter as launcher (tests/plan_interp_compose.py, which states COMPOSE_X0's contract), in the style of
tests/test_guide_cpu.py.

  1. how the keywords resolve (batch-1 broadcast, per-unet tuples, [B] weights, masks), and every refusal, before anything is launched;
  2. ABI 15, the new kind in the extension range, its launcher's refusals; a call without the keyword builds the parent commit's launch lists;
  3. engine staging: branch k of a (K + 1) B-row engine == a B-row engine's forward on prompt k alone (through the interpreter);
  4. the recorded runs (tests/fixtures_compose.py, tests/golden/compose_runs.pt) against the driver, bar 2e-2, each >= 10 bars from its twin;
  5. two calls with different weights and masks reuse one stage and one captured plan (counted);
  6. sample_pipelined, lanes, sample_sharded (slices);
  7. the kernel cases of tests/test_compose_kernel_gpu.py on the CPU emulation of the kernel library when IMAGEN_EMUL_TESTS=1."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_compose as fc  # noqa: E402
import fixtures_solver as fs  # noqa: E402
from fixtures_compose import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend as _replay_backend  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-2      # the project's bar of a sampled stage against its restatement (tests/test_guide_cpu.py, tests/test_solver_cpu.py)


@pytest.fixture()
def cpu_backend(_replay_backend, monkeypatch):  # noqa: F811
    """The replay backend of tests/test_sample_cpu_replay.py with the interpreter that knows COMPOSE_X0 behind ops.Plan.run."""
    from imagen_pytorch_amd import ops
    from plan_interp_compose import ComposeInterpreter

    it = ComposeInterpreter()
    monkeypatch.setattr(ops.Plan, "run", lambda self, stream=None: it.run(self))
    return it


def _common(te, noise, **kw):
    return dict(text_embeds=te, cond_scale=fc.COND_SCALE, use_tqdm=False, noise_fn=noise, device="cpu", **kw)


# ------------------------------------------------------------------------------------------------ 1. resolution and refusals

def test_keywords_resolve(cpu_backend):
    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False, timesteps=(4, 5))
    te = g["text_embeds"]
    resolve = lambda **kw: model._resolve(model._call(text_embeds=te, device="cpu", **{"cond_scale": 3.0, **kw})).composed
    assert resolve() is None
    p1, pB = fc.prompt(1, batch=1), fc.prompt(2, batch=2, tokens=5)
    c = resolve(compose=[dict(text_embeds=p1)])
    assert c["K"] == 2 and c["masks"] is None and len(c["prompts"]) == 1
    assert tuple(c["prompts"][0][0].shape) == (1, 7, 32) and tuple(c["prompts"][0][1].shape) == (1, 7), "a batch-1 prompt stays batch 1: the engine repeats it"
    assert all(torch.equal(w, torch.tensor([[3.0, 3.0], [1.0, 1.0]])) for w in c["weights"]), "default weight 1; the main prompt's is cond_scale"
    c = resolve(cond_scale=(2.0, 5.0), compose=[dict(text_embeds=pB, weight=(0.5, -2)), dict(text_embeds=p1, weight=torch.tensor([1.5, 0.0]))])
    assert c["K"] == 3
    assert torch.equal(c["weights"][0], torch.tensor([[2.0, 2.0], [0.5, 0.5], [1.5, 0.0]]))
    assert torch.equal(c["weights"][1], torch.tensor([[5.0, 5.0], [-2.0, -2.0], [1.5, 0.0]]))
    m2, m3 = torch.rand(16, 16), torch.rand(2, 8, 8)
    c = resolve(compose=[dict(text_embeds=p1, mask=m2), dict(text_embeds=p1)], compose_mask=m3)
    assert [None if m is None else tuple(m.shape) for m in c["masks"]] == [(2, 8, 8), (1, 16, 16), None]
    c = resolve(compose=[dict(text_embeds=p1, text_masks=torch.tensor([[True] * 3 + [False] * 4]))])
    assert c["prompts"][0][1].sum() == 3
    # texts go through the encoder hook
    model.encode_text = lambda texts, return_attn_mask=False: (torch.ones(len(texts), 4, 32), torch.ones(len(texts), 4, dtype=torch.bool))
    c = resolve(compose=[dict(texts="fog", weight=2.0), dict(texts=["a", "b"])])
    assert [tuple(e.shape) for e, _ in c["prompts"]] == [(1, 4, 32), (2, 4, 32)]
    # cond_scale 1 with a non-zero further weight is a composition
    assert resolve(cond_scale=1.0, compose=[dict(text_embeds=p1, weight=2.0)])["K"] == 2
    assert not model._stages


@pytest.fixture()
def no_launch(cpu_backend, monkeypatch):
    from imagen_pytorch_amd import ops

    def launched(self, stream=None):
        raise AssertionError(f"plan '{self.name}' was launched")
    monkeypatch.setattr(ops.Plan, "run", launched)


def test_refusals_come_before_any_launch(no_launch):
    from imagen_pytorch_amd import ElucidatedImagen, Imagen, Unet, Unet3D, ops
    from imagen_pytorch_amd.distributed import sample_sharded
    from oracle.make_golden import ELUCIDATED_HP

    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False, timesteps=4)
    te = g["text_embeds"]
    base = dict(text_embeds=te, cond_scale=3.0, use_tqdm=False, device="cpu")
    p = fc.prompt(1, batch=1)
    one = [dict(text_embeds=p)]
    known, keep = torch.rand(2, 3, 32, 32), torch.rand(2, 32, 32) > 0.5
    nan, inf = float("nan"), float("inf")
    bad = (
        (dict(compose=one, guidance_schedule=lambda t: 3.0), "guidance_schedule"), (dict(compose=one, guidance_interval=(0.2, 0.8)), "guidance_interval"),
        (dict(compose=one, guidance_rescale=0.5), "guidance_rescale"), (dict(compose=one, guidance_apg={}), "guidance_apg"),
        (dict(compose=one, inpaint_images=known, inpaint_masks=keep), "inpainting"),
        (dict(compose=one, cond_scale=1.0), None), (dict(compose=[dict(text_embeds=p, weight=0.0)], cond_scale=1.0), "silently ignored"),
        (dict(compose=[dict(text_embeds=p, weight=(0.0, 0.0))], cond_scale=(1.0, 1.0)), "silently ignored"),
        (dict(compose=[]), "non-empty"), (dict(compose=dict(text_embeds=p)), "non-empty"), (dict(compose=[p]), "non-empty"), (dict(compose_mask=torch.ones(16, 16)), "non-empty"),
        (dict(compose=one * 4), "at most 4"),
        (dict(compose=[dict(text_embeds=p, scale=2.0)]), "unknown keys"), (dict(compose=[dict(weight=2.0)]), "one of text_embeds and texts"),
        (dict(compose=[dict(text_embeds=p, texts=["a"])]), "one of text_embeds and texts"),
        (dict(compose=[dict(text_embeds=p[0])]), "invalid text embedding shape"), (dict(compose=[dict(text_embeds=torch.zeros(1, 7, 16))]), "invalid text embedding shape"),
        (dict(compose=[dict(text_embeds=fc.prompt(1, batch=3))]), "neither 1 nor"),
        (dict(compose=[dict(text_embeds=p, text_masks=torch.ones(1, 6, dtype=torch.bool))]), "does not match"),
        (dict(compose=[dict(text_embeds=p, weight=nan)]), "finite"), (dict(compose=[dict(text_embeds=p, weight=(1.0, inf))]), "finite"),
        (dict(compose=[dict(text_embeds=p, weight=torch.tensor([1.0, nan]))]), "finite"),
        (dict(compose=[dict(text_embeds=p, weight="2")]), "a float"), (dict(compose=[dict(text_embeds=p, weight=(1.0, 2.0, 3.0))]), "a float"),
        (dict(compose=[dict(text_embeds=p, weight=torch.ones(3))]), r"\[B\] tensor"),
        (dict(compose=[dict(text_embeds=p, mask=torch.ones(3, 16, 16))]), "H, W"), (dict(compose=[dict(text_embeds=p, mask=torch.ones(16))]), "H, W"),
        (dict(compose=[dict(text_embeds=p, mask=[[1.0]])]), "H, W"), (dict(compose=[dict(text_embeds=p, mask=torch.full((16, 16), 1.5))]), r"outside \[0, 1\]"),
        (dict(compose=[dict(text_embeds=p, mask=torch.full((16, 16), -0.1))]), r"outside \[0, 1\]"), (dict(compose=[dict(text_embeds=p, mask=torch.full((16, 16), nan))]), r"outside \[0, 1\]"),
        (dict(compose=one, compose_mask=torch.full((1, 4, 4), 2.0)), r"compose_mask: values outside"),
    )
    for kw, msg in bad:
        if msg is None:          # (cond_scale 1 with the default further weight 1 is a composition, no refusal: resolved without a launch)
            assert model._resolve(model._call(**{**base, **kw})).composed["K"] == 2
            continue
        kw = {**base, **kw}
        with pytest.raises(ValueError, match=msg):
            model.sample(**kw)
        rest = {k: v for k, v in kw.items() if k not in ("text_embeds", "use_tqdm")}
        with pytest.raises(ValueError, match=msg):
            model.sample_pipelined([dict(text_embeds=te)], **rest)
        with pytest.raises(ValueError, match=msg):
            sample_sharded(model.sample, te, **{k: v for k, v in kw.items() if k != "text_embeds"})
    # a conditioning handle; merged requests, inside and beside
    handle = model.prepare_conditioning(text_embeds=te, device="cpu")
    with pytest.raises(ValueError, match="conditioning"):
        model.sample(conditioning=handle, cond_scale=3.0, use_tqdm=False, device="cpu", compose=one)
    with pytest.raises(ValueError, match="sample_requests"):
        model.sample_requests([dict(text_embeds=te, compose=one)], cond_scale=3.0, device="cpu")
    with pytest.raises(ValueError, match="sample_requests"):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", compose=one)
    with pytest.raises(ValueError, match="sample_requests"):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", compose_mask=torch.ones(4, 4))
    # models that cannot compose: no conditional dropout; no text branch; a stage whose unet has none; a Unet3D stage; ElucidatedImagen
    unets = lambda **kw: [Unet(**{**u["kwargs"], **kw}).eval() for u in g["unets"]]
    plain = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.0).eval()
    uncond = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, condition_on_text=False).eval()
    mixed = Imagen(unets(), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.1).eval()
    mixed.unets[1].cond_on_text = False
    with pytest.raises(ValueError, match="conditional dropout"):
        plain.sample(text_embeds=te, use_tqdm=False, device="cpu", compose=one)
    with pytest.raises(ValueError, match="text branch"):
        uncond.sample(batch_size=2, use_tqdm=False, device="cpu", compose=one)
    with pytest.raises(ValueError, match="unet 2 has no text branch"):
        mixed.sample(**base, compose=one)
    v = fs.load("sample_tiny_video.pt")
    video = fs.video_model("cpu", timesteps=4)
    assert isinstance(video.unets[0], Unet3D)
    with pytest.raises(ValueError, match="Unet3D"):
        video.sample(text_embeds=v["text_embeds"], video_frames=v["frames"], cond_scale=3.0, use_tqdm=False, device="cpu", compose=one)
    edm = ElucidatedImagen(unets(), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **ELUCIDATED_HP)
    with pytest.raises(ValueError, match="ElucidatedImagen"):
        edm.sample(**base, compose=one)
    with pytest.raises(ValueError, match="ElucidatedImagen"):
        edm.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", compose=one)
    for m in (model, edm, plain, uncond, mixed, video):
        assert not m._stages
    # the op validates its arguments before it adds anything to the plan
    t, z = torch.zeros(8, 8), torch.zeros(1, dtype=torch.int32)
    w = torch.ones(2, 1)
    ok = dict(B=1, n_per_sample=8, hw=4, weights=w)
    for kw, msg in ((dict(weights=torch.ones(5, 1)), "K = 5"), (dict(weights=torch.ones(0, 1)), "K = 0"), (dict(weights=torch.ones(2, 3)), "batch"),
                    (dict(weights=torch.ones(2, 1, dtype=torch.float64)), "fp32"), (dict(weights=[1.0]), "fp32"), (dict(hw=0), "hw"), (dict(hw=-4), "hw"),
                    (dict(hw=3), "hw"), (dict(masks=torch.ones(2, 1, 8)), "masks"), (dict(masks=torch.ones(1, 1, 4)), "masks"),
                    (dict(objective="eps"), "objective"), (dict(n_per_sample=64), "pred holds")):
        plan = ops.Plan()
        with pytest.raises(ValueError, match=msg):
            ops.compose_x0(plan, t, t, t, z, t, t, **{**ok, **kw})
        assert len(plan) == 0


# ------------------------------------------------------------------------------------------------ 2. ABI, launch lists

def test_abi_is_15_and_the_new_kind_is_an_extension(monkeypatch):
    from imagen_pytorch_amd import _abi, engine
    from plan_interp_compose import ComposeInterpreter
    from plan_interp_guide import GuideInterpreter

    assert _abi.ENUMS["IMAGEN_ABI_VERSION"] == 15 and _abi.ENUMS["IMAGEN_OP_KIND_COUNT"] == 33
    kind = _abi.ENUMS["IMAGEN_OP_COMPOSE_X0"]
    st = _abi.STRUCTS["ImagenComposeX0Params"]
    assert kind == 34 and _abi.ENUMS["IMAGEN_OP_EXT_END"] == 35 and _abi.ENUMS["IMAGEN_OP_GUIDE_X0"] == 33 and _abi.ENUMS["IMAGEN_COMPOSE_MAX"] == 4
    assert kind not in _abi.OP_STRUCT and _abi.EXT_OP_STRUCT[kind] is st and _abi.STRUCT_KIND[st] == kind and len(_abi.OP_STRUCT) == 32
    assert set(ComposeInterpreter.DISPATCH) == set(GuideInterpreter.DISPATCH) | {kind}
    lib = _abi.load_library()
    assert lib.imagen_sizeof(kind) == ctypes.sizeof(st) > 0
    _abi.require_ext_op(kind, "test")
    # a library from before the kind: refused with a message that says what to do, not a crash
    monkeypatch.setitem(_abi.EXT_OP_STRUCT, 9999, st)
    with pytest.raises(_abi.ImagenHipError, match="rebuild"):
        _abi.require_ext_op(9999, "compose_x0")
    # the launcher's refusals go through the library's error path, on the host, no GPU needed
    buf = (ctypes.c_float * 64)()
    step = (ctypes.c_int32 * 1)()

    def params(**kw):
        p = st()
        for f in ("x", "pred", "coef", "x0", "absx0", "weights"):
            setattr(p, f, ctypes.addressof(buf))
        p.step_ptr = ctypes.addressof(step)
        p.B, p.n_per_sample, p.hw, p.K, p.objective = 1, 8, 4, 2, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for kw, msg in ((dict(K=0), b"K outside"), (dict(K=5), b"K outside"), (dict(hw=0), b"hw <= 0"), (dict(hw=-1), b"hw <= 0"), (dict(hw=3), b"no multiple of hw"),
                    (dict(weights=None), b"required"), (dict(objective=3), b"objective")):
        p = params(**kw)
        assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p), None) != 0 and msg in lib.imagen_last_error(), (kw, lib.imagen_last_error())
    p = params()
    assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p) - 4, None) != 0 and b"params struct" in lib.imagen_last_error()
    # the default call's launch lists are the parent commit's
    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))
    want = json.load(open(os.path.join(fs.GOLDEN, "solver_parent_launch_list_abi15.json")))
    assert fs.launch_lists() == want


# ------------------------------------------------------------------------------------------------ 3. engine staging

def _forward_rows(unet, rows, B, size, x, t, **cond):
    """One forward of a dry `rows`-row engine through a fresh interpreter (tests/plan_interp.run_engine, with the keep mask of K prompt sets:
    only the LAST B rows are null rows)."""
    from imagen_pytorch_amd import engine
    from plan_interp import register_engine
    from plan_interp_compose import ComposeInterpreter

    eng = engine.UnetEngine(unet, rows, B, size, torch.device("cpu"), dry=True)
    keep = torch.ones(rows, dtype=torch.bool)
    if rows > B:
        keep[rows - B:] = False
    eng.set_conditioning(keep=keep, lowres_noise_times=None, **cond)
    it = ComposeInterpreter()
    register_engine(it, eng)
    for pl in eng._last_static:
        it.run(pl)
    eng.x_in.copy_(x)
    eng.times.copy_(t.repeat(rows // B))
    it.run(eng.step_plan)
    return eng, eng.out.float().clone().reshape(rows, *x.shape[1:])


@pytest.mark.parametrize("K", [2, 3, 4])
def test_engine_branch_rows_equal_single_prompt_forwards(cpu_backend, K):
    """On a (K + 1) B-row engine over the cascade's first unet, branch k's output rows equal a B-row engine's forward on prompt k alone, the null
    rows equal the B-row null forward (a 2 B-row engine's second half), and with a negative prompt the B-row forward on that prompt.  Both sides
    run through the interpreter, which is deterministic (two B-row runs of one prompt differ by exactly 0: asserted first), and row r of a
    launch depends on row r's inputs alone — so the bar is 0 and the comparison is torch.equal; the measured distance is printed."""
    from imagen_pytorch_amd import Unet

    sd, kw = fs.cascade_specs()[0]
    unet = Unet(**kw).eval()
    unet.load_state_dict(sd)
    B, size = 2, 16
    g = torch.Generator().manual_seed(9)
    x, t = torch.randn(B, 3, size, size, generator=g), torch.tensor([0.3, -1.2])
    te = fs.cascade_fixture()["text_embeds"]
    tm = torch.any(te != 0.0, dim=-1)                # (the mask Imagen.sample derives; None would attend the zero padding up to max_text_len)
    # prompts of different lengths, one of batch 1, one with a mask: the shorter ones are zero-padded and masked inside the shared static plan
    extra = [(fc.prompt(51, batch=1, tokens=5), None), (fc.prompt(52, tokens=11), torch.rand(2, 11, generator=g) > 0.3), (fc.prompt(53, tokens=9), None)][:K - 1]
    prompts = [(te, None)] + extra
    single = lambda emb, mask: _forward_rows(unet, B, B, size, x, t, text_embeds=emb.expand(B, -1, -1),
                                             text_mask=torch.any(emb != 0.0, dim=-1).expand(B, -1) if mask is None else mask)[1]
    a, b = single(*prompts[0]), single(*prompts[0])
    assert torch.equal(a, b), "two B-row interpreter runs of one prompt differ: the bar below would not be 0"
    eng, out = _forward_rows(unet, (K + 1) * B, B, size, x, t, text_embeds=te, text_mask=tm, extra_prompts=extra)
    assert eng.n_prompts == K and tuple(out.shape) == ((K + 1) * B, 3, size, size)
    dist = [nerr(out[k * B:(k + 1) * B], single(*prompts[k])) for k in range(K)]
    two = _forward_rows(unet, 2 * B, B, size, x, t, text_embeds=te, text_mask=tm)[1]
    dist.append(nerr(out[K * B:], two[B:]))
    print(f"K = {K}: branch rows vs the B-row forwards {dist} (bar 0)")
    assert max(dist) == 0.0, dist
    assert all(nerr(out[k * B:(k + 1) * B], out[K * B:]) > 1e-3 for k in range(K)), "every prompt moves its rows off the null ones"
    # a negative prompt sits on the null rows and leaves the prompt rows alone
    neg = fc.NEGATIVE
    _, outn = _forward_rows(unet, (K + 1) * B, B, size, x, t, text_embeds=te, text_mask=tm, extra_prompts=extra,
                            negative_text_embeds=neg[0], negative_text_mask=neg[1])
    assert torch.equal(outn[:K * B], out[:K * B])
    d = nerr(outn[K * B:], single(neg[0], neg[1].expand(B, -1)))
    print(f"K = {K}: null rows with a negative prompt vs the B-row forward on it {d} (bar 0)")
    assert d == 0.0
    with pytest.raises(AssertionError, match="extra_prompts"):
        eng.set_conditioning(keep=torch.ones((K + 1) * B, dtype=torch.bool), lowres_noise_times=None, text_embeds=te, text_mask=tm, extra_prompts=extra[:-1])


# ------------------------------------------------------------------------------------------------ 4. the recorded runs

def _group_call(name, which, dev="cpu"):
    grp, rec = fc.groups()[name], fc.runs_fixture()["groups"][name]
    steps = rec["steps"]
    model = fc.group_model(grp, dev, steps)
    kw = dict(fc.keywords(which, grp["stages"], dev), **fc.to_device(grp.get("sample", {}), dev),
              **({} if grp["sampler"] == "ddpm" else dict(sampler=grp["sampler"], sample_steps=steps)))
    return grp, rec, model, kw


@pytest.mark.parametrize("name,which", [(n, w) for n, grp in fc.groups().items() for w in grp["which"]])
def test_recorded_runs_through_the_interpreter(cpu_backend, name, which):
    """The recorded restatement — recomputed here and equal to the stored one the GPU tests read — against the driver, graph path and eager;
    every run >= 10 bars from its plain-CFG twin."""
    g = fs.cascade_fixture()
    grp, rec, model, kw = _group_call(name, which)
    want, twin, steps, n = rec["runs"][which], rec["twin"], rec["steps"], grp["stages"]
    assert nerr(want[-1], twin[-1]) > 10 * BAR, "the keyword must matter for this test to say anything"
    noise = fs.fixed_noise(rec["noise"])
    again = fc.compose_sample(fs.cascade_specs()[:n], grp.get("sizes", g["image_sizes"][:n]), g["text_embeds"], sampler=grp["sampler"], steps=steps,
                              cond_scale=fc.COND_SCALE, noise_fn=noise, return_all=True, **fc.settings()[which], **grp.get("restate", {}))
    assert all(torch.allclose(a, b, atol=1e-5) for a, b in zip(again, want)), "tests/golden/compose_runs.pt is stale"
    outs = model.sample(return_all_unet_outputs=True, **kw, **_common(g["text_embeds"], noise))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"{name}, {which} at {steps} steps vs the restatement: {errs}; vs the plain-CFG twin {[nerr(o, t) for o, t in zip(outs, twin)]}")
    assert [tuple(o.shape) for o in outs] == [tuple(w.shape) for w in want] and max(errs) < BAR, errs
    K, masked = len(fc.settings()[which]["compose"]) + 1, "mask" in which
    assert cpu_backend.composes and set(cpu_backend.composes) == {(K, masked)} and not cpu_backend.launches, "every step is COMPOSE_X0's, none CFG_X0's"
    eager = model.sample(use_graph=False, return_all_unet_outputs=True, **kw, **_common(g["text_embeds"], noise))
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))


# ------------------------------------------------------------------------------------------------ 5. cache reuse

def _labels(st):
    return [l for _, _, l in st["plan"].ops]


def test_weights_and_masks_are_per_call_state(cpu_backend):
    """A call without the keyword keeps its stages (keys of 16 entries, CFG_X0).  Composed calls of one (K, masks present) share ONE stage per
    unet and ONE plan, whatever their weights, cond_scale, masks and prompts: the key ends with (K, masks present) and the launch list is the
    plain one with COMPOSE_X0 where CFG_X0 stood and (K + 1) B engine rows."""
    g = fs.cascade_fixture()
    model = fs.cascade_model()
    noise = fs.memo_noise(3)
    kw = _common(g["text_embeds"], noise)
    a = model.sample(**kw)
    plain = dict(model._stages)
    assert len(plain) == 2 and all(len(k) == 16 for k in plain) and not cpu_backend.composes
    p, q = fc.prompt(61, scale=4.0), fc.prompt(62, batch=1, tokens=4, scale=4.0)
    b = model.sample(**kw, compose=[dict(text_embeds=p, weight=20.0)])
    new = {k: v for k, v in model._stages.items() if k not in plain}
    assert len(new) == 2 and all(k[-2:] == ("compose", (2, False)) for k in new), list(new)
    for st in new.values():
        assert st["eng"].R == 3 * 2 and st["compose"]["K"] == 2 and st["compose"]["masks"] is None
        (twin,) = [v for k, v in plain.items() if k[0] == st["key"][0]]
        ref = _labels(twin)
        i = ref.index("cfg_x0")
        got = _labels(st)
        assert got.count("compose_x0") == 1 and "cfg_x0" not in got and got[got.index("compose_x0") + 1:] == ref[i + 1:]
    plans = {k: (id(st["plan"]), id(st["graph"]), len(st["plan"])) for k, st in new.items()}
    c = model.sample(**{**kw, "cond_scale": 3.0}, compose=[dict(text_embeds=q, weight=(-5.0, 8.0))])
    d = model.sample(**kw, compose=[dict(text_embeds=p, weight=torch.tensor([20.0, 0.0]))])
    assert {k: (id(st["plan"]), id(st["graph"]), len(st["plan"])) for k, st in model._stages.items() if k not in plain} == plans, "one stage, one captured plan"
    assert nerr(b, a) > BAR and nerr(c, b) > BAR and nerr(d[0], b[0]) < 1e-6 and nerr(d[1], b[1]) > BAR, "the weights act per call and per sample"
    assert torch.equal(model.sample(**kw, compose=[dict(text_embeds=p, weight=20.0)]), b), "nothing of the calls in between is left behind"
    # sample 1 at further weight 0 is its plain-CFG image up to the fp16 rounding of another batch's tile configuration
    assert nerr(d[1], a[1]) < BAR
    # masks present: another stage (the kernel reads a mask buffer), shared by every mask
    m = fc.half_mask("left")
    e = model.sample(**kw, compose=[dict(text_embeds=p, weight=20.0, mask=m)])
    masked = {k: v for k, v in model._stages.items() if k not in plain and k not in new}
    assert len(masked) == 2 and all(k[-1] == (2, True) for k in masked)
    f = model.sample(**kw, compose=[dict(text_embeds=p, weight=20.0)], compose_mask=fc.half_mask("top", batch=2))
    assert len(model._stages) == 6 and nerr(e, b) > BAR and nerr(f, e) > BAR
    ones = model.sample(**kw, compose=[dict(text_embeds=p, weight=20.0, mask=torch.ones(1, 4, 4))])
    assert torch.equal(ones, b), "a mask of ones (resized to every stage) is no mask"
    assert torch.equal(model.sample(**kw), a), "the call without the keyword still meets its own stages"
    # skip_steps / init_images, stop_at / start_at
    comp = dict(compose=[dict(text_embeds=p, weight=20.0)])
    outs = model.sample(**kw, **comp, return_all_unet_outputs=True)
    assert torch.equal(outs[1], b)
    assert torch.equal(model.sample(**kw, **comp, stop_at_unet_number=1), outs[0])
    assert torch.equal(model.sample(**kw, **comp, start_at_unet_number=2, start_image_or_video=outs[0]), outs[1])
    init = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    s = model.sample(**kw, **comp, stop_at_unet_number=1, init_images=init, skip_steps=1)
    assert nerr(s, outs[0]) > BAR and len(model._stages) == 6


def test_self_cond_stage_composes(cpu_backend):
    g = fs.cascade_fixture()
    model = fs.single_stage_model(fs.selfcond_spec(), 16, "cpu", timesteps=4)
    noise = fs.memo_noise(8)
    kw = _common(g["text_embeds"], noise)
    a = model.sample(**kw)
    b = model.sample(**kw, compose=[dict(text_embeds=fc.prompt(63, scale=4.0), weight=20.0)])
    assert nerr(b, a) > BAR and cpu_backend.composes
    assert torch.equal(model.sample(**kw, compose=[dict(text_embeds=fc.prompt(63, scale=4.0), weight=20.0)]), b)


# ------------------------------------------------------------------------------------------------ 6. the other entry points

def test_pipelined_lanes_and_sharded(cpu_backend, monkeypatch):
    from imagen_pytorch_amd import distributed
    from imagen_pytorch_amd.distributed import sample_sharded, shard_compose

    g = fs.cascade_fixture()
    model = fs.cascade_model()
    te = g["text_embeds"]
    common = dict(cond_scale=fc.COND_SCALE, device="cpu")
    fns = [fs.memo_noise(11), fs.memo_noise(12)]
    comps = [dict(compose=[dict(text_embeds=fc.prompt(71, scale=4.0), weight=torch.tensor([20.0, -4.0]), mask=fc.half_mask("left", batch=2))]),
             dict(compose=[dict(text_embeds=fc.prompt(72, batch=1, scale=4.0), weight=(10.0, 20.0), mask=fc.half_mask("top"))], compose_mask=fc.half_mask("bottom", batch=2))]
    batches = [dict(text_embeds=te * s, noise_fn=fn, **c) for s, fn, c in zip((1.0, 0.9), fns, comps)]
    seq = [model.sample(use_tqdm=False, **common, **b) for b in batches]
    pipe = model.sample_pipelined(batches, **common)                       # compose is a per-batch key, as text_embeds is
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(pipe[0], pipe[1])
    with model.lane(3):
        assert torch.equal(model.sample(use_tqdm=False, **common, **batches[0]), seq[0])
    assert torch.equal(sample_sharded(model.sample, te, use_tqdm=False, noise_fn=fns[0], **common, **comps[0]), seq[0])
    # the slices a rank takes: per-sample rows are cut, batch-1 entries, [H, W] masks, floats and tuples go as they are
    emb, tm, w, m = fc.prompt(73, batch=4), torch.ones(4, 7, dtype=torch.bool), torch.arange(4.0), torch.rand(4, 8, 8)
    e1 = fc.prompt(74, batch=1)
    cut = shard_compose(1, 3, 4, [dict(text_embeds=emb, text_masks=tm, weight=w, mask=m), dict(text_embeds=e1, weight=(1.0, 2.0), mask=m[0]),
                                  dict(texts=["a", "b", "c", "d"], weight=2.0), dict(texts=["a"])], m)
    c0, c1, c2, c3 = cut["compose"]
    assert torch.equal(c0["text_embeds"], emb[1:3]) and torch.equal(c0["text_masks"], tm[1:3]) and torch.equal(c0["weight"], w[1:3]) and torch.equal(c0["mask"], m[1:3])
    assert c1["text_embeds"] is e1 and c1["weight"] == (1.0, 2.0) and torch.equal(c1["mask"], m[0])
    assert c2["texts"] == ["b", "c"] and c2["weight"] == 2.0 and c3["texts"] == ["a"] and torch.equal(cut["compose_mask"], m[1:3])
    assert shard_compose(0, 2, 4) == {}
    # two ranks: each rank's call is the slice of the whole batch's call
    calls = []
    monkeypatch.setattr(distributed.dist, "is_available", lambda: True)
    monkeypatch.setattr(distributed.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(distributed.dist, "get_world_size", lambda group=None: 2)
    for rank in (0, 1):
        monkeypatch.setattr(distributed.dist, "get_rank", lambda group=None, r=rank: r)
        sample_sharded(lambda **kw: calls.append(kw), te, gather=False, **comps[0])
    assert [c["sample_offset"] for c in calls] == [0, 1]
    full = comps[0]["compose"][0]
    for r, c in enumerate(calls):
        e = c["compose"][0]
        assert torch.equal(e["text_embeds"], full["text_embeds"][r:r + 1]) and torch.equal(e["weight"], full["weight"][r:r + 1]) and torch.equal(e["mask"], full["mask"][r:r + 1])


# ------------------------------------------------------------------------------------------------ 7. the kernel on the CPU emulation

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_kernel_cases_on_the_emulation():
    """csrc/sampler.hip compiled by tools/emul: every case of tests/test_compose_kernel_gpu.py in a child pytest on the emulated library
    (IMAGEN_EMUL_TESTS=1, as GUIDE_X0's cases run there)."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_compose_kernel_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
