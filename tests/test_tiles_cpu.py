"""CPU: tiled sampling of Imagen.sample (tile_shapes=, tile_overlap=, tile_blend=) and the TILES op.
  1. geometry and weights: the origin rule enumerated, every pixel covered, sum_t nw == 1 to 1 ulp, nw == 1.0 under single coverage, T as stated;
  2. ABI: kind 35 is an extension kind with its struct, ABI 15, KIND_COUNT 33, IMAGEN_OP_EXT_END 35, len(OP_STRUCT) == 32, "rebuild"; the launcher's
     refusals through the library's error path on the host; the default call's launch lists are the parent commit's;
  3. every refusal of the keywords, matched on its reason, before any launch;
  4. on the plan interpreter: T = 1 on every stage gives the bits of the call without the keywords; one stage and one graph serve any seed; the stage
     key differs by geometry; start / stop, init_images / skip_steps, sample_pipelined, lanes, sample_sharded;
  5. the recorded runs (tests/fixtures_tile.py, tests/golden/tile_runs.pt) against the driver, bar 2e-2, each >= 10 bars from its untiled twin;
  6. the kernel cases of tests/test_tiles_kernel_gpu.py on the CPU emulation of the kernel library."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_solver as fs  # noqa: E402
import fixtures_tile as ft  # noqa: E402
from fixtures_tile import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend as _replay_backend  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-2      # the project's bar of a sampled stage against its restatement (tests/test_compose_cpu.py, tests/test_solver_cpu.py)


@pytest.fixture()
def cpu_backend(_replay_backend, monkeypatch):  # noqa: F811
    """The replay backend of tests/test_sample_cpu_replay.py with the interpreter that knows TILES behind ops.Plan.run."""
    from imagen_pytorch_amd import ops
    from plan_interp_tile import TileInterpreter

    it = TileInterpreter()
    monkeypatch.setattr(ops.Plan, "run", lambda self, stream=None: it.run(self))
    return it


def _common(te, noise, **kw):
    return dict(text_embeds=te, cond_scale=ft.COND_SCALE, use_tqdm=False, noise_fn=noise, device="cpu", **kw)


# ------------------------------------------------------------------------------------------------ 1. geometry and weights

@pytest.mark.parametrize("L", [4, 8])
def test_origin_rule_and_weights(L):
    from imagen_pytorch_amd.sample_call import tile_geometry, tile_origins

    for N in range(L, 3 * L + 1):
        for o in range(L):
            s = L - o
            want = [v for v in range(0, 10 * N, s) if v < N - L] + [N - L]           # 0, s, 2 s, ... while < N - L, then N - L
            got = tile_origins(N, L, o)
            assert got == want == ft.restated_origins(N, L, o) and got == sorted(set(got)), (N, L, o, got)
            assert (len(got) == 1) == (N == L)
            cover = torch.zeros(N, dtype=torch.int32)
            for v in got:
                assert 0 <= v <= N - L
                cover[v:v + L] += 1
            assert bool((cover >= 1).all()), (N, L, o, "a pixel no tile covers")
    with pytest.raises(ValueError, match="larger than the canvas"):
        tile_origins(L - 1, L, 0)
    for o in (-1, L):
        with pytest.raises(ValueError, match="outside"):
            tile_origins(2 * L, L, o)
    # the weights, on a rectangular canvas with different overlaps per axis, both blends
    for blend in ("ramp", "uniform"):
        for (H, W), (oy, ox) in (((L, L), (1, 1)), ((2 * L + 1, 3 * L - 2), (L // 2, L // 4)), ((3 * L, 2 * L), (0, L - 1))):
            geo = tile_geometry(H, W, L, L, oy, ox, blend)
            ys, xs = tile_origins(H, L, oy), tile_origins(W, L, ox)
            assert geo["T"] == len(ys) * len(xs) == geo["Ty"] * geo["Tx"] and geo["origins"].tolist() == [[y, x] for y in ys for x in xs], "row-major, y outer"
            assert geo["nw"].dtype == torch.float32 and tuple(geo["nw"].shape) == (geo["T"], L * L) and geo["origins"].dtype == torch.int32
            total, count = torch.zeros(H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.int32)
            for t, (y0, x0) in enumerate(geo["origins"].tolist()):
                total[y0:y0 + L, x0:x0 + L] += geo["nw"][t].reshape(L, L).double()
                count[y0:y0 + L, x0:x0 + L] += 1
            assert bool((count >= 1).all())
            assert float((total - 1).abs().max()) <= 2.0 ** -23 * 1.0001, "sum_t nw == 1 to 1 ulp"
            for t, (y0, x0) in enumerate(geo["origins"].tolist()):
                m = count[y0:y0 + L, x0:x0 + L] == 1
                assert bool((geo["nw"][t].reshape(L, L)[m] == 1.0).all()), "exactly 1.0 where one tile covers the pixel"
            o2, w2 = ft.restated_weights(H, W, L, L, oy, ox, blend)
            assert [list(v) for v in o2] == geo["origins"].tolist() and torch.equal(w2.float().reshape(geo["T"], -1), geo["nw"])
    with pytest.raises(ValueError, match="tile_blend"):
        tile_geometry(8, 8, 4, 4, 1, 1, "cosine")


# ------------------------------------------------------------------------------------------------ 2. ABI, launch lists

def test_abi_is_15_and_kind_35_is_an_extension(monkeypatch):
    from imagen_pytorch_amd import _abi, engine
    from plan_interp_compose import ComposeInterpreter
    from plan_interp_tile import TileInterpreter

    assert _abi.ENUMS["IMAGEN_ABI_VERSION"] == 15 and _abi.ENUMS["IMAGEN_OP_KIND_COUNT"] == 33 and _abi.ENUMS["IMAGEN_OP_EXT_END"] == 35
    kind, st = _abi.ENUMS["IMAGEN_OP_TILES"], _abi.STRUCTS["ImagenTilesParams"]
    assert kind == 35 and _abi.ENUMS["IMAGEN_OP_EXT2_END"] == 36 and _abi.ENUMS["IMAGEN_TILE_MAX"] == 64
    assert kind not in _abi.OP_STRUCT and _abi.EXT_OP_STRUCT[kind] is st and _abi.STRUCT_KIND[st] == kind and len(_abi.OP_STRUCT) == 32
    assert [f for f, _ in st._fields_] == ["src", "dst", "absdst", "origins", "nw", "B", "C", "H", "W", "h", "w", "T", "mode"]
    assert set(TileInterpreter.DISPATCH) == set(ComposeInterpreter.DISPATCH) | {kind}
    lib = _abi.load_library()
    assert lib.imagen_sizeof(kind) == ctypes.sizeof(st) > 0
    _abi.require_ext_op(kind, "test")
    # a library from before the kind: refused with a message that says what to do, not a crash
    monkeypatch.setitem(_abi.EXT_OP_STRUCT, 9999, st)
    with pytest.raises(_abi.ImagenHipError, match="rebuild"):
        _abi.require_ext_op(9999, "tiles")
    # the launcher's refusals go through the library's error path, on the host, no GPU needed
    buf = (ctypes.c_float * 64)()

    def params(**kw):
        p = st()
        for f in ("src", "dst", "absdst", "origins", "nw"):
            setattr(p, f, ctypes.addressof(buf))
        p.B, p.C, p.H, p.W, p.h, p.w, p.T, p.mode = 1, 1, 4, 4, 2, 2, 4, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for kw, msg in ((dict(T=0), b"T outside"), (dict(T=65), b"T outside"), (dict(T=-1), b"T outside"), (dict(h=5), b"larger than the canvas"),
                    (dict(w=5), b"larger than the canvas"), (dict(B=0), b"non-positive"), (dict(C=0), b"non-positive"), (dict(H=-4), b"non-positive"),
                    (dict(W=0), b"non-positive"), (dict(h=0), b"non-positive"), (dict(w=-2), b"non-positive"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                    (dict(nw=None), b"nw == NULL"), (dict(src=None), b"required"), (dict(origins=None), b"required")):
        p = params(**kw)
        assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p), None) != 0 and msg in lib.imagen_last_error(), (kw, lib.imagen_last_error())
    p = params()
    assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p) - 4, None) != 0 and b"params struct" in lib.imagen_last_error()
    # the default call's launch lists are the parent commit's
    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))
    want = json.load(open(os.path.join(fs.GOLDEN, "solver_parent_launch_list_abi15.json")))
    assert fs.launch_lists() == want


def test_the_op_validates_before_it_adds():
    from imagen_pytorch_amd import ops

    canvas, rows, origins, nw = torch.zeros(1, 3, 8, 8), torch.zeros(2, 1, 3, 4, 4), torch.zeros(2, 2, dtype=torch.int32), torch.ones(2, 16)
    ok = dict(B=1, C=3, H=8, W=8, h=4, w=4, mode="blend", nw=nw)
    for kw, msg in ((dict(mode="sum"), "mode"), (dict(h=9), "no larger"), (dict(B=0), "positive"), (dict(nw=None), "nw"), (dict(nw=torch.ones(3, 16)), "nw"),
                    (dict(nw=nw.double()), "nw"), (dict(C=4), "elements"), (dict(H=16), "elements")):
        plan = ops.Plan()
        with pytest.raises(ValueError, match=msg):
            ops.tiles(plan, rows, canvas, origins, **{**ok, **kw})
        assert len(plan) == 0
    for bad, msg in ((origins.long(), "int32"), (torch.zeros(0, 2, dtype=torch.int32), "T = 0"), (torch.zeros(65, 2, dtype=torch.int32), "T = 65")):
        with pytest.raises(ValueError, match=msg):
            ops.tiles(ops.Plan(), rows, canvas, bad, **ok)


# ------------------------------------------------------------------------------------------------ 3. refusals

@pytest.fixture()
def no_launch(cpu_backend, monkeypatch):
    from imagen_pytorch_amd import ops

    def launched(self, stream=None):
        raise AssertionError(f"plan '{self.name}' was launched")
    monkeypatch.setattr(ops.Plan, "run", launched)


def test_refusals_come_before_any_launch(no_launch):
    from imagen_pytorch_amd import ElucidatedImagen, Imagen, Unet, Unet3D
    from imagen_pytorch_amd.distributed import sample_sharded
    from oracle.make_golden import ELUCIDATED_HP

    g = fs.cascade_fixture()
    model = fs.cascade_model(weights=False, timesteps=4)
    te = g["text_embeds"]
    base = dict(text_embeds=te, cond_scale=3.0, use_tqdm=False, device="cpu")
    tiled = dict(image_shapes=((16, 24), (32, 48)), tile_shapes=((16, 16), (32, 32)))       # (the refusals' own canvas: T = 2 per stage)
    known, keep = torch.rand(2, 3, 32, 32), torch.rand(2, 32, 32) > 0.5
    prompt = torch.randn(1, 7, 32)
    bad = (
        (dict(tiled, inpaint_images=known, inpaint_masks=keep), "inpainting"),
        (dict(tiled, compose=[dict(text_embeds=prompt)]), "tile_shapes with compose"), (dict(tiled, guidance_rescale=0.5), "per-tile sums"),
        (dict(tiled, guidance_apg={}), "per-tile sums"), (dict(tiled, guidance_interval=(0.2, 0.8)), "guidance_interval"),
        (dict(tiled, guidance_schedule=[3.0, 1.0, 3.0, 3.0]), "unguided steps"),
        (dict(image_shapes=((16, 24), (32, 48)), tile_shapes=((16, 32), None)), r"tile_shapes\[0\] = 16 x 32 is larger than the canvas of unet 1, 16 x 24"),
        (dict(tile_shapes=(32, 32)), "larger than the canvas"), (dict(tile_shapes=64), "larger than the canvas"),
        (dict(image_shapes=((16, 16), (256, 256)), tile_shapes=(None, 16), tile_overlap=0), "256 tiles"),
        (dict(tiled, tile_overlap=16), r"outside \[0, 16\)"), (dict(tiled, tile_overlap=-1), r"outside \[0, 16\)"),
        (dict(tiled, tile_overlap=((4, 16), None)), r"16 along x is outside \[0, 16\)"),
        (dict(tiled, tile_blend="cosine"), "tile_blend"), (dict(tile_overlap=4), "without tile_shapes"), (dict(tile_blend="uniform"), "without tile_shapes"),
        (dict(tiled, tile_shapes=((16, 16), (32, 32), (64, 64))), "3 entries for 2 unets"), (dict(tiled, tile_shapes="16"), "tile_shapes"),
        (dict(tiled, tile_shapes=((16.0, 16), None)), r"tile_shapes\[0\]"), (dict(tiled, tile_shapes=((15, 16), None)), "multiples"),
        (dict(tiled, tile_overlap=(4.5, None)), r"tile_overlap\[0\]"),
    )
    for kw, msg in bad:
        kw = {**base, **kw}
        with pytest.raises(ValueError, match=msg):
            model.sample(**kw)
        rest = {k: v for k, v in kw.items() if k not in ("text_embeds", "use_tqdm")}
        with pytest.raises(ValueError, match=msg):
            model.sample_pipelined([dict(text_embeds=te)], **rest)
        with pytest.raises(ValueError, match=msg):
            sample_sharded(model.sample, te, **{k: v for k, v in kw.items() if k != "text_embeds"})
    # an engine row count the engine refuses: 2 T B rows x 8 heads beyond a launch axis
    big = torch.zeros(300, 7, 32)
    with pytest.raises(ValueError, match="engine rows"):
        model.sample(text_embeds=big, cond_scale=3.0, use_tqdm=False, device="cpu", image_shapes=((16, 16), (128, 128)), tile_shapes=(None, 16), tile_overlap=0)
    # a conditioning handle; merged requests, inside and beside
    handle = model.prepare_conditioning(text_embeds=te, device="cpu")
    with pytest.raises(ValueError, match="conditioning"):
        model.sample(conditioning=handle, cond_scale=3.0, use_tqdm=False, device="cpu", **tiled)
    with pytest.raises(ValueError, match="sample_requests"):
        model.sample_requests([dict(text_embeds=te, tile_shapes=16)], cond_scale=3.0, device="cpu")
    with pytest.raises(ValueError, match="sample_requests"):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", **tiled)
    with pytest.raises(ValueError, match="sample_requests"):
        model.sample_requests([dict(text_embeds=te)], cond_scale=3.0, device="cpu", tile_blend="uniform")
    # self-conditioning unets, unets with conditioning images, a Unet3D stage, ElucidatedImagen
    unets = lambda **kw: [Unet(**{**u["kwargs"], **kw}).eval() for u in g["unets"]]
    selfc = Imagen(unets(self_cond=True), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.1).eval()
    with pytest.raises(ValueError, match="self-conditions"):
        selfc.sample(**base, **tiled)
    condi = Imagen(unets(cond_images_channels=3), image_sizes=g["image_sizes"], timesteps=4, text_embed_dim=32, cond_drop_prob=0.1).eval()
    with pytest.raises(ValueError, match="cond_images"):
        condi.sample(**base, **tiled, cond_images=torch.rand(2, 3, 16, 16))
    v = fs.load("sample_tiny_video.pt")
    video = fs.video_model("cpu", timesteps=4)
    assert isinstance(video.unets[0], Unet3D)
    with pytest.raises(ValueError, match="Unet3D"):
        video.sample(text_embeds=v["text_embeds"], video_frames=v["frames"], cond_scale=3.0, use_tqdm=False, device="cpu", tile_shapes=8)
    edm = ElucidatedImagen(unets(), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **ELUCIDATED_HP)
    with pytest.raises(ValueError, match="ElucidatedImagen"):
        edm.sample(**base, tile_shapes=16)
    with pytest.raises(ValueError, match="ElucidatedImagen"):
        edm.sample_pipelined([dict(text_embeds=te)], cond_scale=3.0, device="cpu", tile_overlap=4)
    for m in (model, selfc, condi, video, edm):
        assert not m._stages
    # what resolves: None for every stage the call runs is the untiled call; the default overlap is a quarter of the side
    resolve = lambda **kw: model._resolve(model._call(**{**base, **kw})).tiles
    assert resolve() is None and resolve(tile_shapes=(None, None)) is None and resolve(tile_shapes=((16, 16), None), start_at_unet_number=2,
                                                                                      start_image_or_video=torch.rand(2, 3, 16, 16)) is None
    t = resolve(**tiled)
    assert [(s["h"], s["w"], s["oy"], s["ox"], s["T"], s["blend"]) for s in t] == [(16, 16, 4, 4, 2, "ramp"), (32, 32, 8, 8, 2, "ramp")]
    t = resolve(image_shapes=((16, 24), (32, 48)), tile_shapes=(None, 16), tile_overlap=(None, (8, 0)), tile_blend="uniform")
    assert t[0] is None and (t[1]["Ty"], t[1]["Tx"], t[1]["T"], t[1]["blend"]) == (3, 3, 9, "uniform")
    assert resolve(image_shapes=((16, 24), (32, 48)), tile_shapes=(16, 16), stop_at_unet_number=1)[0]["T"] == 2, "a pair of ints is ONE tile shape"


# ------------------------------------------------------------------------------------------------ 4. on the plan interpreter

def _labels(st):
    return [l for _, _, l in st["plan"].ops]


@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
def test_one_tile_is_the_untiled_call(cpu_backend, sampler):
    """T = 1 on every stage: the gather is a copy, the blend multiplies by 1.0f, so the images have the bits of the call without the keywords; the
    stages are others (their key ends with the geometry), and their launch lists are the plain ones with the two TILES launches around the
    denoiser and CFG_X0."""
    g = fs.cascade_fixture()
    model = fs.cascade_model(timesteps=4)
    noise = fs.memo_noise(11)
    kw = _common(g["text_embeds"], noise, **({} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=5)))
    a = model.sample(return_all_unet_outputs=True, **kw)
    plain = dict(model._stages)
    assert len(plain) == 2 and not cpu_backend.tiles
    b = model.sample(return_all_unet_outputs=True, tile_shapes=((16, 16), 32), tile_overlap=(3, (5, 0)), **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    new = {k: v for k, v in model._stages.items() if k not in plain}
    assert len(new) == 2 and [k[-1] for k in sorted(new, key=lambda k: k[0])] == [("tile", ((16, 16), (3, 3), "ramp")), ("tile", ((32, 32), (5, 0), "ramp"))]
    assert cpu_backend.tiles and set(cpu_backend.tiles) == {(0, 1), (1, 1)}
    for st in new.values():
        (twin,) = [v for k, v in plain.items() if k[0] == st["key"][0]]
        ref, got = _labels(twin), _labels(st)
        i = ref.index("cfg_x0")
        assert got == ["tiles.gather"] + ref[:i + 1] + ["tiles.blend"] + ref[i + 1:]
        assert st["eng"].R == twin["eng"].R and st["x"] is not st["eng"].x_in and twin["x"] is twin["eng"].x_in
    assert torch.equal(model.sample(**kw), a[-1]), "the call without the keywords still meets its own stages"
    assert torch.equal(model.sample(tile_shapes=((16, 16), 32), tile_blend="uniform", **kw), a[-1]) and len(model._stages) == 6, "the blend is part of the key"


def test_stage_graph_and_key(cpu_backend):
    """One stage and one captured plan serve any seed and prompt; the key ends with (tile shape, overlap, blend), so another geometry is another
    stage; cond_scale 1 runs T B rows; start / stop, init_images / skip_steps; sample_pipelined, lanes, sample_sharded."""
    from imagen_pytorch_amd.distributed import sample_sharded

    g = fs.cascade_fixture()
    TWO = ((16, 16), (32, 32))
    model = fs.cascade_model()
    te = g["text_embeds"]
    tiled = dict(image_shapes=((16, 24), (32, 48)), tile_shapes=TWO, tile_overlap=((8, 8), (16, 16)), sampler="dpmpp_2m", sample_steps=3)    # T = 2 per stage
    kw = dict(text_embeds=te, cond_scale=ft.COND_SCALE, use_tqdm=False, device="cpu", **tiled)
    a = model.sample(seed=5, return_all_unet_outputs=True, **kw)
    assert [tuple(o.shape) for o in a] == [(2, 3, 16, 24), (2, 3, 32, 48)]
    stages = dict(model._stages)
    ids = {k: (id(st["plan"]), id(st["graph"]), len(st["plan"])) for k, st in stages.items()}
    assert len(stages) == 2 and all(st["eng"].R == 2 * 2 * 2 and st["eng"].src_batch == 4 and st["eng"].HW == hw for st, hw in
                                    zip(sorted(stages.values(), key=lambda s: s["key"][0]), TWO))
    b = model.sample(seed=6, **kw)
    c = model.sample(seed=5, **{**kw, "text_embeds": te.flip(0)})
    assert {k: (id(st["plan"]), id(st["graph"]), len(st["plan"])) for k, st in model._stages.items()} == ids, "one stage, one captured plan"
    assert nerr(b, a[-1]) > BAR and nerr(c, a[-1]) > 1e-4 and torch.equal(model.sample(seed=5, **kw), a[-1])
    model.sample(seed=5, **{**kw, "tile_overlap": ((8, 4), (16, 16))})
    assert len(model._stages) == 3, "another overlap on stage 1: one more stage, stage 2's is shared"
    model.sample(seed=5, **{**kw, "cond_scale": 1.0}, stop_at_unet_number=1)
    (unguided,) = [st for k, st in model._stages.items() if k not in stages and k[4] == 1.0]
    assert unguided["eng"].R == 2 * 2 and "tiles.blend" in _labels(unguided)
    n = len(model._stages)
    # start / stop, init_images / skip_steps
    assert torch.equal(model.sample(seed=5, stop_at_unet_number=1, **kw), a[0])
    assert torch.equal(model.sample(seed=5, start_at_unet_number=2, start_image_or_video=a[0], **kw), a[1])
    init = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(1))
    s = model.sample(seed=5, stop_at_unet_number=1, init_images=init, skip_steps=1, **kw)
    assert nerr(s, a[0]) > BAR and len(model._stages) == n
    # sample_pipelined (a per-batch key), lanes, sample_sharded
    rest = {k: v for k, v in kw.items() if k not in ("text_embeds", "tile_shapes")}
    outs = model.sample_pipelined([dict(text_embeds=te, seed=5, tile_shapes=TWO), dict(text_embeds=te, seed=6, tile_shapes=TWO)], **rest)
    assert torch.equal(outs[0], a[-1]) and torch.equal(outs[1], b)
    with model.lane(3):
        assert torch.equal(model.sample(seed=5, **kw), a[-1])
    assert torch.equal(sample_sharded(model.sample, te, seed=5, **{k: v for k, v in kw.items() if k != "text_embeds"}), a[-1])
    lo = model.sample(seed=5, sample_offset=1, **{**kw, "text_embeds": te[1:]})
    assert nerr(lo, a[-1][1:]) < BAR, "a shard's rows are the whole batch's up to the rounding of another batch's tile configuration"


# ------------------------------------------------------------------------------------------------ 5. the recorded runs

@pytest.mark.parametrize("name", list(ft.groups()))
def test_recorded_runs_through_the_interpreter(cpu_backend, name):
    """The recorded restatement — recomputed here and equal to the stored one the GPU tests read — against the driver, graph path and eager;
    every run >= 10 bars from its untiled twin, which the driver meets through image_shapes alone."""
    g = fs.cascade_fixture()
    grp, rec = ft.groups()[name], ft.runs_fixture()["groups"][name]
    want, twin, steps = rec["run"], ft.twins_fixture()[name], rec["steps"]
    assert min(nerr(w, t) for w, t in zip(want, twin)) > 10 * BAR, "the keywords must matter on every stage for this test to say anything"
    noise = fs.fixed_noise(ft.noise_fixture())
    again = ft.restate(grp, steps, noise)
    assert all(torch.allclose(a, b, atol=1e-5) for a, b in zip(again, want)), "tests/golden/tile_runs.pt is stale"
    model = ft.group_model(grp, "cpu", steps)
    outs = model.sample(return_all_unet_outputs=True, **ft.keywords(grp, steps), **_common(g["text_embeds"], noise))
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    print(f"{name} at {steps} steps vs the restatement: {errs}; vs the untiled twin {[nerr(o, t) for o, t in zip(outs, twin)]}")
    assert [tuple(o.shape) for o in outs] == [tuple(w.shape) for w in want] and max(errs) < BAR, errs
    T = [len(ft.restated_weights(*hw, *t, *o, "ramp")[0]) for hw, t, o in zip(ft.SHAPES, ft.TILES, ft.OVERLAPS)]
    assert set(cpu_backend.tiles) == {(m, t) for m in (0, 1) for t in T}
    eager = model.sample(use_graph=False, return_all_unet_outputs=True, **ft.keywords(grp, steps), **_common(g["text_embeds"], noise))
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    assert min(nerr(o, t) for o, t in zip(outs, twin)) > 10 * BAR, "every tiled stage lies >= 10 bars from the untiled twin's"
    plain = model.sample(return_all_unet_outputs=True, **ft.keywords(grp, steps, tiled=False), **_common(g["text_embeds"], noise))
    assert max(nerr(p, t) for p, t in zip(plain, twin)) < BAR, "the twin is the untiled call"


# ------------------------------------------------------------------------------------------------ 6. the kernel on the CPU emulation

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_kernel_cases_on_the_emulation():
    """csrc/tiles.hip compiled by tools/emul: every case of tests/test_tiles_kernel_gpu.py in a child pytest on the emulated library
    (IMAGEN_EMUL_TESTS=1, as COMPOSE_X0's cases run there)."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_tiles_kernel_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and " passed" in out and "skipped" not in out and "failed" not in out, out[-3000:]
