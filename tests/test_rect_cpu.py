"""CPU: rectangular images (H != W) — Unet.forward on any H x W the down path divides, Imagen.sample / ElucidatedImagen.sample with
`image_shapes=` (no ABI change: the kernel structs carry H and W since the first round).

  * surface: a 16x24 forward no longer asserts (on the CPU it reaches "no CPU path", as a square call does); a side the downsamples do not
    divide raises ValueError naming the divisor; one case per `image_shapes` rule, raised before anything is built;
  * the planner: the dry-run launch lists of the fixture unets at every recorded shape, BOTH orientations, executed by the plan interpreter
    against the recorded forwards of the live reference (tests/golden/rect_forward_*.pt) on both branches, at the 1e-2 of
    tests/test_plan_interp.py; every record lies >= 10 bars from the same unet's output on the centre-cropped square input;
  * the real sample drivers replayed through the interpreter against tests/golden/rect_sample_*.pt at the bars of
    tests/test_sample_cpu_replay.py (2e-2 DDPM, 3e-2 Karras): cascade in both orientations, negative prompt, init_images / skip_steps,
    inpainting, Karras; graph == eager bit for bit;
  * no regression: an engine of (S, S) has the launch list of the engine of S; ops.small_tile answers what it answered for the square maps,
    and a ragged block only where it answered None and the map is not square;
  * conv_small on the ragged blocks, emulated: the contract cases of tests/test_rect_gpu.py in a child pytest on the emulated library.
    The measured figures are printed by each test (planner + interpreter vs the reference; replays per stage)."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_rect as fr  # noqa: E402
from fixtures_rect import FORWARD_BAR, SAMPLE_BAR, crop, nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401  (the fixture that sends Plan.run / Graph to the interpreter)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TINY = dict(dim=16, dim_mults=(1, 2), num_resnet_blocks=1, attn_heads=2, layer_attns=(False, True), layer_cross_attns=(False, True), cond_dim=32,
            text_embed_dim=32, attn_pool_num_latents=8, max_text_len=16)


@pytest.fixture()
def reference_weights():
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        yield ops
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


# ------------------------------------------------------------------------------------------------ 1. surface

def test_rectangular_forward_reaches_the_engine():
    """Fails before this feature with `square images only`."""
    from imagen_pytorch_amd import Unet

    u = Unet(**TINY).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        u(torch.zeros(1, 3, 16, 24), torch.zeros(1), text_embeds=torch.zeros(1, 4, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        u(torch.zeros(1, 3, 16, 16), torch.zeros(1), text_embeds=torch.zeros(1, 4, 32))


@pytest.mark.parametrize("kw,hw,div", [(TINY, (16, 23), 2), (TINY, (17, 24), 2), (dict(TINY, memory_efficient=True), (16, 18), 4),
                                       (dict(TINY, dim_mults=(1, 2, 2, 4), layer_attns=False, layer_cross_attns=(False, False, False, True)), (32, 44), 8)])
def test_bad_divisor_raises(kw, hw, div):
    from imagen_pytorch_amd import Unet

    u = Unet(**kw).eval()
    assert u.size_divisor == div
    with pytest.raises(ValueError, match=f"multiples of {div}"):
        u(torch.zeros(1, 3, *hw), torch.zeros(1), text_embeds=torch.zeros(1, 4, 32))


def test_unet3d_keeps_square_frames():
    import inspect

    from imagen_pytorch_amd import unet3d

    assert "'square frames only'" in inspect.getsource(unet3d)


@pytest.mark.parametrize("shapes,msg", [(((16, 24),), "2 unets"), (((16, 23), (32, 48)), "multiples of 2"), (((16, 24), (32, 20)), "smaller than"),
                                        ((16, (32, 48)), r"an \(H, W\) pair")])
def test_image_shapes_rules(cpu_backend, shapes, msg):
    model = fr.sample_model("ddpm")
    built = len(model._stages)
    with pytest.raises(ValueError, match=msg):
        model.sample(text_embeds=torch.zeros(1, 4, 32), image_shapes=shapes, device="cpu", use_tqdm=False)
    assert len(model._stages) == built, "refused before a stage is built"


def test_image_shapes_on_a_video_cascade_raises(cpu_backend):
    from imagen_pytorch_amd import Imagen, Unet3D

    model = Imagen((Unet3D(dim=8, dim_mults=(1, 2), text_embed_dim=32),), image_sizes=(16,), timesteps=2, text_embed_dim=32).eval()
    with pytest.raises(ValueError, match="video cascade"):
        model.sample(text_embeds=torch.zeros(1, 4, 32), video_frames=4, image_shapes=((16, 24),), device="cpu", use_tqdm=False)


def test_square_image_shapes_meet_the_square_stage(cpu_backend):
    """image_shapes = ((S, S), ...) is the call without it: same stage keys, same bits."""
    g, kw = fr.run_kwargs("ddpm")
    draw = lambda tag, shape: torch.randn(shape, generator=torch.Generator().manual_seed(sum(map(ord, str(tag)))))
    kw.update(image_shapes=None, noise_fn=draw, max_steps=1, device="cpu")
    model = fr.sample_model("ddpm")
    a = model.sample(**kw)
    keys = set(model._stages)
    b = model.sample(**dict(kw, image_shapes=((16, 16), (32, 32))))
    assert set(model._stages) == keys and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 2. planner

def run_unet(u, f, size=None):
    from imagen_pytorch_amd.engine import UnetEngine
    from plan_interp import run_engine

    B = f["x"].shape[0]
    eng = UnetEngine(u, 2 * B, B, tuple(f["x"].shape[-2:]) if size is None else size, "cpu", dry=True)
    return run_engine(eng, f["x"], f["time"], f["text_embeds"], f["text_mask"], **fr.low_kw(f))[:3]


@pytest.mark.parametrize("name,shape", fr.forward_cases())
def test_unet_plan_on_cpu_matches_reference_fixture(name, shape, reference_weights):
    f = fr.forward_records(name)[shape]
    H, W = (int(v) for v in shape.split("x"))
    assert tuple(f["x"].shape[-2:]) == (H, W) and H != W
    for branch in ("out_cond", "out_null"):      # the separation check: a plan that ignored the extra columns would not pass below
        assert nerr(crop(f[branch]), f[branch + "_crop"].float()) >= 10 * FORWARD_BAR
    oc, on, eng = run_unet(fr.unet(name), f)
    assert tuple(oc.shape) == tuple(f["out_cond"].shape) and eng.HW == (H, W)
    e_c, e_n = nerr(oc, f["out_cond"]), nerr(on, f["out_null"])
    print(f"planner + interpreter [{name} {shape}] vs the reference: cond {e_c:.3e} null {e_n:.3e}")
    assert e_c < FORWARD_BAR and e_n < FORWARD_BAR, (e_c, e_n)


def test_both_orientations_are_recorded():
    for name in fr.FORWARD_UNETS:
        shapes = {tuple(int(v) for v in k.split("x")) for k in fr.forward_records(name)}
        assert any((w, h) in shapes for h, w in shapes), name


def test_rectangular_levels_reach_conv_small():
    """four_sr at 64x96 (8 / 16 / 32 / 32 channels): its 16x24 and 8x12 levels — the measured maps of ops.SMALL_RAGGED_MAPS — launch family 8
    on 4 x 8 blocks; with the switch off none does."""
    from imagen_pytorch_amd import _abi, ops
    from imagen_pytorch_amd.engine import UnetEngine

    K = _abi.ENUMS
    fam = lambda p: ops.cfg_table()[p.cfg][3]

    def tiles(flag):
        keep, ops.SMALL_RAGGED = ops.SMALL_RAGGED, flag
        try:
            eng = UnetEngine(fr.unet("four_sr"), 2, 1, (64, 96), "cpu", dry=True)
        finally:
            ops.SMALL_RAGGED = keep
        return {(p.OH, p.OW): (p.TH, p.TW) for k, p, _ in eng.step_plan.ops if k == K["IMAGEN_OP_IGEMM"] and fam(p) == 8 and p.KH == 3}
    assert tiles(1) == {hw: (4, 8) for hw in ops.SMALL_RAGGED_MAPS if hw in ((16, 24), (8, 12))} and tiles(1)
    assert tiles(0) == {}


# ------------------------------------------------------------------------------------------------ 3. drivers

@pytest.mark.parametrize("run", fr.RUNS)
def test_sample_driver_replay(cpu_backend, run):
    g, kw = fr.run_kwargs(run)
    r = g["run"]
    bar = SAMPLE_BAR[r["kind"]]
    assert r["bar"] == bar and min(nerr(crop(a), b.float()) for a, b in zip(r["outputs"], r["outputs_square"])) >= 10 * bar
    model = fr.sample_model(r["kind"])
    outs = model.sample(device="cpu", **kw)
    assert [tuple(o.shape) for o in outs] == [tuple(o.shape) for o in r["outputs"]] == [(2, 3, *s) for s in r["image_shapes"]]
    eager = model.sample(device="cpu", use_graph=False, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    errs = [nerr(o, ref) for o, ref in zip(outs, r["outputs"])]
    print(f"rectangular {run} replay per stage: {['%.2e' % e for e in errs]}")
    assert max(errs) < bar, (run, errs)


def test_start_image_and_stop_at_unet(cpu_backend):
    """start_image_or_video at the first stage's rectangular size feeds the second stage what the cascade hands it."""
    g, kw = fr.run_kwargs("ddpm")
    model = fr.sample_model("ddpm")
    both = model.sample(device="cpu", **kw)
    kw.pop("return_all_unet_outputs")
    first = model.sample(device="cpu", stop_at_unet_number=1, **kw)
    second = model.sample(device="cpu", start_at_unet_number=2, start_image_or_video=first, **kw)
    assert torch.equal(first, both[0]) and torch.equal(second, both[1])


def test_square_stage_in_a_rectangular_cascade(cpu_backend):
    """image_shapes = ((16, 24), (24, 24)): the second stage is square, its 16x24 init image is resized on BOTH axes."""
    g, kw = fr.run_kwargs("init_skip")
    kw.update(image_shapes=((16, 24), (24, 24)), max_steps=1, noise_fn=lambda tag, shape: torch.randn(shape, generator=torch.Generator().manual_seed(len(str(tag)))))
    outs = fr.sample_model("ddpm").sample(device="cpu", **kw)
    assert [tuple(o.shape[-2:]) for o in outs] == [(16, 24), (24, 24)]


def test_return_pil_images(cpu_backend):
    g, kw = fr.run_kwargs("ddpm")
    kw.pop("return_all_unet_outputs")
    pil = fr.sample_model("ddpm").sample(device="cpu", return_pil_images=True, max_steps=1, **kw)
    assert [im.size for im in pil] == [(48, 32)] * 2      # PIL: (width, height)


# ------------------------------------------------------------------------------------------------ 4. no regression

@pytest.mark.parametrize("name,S", [("tiny", 16), ("tiny_sr", 32), ("four_sr", 64)])
def test_square_pair_builds_the_square_engine(name, S):
    from imagen_pytorch_amd import _abi
    from imagen_pytorch_amd.engine import UnetEngine

    K = _abi.ENUMS
    u = fr.unet(name)
    a, b = UnetEngine(u, 4, 2, S, "cpu", dry=True), UnetEngine(u, 4, 2, (S, S), "cpu", dry=True)
    assert a.S == b.S == S and a.HW == b.HW == (S, S)
    sig = lambda e: [(k, l, (p.TH, p.TW, p.cfg) if k == K["IMAGEN_OP_IGEMM"] else None) for k, p, l in e.step_plan.ops]
    assert sig(a) == sig(b)


def test_small_tile_answers():
    from imagen_pytorch_amd import ops

    assert [ops.small_tile(s, s) for s in (8, 16, 32, 64)] == [(4, 8), (2, 16), (1, 32), (1, 32)]
    assert [ops.small_tile(s, s) for s in (2, 4, 12, 24, 48)] == [None] * 5, "a square map keeps the launch it has"
    assert ops.small_tile(12, 8) == (4, 8) and ops.small_tile(24, 16) == (2, 16) and ops.small_tile(1, 96) == (1, 32)
    assert ops.small_tile(48, 32) == (1, 32) and ops.small_tile(1, 12) is None
    keep = ops.SMALL_RAGGED, ops.SMALL_RAGGED_MAPS
    try:
        for hw in ((8, 12), (16, 24), (32, 48), (4, 6), (6, 4), (12, 12)):      # the measured maps, and no other
            assert ops.small_tile(*hw) == ((4, 8) if hw in keep[1] else None), hw
        ops.SMALL_RAGGED_MAPS = ((32, 48), (4, 6))
        assert ops.small_tile(32, 48) == (4, 8) and ops.small_tile(6, 4) == (4, 8) and ops.small_tile(8, 12) is None
        ops.SMALL_RAGGED, ops.SMALL_RAGGED_MAPS = 0, keep[1]
        assert ops.small_tile(8, 12) is None and ops.small_tile(8, 8) == (4, 8)
    finally:
        ops.SMALL_RAGGED, ops.SMALL_RAGGED_MAPS = keep


# ------------------------------------------------------------------------------------------------ 5. the kernel, emulated

@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_ragged_blocks():
    """csrc/conv_small.hip compiled by tools/emul: the contract cases of tests/test_rect_gpu.py (batch 2) and its PACK_IMAGE / LOWRES_PREP
    cases in a child pytest on the emulated library."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_rect_gpu.py"), "-q", "-m", "gpu", "-k", "(ragged and B2) or pack or lowres",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
    assert int(out.split(" passed")[0].split()[-1]) == 6 + 2 + 3, out[-800:]
