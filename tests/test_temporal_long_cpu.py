"""CPU: clips of 33 .. 128 frames (ABI 15: TEMPORAL_ATTENTION takes F <= 128; csrc/temporal.hip temporal_attention_long_kernel).

  * the tiled kernel on the functional emulation: the kernel, launcher and causal tests of tests/test_temporal_long_gpu.py in a child pytest
    on the emulated library (every case, F = 128 included: the slowest takes about two seconds);
  * the planner: the dry-run launch lists of `long` / `long32` (36 frames: level 0 on the tiled kernel, level 1 at 18 frames) executed by the
    plan interpreter against the recorded forwards of the live reference, bar = 1.5 x the twin's larger figure measured the same way;
  * both sample drivers replayed through the interpreter against the recorded runs (the bars of tests/test_selfcond_gpu.py);
  * a short-clip video config builds the launch lists it built before the change (tests/golden/longclip_short_launch_list_abi14.json,
    recorded from the parent commit by tools/make_longclip_golden.py --launch-list);
  * the host bound: an engine for 128 frames builds dry, 129 frames is refused with the bound in the message."""
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_longclip as lc  # noqa: E402
from fixtures_longclip import nerr  # noqa: E402
from plan_interp import run_engine  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture()
def reference_weights():
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        yield ops
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_long_kernel():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_temporal_long_gpu.py"), "-q", "-m", "gpu", "-k",
                        "long_kernel or launcher", "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    print(out[-3000:])
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
    assert int(out.split(" passed")[0].split()[-1]) == 40 + 4 + 2 + 2, out[-800:]


_figures = {}


def _forward(name):
    if name not in _figures:
        from imagen_pytorch_amd.engine3d import UnetEngine3D

        f, _, _ = lc.unet_record(name)
        B, _, Fr, S, _ = f["x"].shape
        oc, on, eng, _ = run_engine(UnetEngine3D(lc.unet(name), 2 * B, B, Fr, S, "cpu", dry=True), f["x"], f["time"], f["text_embeds"], f["text_mask"])
        _figures[name] = (nerr(oc, f["out_cond"]), nerr(on, f["out_null"]), eng)
    return _figures[name]


@pytest.mark.parametrize("name", ["long", "long32"])
def test_long_unet3d_plan_on_cpu_matches_reference_fixture(name, reference_weights):
    from imagen_pytorch_amd import _abi

    t_c, t_n, _ = _forward("twin")
    e_c, e_n, eng = _forward(name)
    bar = 1.5 * max(t_c, t_n)
    print(f"planner + interpreter [{name}] 36 frames vs the reference: cond {e_c:.3e} null {e_n:.3e}; twin (16 frames) cond {t_c:.3e} null {t_n:.3e}; bar {bar:.3e}")
    frames = sorted({p.F for k, p, _ in eng.step_plan.ops if k == _abi.ENUMS["IMAGEN_OP_TEMPORAL_ATTENTION"]})
    assert frames == [18, 36], frames          # one forward mixes the tiled kernel and the kernels of before
    assert max(e_c, e_n) <= bar, (e_c, e_n, bar)


@pytest.mark.parametrize("kind,bar", [("ddpm", 2e-2), ("edm", 5e-2)])
def test_long_sample_driver_replay(cpu_backend, kind, bar):
    g = lc.sample_fixture()
    run = g[kind]
    model = lc.sample_model(kind)
    out = model.sample(text_embeds=g["text_embeds"], video_frames=g["frames"], cond_scale=g["cond_scale"], use_tqdm=False,
                       noise_fn=lambda t, shape: run["noise"][t], device="cpu")
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    e = nerr(out, run["outputs"][0])
    far = nerr(out[:, :, :g["short_frames"]], run["outputs_short"][0])
    print(f"long-clip {kind} replay: {e:.2e} (bar {bar:.0e}); first {g['short_frames']} frames vs the recorded short run {far:.3f}")
    assert e < bar, (kind, e)


def test_short_clip_launch_list_is_the_parent_commits():
    """The 'base' clip of tests/golden/unet3d_tiny.pt (4 frames): op kinds and labels of both plans equal the recording of the commit before."""
    from imagen_pytorch_amd import Unet3D
    from imagen_pytorch_amd.engine3d import UnetEngine3D

    g = torch.load(os.path.join(lc.GOLDEN, "unet3d_tiny.pt"), weights_only=False)["runs"]["base"]
    u = Unet3D(**g["kwargs"]).eval()
    u.load_state_dict(g["state_dict"])
    B, _, Fr, size, _ = g["x"].shape
    eng = UnetEngine3D(u, 2 * B, B, Fr, size, "cpu", dry=True)
    eng.set_conditioning(text_embeds=g["text_embeds"], text_mask=g["text_mask"], keep=torch.tensor([True] * B + [False] * B), lowres_noise_times=None)
    want = json.load(open(os.path.join(lc.GOLDEN, "longclip_short_launch_list_abi14.json")))
    assert lc.launch_list(eng, g["text_embeds"].shape[1]) == want


def test_engine_frame_bound():
    from imagen_pytorch_amd.engine3d import UnetEngine3D

    u = lc.unet("long")
    eng = UnetEngine3D(u, 2, 1, 128, 8, "cpu", dry=True)
    assert eng.F == 128
    with pytest.raises(AssertionError, match="128 frames"):
        UnetEngine3D(u, 2, 1, 129, 8, "cpu", dry=True)
