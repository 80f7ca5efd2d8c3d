"""CPU: LinearCrossAttention on the HIP path (Unet(use_linear_cross_attn=...), ip.py:836-874; ABI 14: LINCTX, LINEAR_XATTN).

  * surface: the constructor rules of ip.py:1306, 1341, 1370, 1395, 1409 (the flag conditions the level's FIRST block, on the down and the up
    side, also where layer_cross_attns is False), strict state_dict loading, configs; `use_linear_attn` and both flags on Unet3D still raise;
  * the fp32 restatement of LinearCrossAttention.forward (tests/fixtures_linxattn.py) against the recorded output of the reference's module;
  * the planner: the dry-run launch lists of the fixture unets executed by the plan interpreter (tests/plan_interp.py), against the
    recorded forwards of the live reference (tests/golden/linxattn_unet*.pt) on both branches, 1e-2 as tests/test_plan_interp.py; the flag-off
    twin's launch list equals the one recorded from the commit before this feature (tests/golden/linxattn_twin_launch_list_abi13.json);
  * the two kernels on the functional emulation (tests/test_linear_xattn_gpu.py's kernel tests in a child pytest);
  * the real sample drivers replayed against tests/golden/linxattn_sample.pt through the interpreter.
    Measured here: planner lin64 cond / null 1.01e-3 / 1.40e-3, lin32 1.42e-3 / 6.2e-4 (the twin: 1.30e-3 / 1.41e-3); DDPM replay
    1.6e-3, Karras replay 2.6e-3; the restatement equals the reference's module bit for bit; emulated kernels: LINEAR_XATTN 2.1e-4 on every
    shape (the fp16 rounding of o), LINCTX <= 3.3e-7."""
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_linxattn as lx  # noqa: E402
from fixtures_linxattn import nerr  # noqa: E402
from plan_interp import Interpreter, register_engine, run_engine  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401  (the fixture that sends Plan.run / Graph to the interpreter)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TINY = dict(dim=16, cond_dim=16, text_embed_dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), max_text_len=16,
            attn_pool_num_latents=8, attn_heads=2)


@pytest.fixture()
def reference_weights():
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        yield ops
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


def run_unet(u, f):
    """One guided pair of `u` on the forward record f: (out_cond, out_null, engine)."""
    from imagen_pytorch_amd.engine import UnetEngine

    B, S = f["x"].shape[0], f["x"].shape[-1]
    return run_engine(UnetEngine(u, 2 * B, B, S, "cpu", dry=True), f["x"], f["time"], f["text_embeds"], f["text_mask"])[:3]


# ------------------------------------------------------------------------------------------------ 1. surface

def _sites(u):
    """{module path: linear?} of every cross-attention of the unet."""
    from imagen_pytorch_amd.modules import CrossAttentionP

    return {name: m.linear for name, m in u.named_modules() if isinstance(m, CrossAttentionP)}


def test_constructor_places_linear_sites():
    from imagen_pytorch_amd import Unet

    u = Unet(**TINY, use_linear_cross_attn=(True, False), layer_cross_attns=(False, True))
    assert _sites(u) == {"downs.0.1.cross_attn": True, "downs.1.1.cross_attn": False, "mid_block1.cross_attn": False,
                         "mid_block2.cross_attn": False, "ups.0.0.cross_attn": False, "ups.1.0.cross_attn": True}
    assert u.downs[0][2][0].cross_attn is None and u.ups[1][1][0].cross_attn is None      # only the first block of the level
    # a bool casts to every level, and wins over layer_cross_attns on the level's first block (ip.py:1370); the mid blocks stay full attention
    s = _sites(Unet(**TINY, use_linear_cross_attn=True, layer_cross_attns=(False, True)))
    assert all(v == (not k.startswith("mid_")) for k, v in s.items()) and len(s) == 6
    # flag off: nothing changes
    assert not any(_sites(Unet(**TINY, layer_cross_attns=(False, True))).values())
    with pytest.raises(AssertionError):
        Unet(**TINY, use_linear_cross_attn=(True, False, True))


def test_other_linear_flags_still_raise():
    from imagen_pytorch_amd import Unet, Unet3D

    with pytest.raises(NotImplementedError, match="use_linear_attn"):
        Unet(**TINY, use_linear_attn=True)
    with pytest.raises(NotImplementedError, match="use_linear_attn"):
        Unet(**TINY, use_linear_attn=(False, True), use_linear_cross_attn=True)
    for flag in ("use_linear_cross_attn", "use_linear_attn"):
        with pytest.raises(NotImplementedError, match=flag):
            Unet3D(dim=8, dim_mults=(1, 2), **{flag: True})


@pytest.mark.parametrize("name", ["lin64", "lin32"])
def test_reference_state_dict_loads_strictly(name):
    from imagen_pytorch_amd import Unet

    rec, sd = lx.unet_record(name)
    u = Unet(**rec["kwargs"])
    assert list(u.state_dict()) == list(sd), "state_dict keys, in the reference's order"
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in u.state_dict().items())
    res = u.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert "downs.0.1.cross_attn.q_scale" in sd and "downs.0.1.cross_attn.k_scale" in sd       # unused by the linear form, still parameters
    assert u.downs[0][1].cross_attn.linear and u.ups[1][0].cross_attn.linear


def test_config_with_the_flag_builds():
    from imagen_pytorch_amd.checkpoint import imagen_from_config

    unet = dict(TINY, attn_dim_head=32, layer_cross_attns=(False, True), use_linear_cross_attn=(True, False))
    imagen = imagen_from_config("original", dict(unets=[unet], image_sizes=(16,), timesteps=4, text_embed_dim=32))
    assert _sites(imagen.unets[0])["downs.0.1.cross_attn"] is True
    cfg, sd = imagen.unets[0].to_config_and_state_dict()
    again = type(imagen.unets[0]).from_config_and_state_dict(cfg, sd)
    assert _sites(again) == _sites(imagen.unets[0])


# ------------------------------------------------------------------------------------------------ 2. restatement

def test_restated_linear_cross_attention_matches_reference_module():
    rec, sd = lx.unet_record("lin64")
    s = rec["forward"]["site"]
    out = lx.linear_cross_attention(sd, s["module"] + ".", s["x"], s["context"], s["heads"])
    e = (out - s["out"]).abs().max().item()
    print(f"restated LinearCrossAttention.forward vs the reference's module: max abs {e:.2e} (|out| max {s['out'].abs().max():.2f})")
    assert e <= 2e-5 * max(1.0, s["out"].abs().max().item()), e
    # the same restatement in fp64 (what the kernel tests compare with) says the same
    e64 = (lx.linear_cross_attention(sd, s["module"] + ".", s["x"], s["context"], s["heads"], dtype=torch.float64).float() - s["out"]).abs().max().item()
    assert e64 <= 2e-5 * max(1.0, s["out"].abs().max().item()), e64


# ------------------------------------------------------------------------------------------------ 3. planner

@pytest.mark.parametrize("name", ["lin64", "lin32"])
def test_linear_unet_plan_on_cpu_matches_reference_fixture(name, reference_weights):
    from imagen_pytorch_amd import _abi

    rec, _ = lx.unet_record(name)
    f = rec["forward"]
    oc, on, eng = run_unet(lx.unet(name), f)
    e_c, e_n = nerr(oc, f["out_cond"]), nerr(on, f["out_null"])
    print(f"planner + interpreter [{name}] vs the reference: cond {e_c:.3e} null {e_n:.3e}")
    assert e_c < 1e-2 and e_n < 1e-2, (e_c, e_n)
    kinds = [k for k, _, _ in eng.step_plan.ops]
    labels = [l for _, _, l in eng.step_plan.ops]
    sites = [s for s in eng.attn_sites if s.kind == "linear"]
    assert [s.name for s in sites] == ["downs.0.1.cross_attn", "ups.1.0.cross_attn"]
    assert kinds.count(_abi.ENUMS["IMAGEN_OP_LINCTX"]) == 1, "ONE launch covers every linear site"
    assert kinds.count(_abi.ENUMS["IMAGEN_OP_LINEAR_XATTN"]) == len(sites)
    # M is ready before the first site reads it, and after the time tokens' rows are in place
    assert labels.index("ctx.dyn.linear_rows") < labels.index("linctx") < labels.index("downs.0.1.cross_attn.linear_attn")
    # per-pixel chain of a site: rowstat -> to_q -> LINEAR_XATTN -> to_out -> ln_residual
    i = labels.index("downs.0.1.cross_attn.norm")
    assert labels[i:i + 5] == ["downs.0.1.cross_attn" + s for s in (".norm", ".to_q", ".linear_attn", ".to_out", ".out_norm")]
    if name == "lin64":
        twin_f = lx.unet_record("twin")[0]["forward"]
        assert min(nerr(oc, twin_f["out_cond"]), nerr(on, twin_f["out_null"])) > 10 * 1e-2


def test_flag_off_launch_list_is_the_parent_commits(reference_weights):
    """The twin (flag off): op kinds and labels of the static and the step plan equal the lists recorded from the commit before this
    feature, and its output meets its own recording as before."""
    from imagen_pytorch_amd import _abi

    rec, _ = lx.unet_record("twin")
    f = rec["forward"]
    oc, on, eng = run_unet(lx.unet("twin"), f)
    want = json.load(open(os.path.join(lx.GOLDEN, "linxattn_twin_launch_list_abi13.json")))
    got = {"static": [[int(k), l] for k, _, l in eng._static_plans[f["text_embeds"].shape[1]][0].ops], "step": [[int(k), l] for k, _, l in eng.step_plan.ops]}
    assert got == want
    new = {_abi.ENUMS["IMAGEN_OP_LINCTX"], _abi.ENUMS["IMAGEN_OP_LINEAR_XATTN"]}
    assert not any(k in new for k, _ in got["static"] + got["step"])
    e_c, e_n = nerr(oc, f["out_cond"]), nerr(on, f["out_null"])
    print(f"planner + interpreter [twin] vs the reference: cond {e_c:.3e} null {e_n:.3e}")
    assert e_c < 1e-2 and e_n < 1e-2


def test_time_table_plan_equals_per_step_chain_with_linear_sites(reference_weights):
    """enable_time_table: the linear sites' projected time-token rows ride in the cross table, LINCTX runs behind STEP_SLICE, and the fast
    plan gives the bits of the per-step chain."""
    rec, _ = lx.unet_record("lin64")
    f = rec["forward"]
    oc, on, eng = run_unet(lx.unet("lin64"), f)
    B = f["x"].shape[0]
    coef = torch.zeros(3, 8)
    coef[:, 6] = torch.tensor([0.3, float(f["time"][0]), -0.8])
    step = torch.ones(1, dtype=torch.int32)
    fast = eng.enable_time_table(coef, step)
    assert fast is not None
    labels = [l for _, _, l in fast.ops]
    assert labels.index("time_table_rows") < labels.index("ctx.dyn.linear_rows") < labels.index("linctx")
    it = Interpreter()
    register_engine(it, eng)
    for buf in (coef, step):
        it.mem.register(buf)
    it.run(eng._tt_plan)
    eng.times.copy_(f["time"][:1].repeat(2 * B))        # both images at the time of table row 1
    it.run(eng.step_plan)
    want = eng.out.clone()
    eng.out.zero_()
    it.run(fast)
    assert torch.equal(eng.out, want)


# ------------------------------------------------------------------------------------------------ 4. the kernels, emulated

@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_kernels():
    """csrc/linear_xattn.hip compiled by tools/emul: the kernel tests of tests/test_linear_xattn_gpu.py (every shape, the sentinels, the
    saturated softmax, the launcher's refusals) in a child pytest on the emulated library."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_linear_xattn_gpu.py"), "-q", "-m", "gpu", "-k", "kernel or launcher",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
    assert int(out.split(" passed")[0].split()[-1]) == 9 + 1 + 1 + 4, out[-800:]


# ------------------------------------------------------------------------------------------------ 5. drivers

@pytest.mark.parametrize("kind,bar", [("ddpm", 2e-2), ("edm", 3e-2)])
def test_sample_driver_replay(cpu_backend, kind, bar):
    """Imagen.sample / ElucidatedImagen.sample over the lin64 unet through the real driver (time table, graph objects) and eager, against
    the recorded runs of the live reference with the same draws."""
    g = lx.sample_fixture()
    run = g["runs"][kind]
    model = lx.sample_model(kind)
    common = dict(text_embeds=g["text_embeds"], cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=lambda t, shape: run["noise"][t], device="cpu")
    out = model.sample(**common)
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    assert torch.equal(out, model.sample(use_graph=False, **common))
    e, far = nerr(out, run["outputs"][0]), nerr(out, run["outputs_twin"][0])
    print(f"linear cross-attention {kind} replay: {e:.2e}; from the flag-off twin's run {far:.2e}")
    assert e < bar and far > 10 * bar, (kind, e, far)
