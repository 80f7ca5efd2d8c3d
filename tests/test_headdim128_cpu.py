"""CPU: attention head dim 128 on the HIP path (Unet(attn_dim_head=128); no ABI change: ATTENTION / QNORM / KV_PREP / LINCTX / LINEAR_XATTN
take head_dim 128 in the structs they already have).

  * surface: the constructor, strict state_dict loading of the recorded reference parameters, the config round trip, imagen_from_config;
    48 and Unet3D(attn_dim_head=128) still raise;
  * the planner: the dry-run launch lists of the fixture unets (plain and linear cross-attention) executed by the plan interpreter, restated
    for a head dim the params carry (tests/fixtures_headdim128.py), against the recorded forwards of the live reference
    (tests/golden/headdim128_forward.pt) on both branches, at the 1e-2 of the head-dim-32 planner tests (tests/test_linear_xattn_cpu.py);
    no ROWCHAIN launch at head dim 128, the mid blocks (8 x 64) ride in the same KV_PREP_MULTI launch as the 128-wide sites;
  * the real sample drivers replayed against tests/golden/headdim128_sample.pt through the interpreter, at the bars of
    tests/test_sample_cpu_replay.py (2e-2 DDPM, 3e-2 Karras); every recording lies >= 10 bars from the head-dim-64 run of the same seeds;
  * the kernels on the functional emulation (the kernel tests of tests/test_headdim128_gpu.py in a child pytest);
  * no regression: the three snapshot tools report `unchanged`, and under the restated interpreter a head-dim-64 unet gives the bits of
    the stock interpreter.
    Measured here: planner hd128 cond / null 8.9e-4 / 7.3e-4, hd128_lin 1.0e-3 / 1.46e-3; DDPM replay 6.6e-4 / 5.6e-4 per stage, Karras
    replay 1.2e-2 / 1.8e-2; the emulated kernels give the MI355X figures of DESIGN.md section 4.3 to two digits (LINCTX: 0.8-1.4e-7)."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_headdim128 as hd  # noqa: E402
from fixtures_headdim128 import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401  (the fixture that sends Plan.run / Graph to the interpreter)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TINY = dict(dim=16, dim_mults=(1, 2), num_resnet_blocks=1, attn_heads=2, layer_attns=(False, True), layer_cross_attns=(False, True), cond_dim=32,
            text_embed_dim=32, attn_pool_num_latents=8, max_text_len=16)
FORWARD_BAR = 1e-2      # tests/test_linear_xattn_cpu.py::test_linear_unet_plan_on_cpu_matches_reference_fixture (lin32)
SAMPLE_BAR = {"ddpm": 2e-2, "edm": 3e-2}      # tests/test_sample_cpu_replay.py


@pytest.fixture()
def reference_weights():
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        yield ops
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


@pytest.fixture()
def hd_interpreter(monkeypatch):
    """plan_interp.Interpreter -> the restated class, for everything that instantiates it afterwards (cpu_backend among them)."""
    import plan_interp

    cls = hd.interpreter_class()
    monkeypatch.setattr(plan_interp, "Interpreter", cls)
    return cls


def run_unet(u, f, it=None):
    from imagen_pytorch_amd.engine import UnetEngine
    from plan_interp import run_engine

    B, S = f["x"].shape[0], f["x"].shape[-1]
    return run_engine(UnetEngine(u, 2 * B, B, S, "cpu", dry=True), f["x"], f["time"], f["text_embeds"], f["text_mask"], it=it)[:3]


# ------------------------------------------------------------------------------------------------ 1. surface

def test_unet_constructs_at_head_dim_128():
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.modules import CrossAttentionP

    u = Unet(**TINY, attn_dim_head=128)
    attn = u.downs[1][3].layers[0][0]
    C = attn.to_q.weight.shape[1]
    assert (attn.heads, attn.dim_head) == (2, 128) and tuple(attn.to_q.weight.shape) == (256, C) and tuple(attn.to_kv.weight.shape) == (256, C)
    assert tuple(attn.null_kv.shape) == (2, 128) and tuple(attn.q_scale.shape) == (128,)
    assert u.attn_pool.layers[0][0].dim_head == 128
    ca = u.downs[1][1].cross_attn
    assert isinstance(ca, CrossAttentionP) and (ca.heads, ca.dim_head) == (2, 128)
    # the mid ResnetBlocks are built without the attention kwargs, as in the reference: 8 x 64
    assert (u.mid_block1.cross_attn.heads, u.mid_block1.cross_attn.dim_head) == (8, 64)


@pytest.mark.parametrize("name", ["hd128", "hd128_lin", "sr"])
def test_reference_state_dict_loads_strictly(name):
    from imagen_pytorch_amd import Unet

    kw, sd = hd.unet_record(name)
    assert kw["attn_dim_head"] == 128
    u = Unet(**kw)
    assert list(u.state_dict()) == list(sd), "state_dict keys, in the reference's order"
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in u.state_dict().items())
    res = u.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_config_round_trip_and_imagen_from_config():
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.checkpoint import imagen_from_config

    u = Unet(**TINY, attn_dim_head=128)
    cfg, sd = u.to_config_and_state_dict()
    again = Unet.from_config_and_state_dict(cfg, sd)
    assert again.downs[1][3].layers[0][0].dim_head == 128
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), u.state_dict().values()))
    imagen = imagen_from_config("original", dict(unets=[dict(TINY, attn_dim_head=128)], image_sizes=(16,), timesteps=4, text_embed_dim=32))
    assert imagen.unets[0].downs[1][1].cross_attn.dim_head == 128
    elu = imagen_from_config("elucidated", dict(unets=[dict(TINY, attn_dim_head=128)], image_sizes=(16,), text_embed_dim=32, num_sample_steps=3))
    assert elu.unets[0].downs[1][1].cross_attn.dim_head == 128


def test_other_head_dims_still_raise():
    from imagen_pytorch_amd import Unet, Unet3D

    for bad in (48, 16, 256):
        with pytest.raises(NotImplementedError, match="attn_dim_head"):
            Unet(**TINY, attn_dim_head=bad)
    with pytest.raises(NotImplementedError, match="attn_dim_head"):
        Unet3D(dim=8, dim_mults=(1, 2), attn_dim_head=128)


def test_recordings_lie_apart_from_head_dim_64():
    g = hd.sample_fixture()
    for name in ("hd128", "hd128_lin"):
        f = hd.forward_record(name)
        for branch in ("out_cond", "out_null"):
            assert nerr(f[branch], f[branch + "_hd64"]) >= 10 * FORWARD_BAR
    for kind, bar in SAMPLE_BAR.items():
        run = g["runs"][kind]
        assert run["bar"] == bar
        assert min(nerr(a, b) for a, b in zip(run["outputs"], run["outputs_hd64"])) >= 10 * bar


# ------------------------------------------------------------------------------------------------ 2. planner

@pytest.mark.parametrize("name", ["hd128", "hd128_lin"])
def test_unet_plan_on_cpu_matches_reference_fixture(name, reference_weights, hd_interpreter):
    from imagen_pytorch_amd import _abi

    K = _abi.ENUMS
    f = hd.forward_record(name)
    oc, on, eng = run_unet(hd.unet(name), f)
    e_c, e_n = nerr(oc, f["out_cond"]), nerr(on, f["out_null"])
    print(f"planner + interpreter [{name}] vs the reference: cond {e_c:.3e} null {e_n:.3e}")
    assert e_c < FORWARD_BAR and e_n < FORWARD_BAR, (e_c, e_n)
    assert min(nerr(oc, f["out_cond_hd64"]), nerr(on, f["out_null_hd64"])) > 10 * FORWARD_BAR
    ops_ = eng.step_plan.ops
    # every 128-wide site goes launch by launch: ROWCHAIN's head-owning modes are built for 8 x 64, which only the mid blocks have
    dims = {p.head_dim for k, p, _ in ops_ if k == K["IMAGEN_OP_ATTENTION"]}
    assert dims == {128}, dims
    chains = [l for k, p, l in ops_ if k == K["IMAGEN_OP_ROWCHAIN"] and p.mode in (K["IMAGEN_CHAIN_XATTN"], K["IMAGEN_CHAIN_QKV"], K["IMAGEN_CHAIN_FF"])]
    assert chains == ["mid_block1.cross_attn.chain", "mid_block2.cross_attn.chain"], chains
    labels = [l for _, _, l in ops_]
    i = labels.index("downs.1.1.cross_attn.norm")
    assert labels[i:i + 5] == ["downs.1.1.cross_attn" + s for s in (".norm", ".to_q", ".attn", ".to_out", ".out_norm")]
    for s in eng.attn_sites:
        if s.kind == "linear":
            assert s.dh == 128 and tuple(s.M.shape) == (eng.R, 2, 128, 128)
        else:
            assert tuple(s.khat.shape) == (eng.R, s.heads, s.Jp, s.dh) and tuple(s.vt.shape) == (eng.R, s.heads, s.dh, s.Jp)
            assert s.k_strides[2] == s.dh and s.vt_strides[2] == s.Jp
    assert {s.dh for s in eng.attn_sites} == {128, 64}
    if name == "hd128_lin":
        assert sum(k == K["IMAGEN_OP_LINEAR_XATTN"] and p.head_dim == 128 for k, p, _ in ops_) == 2


def test_head_dim_64_plan_is_bit_identical_under_the_restated_interpreter(reference_weights):
    """The restated contracts say what the stock ones say where the stock ones apply."""
    import fixtures_linxattn as lx
    from plan_interp import Interpreter

    rec, _ = lx.unet_record("lin64")
    f = rec["forward"]
    a = run_unet(lx.unet("lin64"), f, it=Interpreter())
    b = run_unet(lx.unet("lin64"), f, it=hd.interpreter_class()())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert [(k, l) for k, _, l in a[2].step_plan.ops] == [(k, l) for k, _, l in b[2].step_plan.ops]


# ------------------------------------------------------------------------------------------------ 3. drivers

@pytest.mark.parametrize("kind", ["ddpm", "edm"])
def test_sample_driver_replay(hd_interpreter, cpu_backend, kind):
    """Imagen.sample / ElucidatedImagen.sample over the two head-dim-128 stages through the real driver (time table, graph objects) and
    eager, against the recorded runs of the live reference with the same draws."""
    g = hd.sample_fixture()
    run, bar = g["runs"][kind], SAMPLE_BAR[kind]
    model = hd.sample_model(kind)
    common = dict(text_embeds=g["text_embeds"], cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=lambda t, shape: run["noise"][t], device="cpu",
                  return_all_unet_outputs=True)
    outs = model.sample(**common)
    assert [tuple(o.shape) for o in outs] == [tuple(o.shape) for o in run["outputs"]]
    eager = model.sample(use_graph=False, **common)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    errs = [nerr(o, r) for o, r in zip(outs, run["outputs"])]
    far = [nerr(o, r) for o, r in zip(outs, run["outputs_hd64"])]
    print(f"head dim 128 {kind} replay per stage: {['%.2e' % e for e in errs]}; from the head-dim-64 run {['%.2e' % e for e in far]}")
    assert max(errs) < bar and min(far) > 10 * bar, (kind, errs, far)


# ------------------------------------------------------------------------------------------------ 4. the kernels, emulated

@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_kernels():
    """csrc/attention.hip, elementwise.hip and linear_xattn.hip compiled by tools/emul: the kernel and launcher tests of
    tests/test_headdim128_gpu.py in a child pytest on the emulated library."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_headdim128_gpu.py"), "-q", "-m", "gpu", "-k", "kernel or launcher",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
    assert int(out.split(" passed")[0].split()[-1]) == 12 + 2 + 6 + 6 + 1 + 9 + 2, out[-800:]


# ------------------------------------------------------------------------------------------------ 5. no regression

@pytest.mark.parametrize("tool", ["routing_snapshot.py", "attn_planner_snapshot.py", "sampler_snapshot.py"])
def test_snapshot_tools_report_unchanged(tool):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and "unchanged" in out.strip().splitlines()[-1], out[-2000:]
