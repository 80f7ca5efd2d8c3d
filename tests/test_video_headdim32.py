"""CPU: the Imagen-Video path at attention head dim 32 — the reference's Unet3DConfig default of 16 heads x 32 (configs.py:61-62), which
`ImagenConfig(video=True)` gives every unet of a config that leaves the head settings alone (ABI 12: ImagenTemporalAttentionParams.head_dim).

Constructor and config surface, the state_dict / oracle against the live reference (where its tree is present), the planner's launch lists on
the CPU plan interpreter (tests/plan_interp.py) against the oracle, and the two kernels of csrc/temporal.hip at D = 32 on the CPU emulation
of the kernel library (the kernel-level tests of tests/test_video_headdim32_gpu.py in a child pytest)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TINY_HD32 = dict(dim=16, dim_mults=(1, 2), attn_dim_head=32, attn_heads=4, text_embed_dim=32, cond_dim=32, max_text_len=16, attn_pool_num_latents=8,
                 layer_attns=(False, True), temporal_strides=(1, 2))


@pytest.fixture()
def reference_weights():
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        yield ops
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


def nerr(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def _derandomise_unet3d(unet, seed=1234):
    """As tests/test_video_gpu.py::_derandomise_unet3d (zero final_conv, dirac temporal convs, zero out-norm gain of the temporal attentions)."""
    g = torch.Generator().manual_seed(seed)
    for name, prm in unet.named_parameters():
        if name.startswith("final_conv."):
            prm.data.copy_(torch.randn(prm.shape, generator=g) * 0.05)
        elif ".temporal_conv." in name:
            prm.data.add_(torch.randn(prm.shape, generator=g) * (0.5 / (3 * prm.shape[1]) ** 0.5 if prm.ndim > 1 else 0.05))
        elif name.endswith("fn.fn.to_out.1.g"):
            prm.data.copy_(1.0 + 0.2 * torch.randn(prm.shape, generator=g))


def _temporal_attentions(unet):
    """The Attention3dP modules of the temporal attentions (init / per level / mid): the ones with a relative position bias."""
    return [m for m in unet.modules() if type(m).__name__ == "Attention3dP" and m.rel_pos_bias is not None]


# ------------------------------------------------------------------------------------------------ constructor / config surface
def test_unet3d_constructs_at_head_dim_32():
    from imagen_pytorch_amd import Unet3D

    u = Unet3D(dim=16, attn_dim_head=32, attn_heads=4, dim_mults=(1, 2), text_embed_dim=32)
    att = [m for m in u.modules() if type(m).__name__ == "Attention3dP"]
    assert att and all(m.dim_head == 32 and m.heads == 4 for m in att)
    ta = _temporal_attentions(u)
    assert len(ta) >= 4 and all(tuple(m.null_kv.shape) == (2, 32) and tuple(m.to_kv.weight.shape)[0] == 64 for m in ta)
    Unet3D(dim=16, attn_dim_head=64, attn_heads=2, dim_mults=(1, 2), text_embed_dim=32)       # 64 as before


def test_unet3d_refuses_other_head_dims():
    from imagen_pytorch_amd import Unet3D

    with pytest.raises(NotImplementedError, match="attn_dim_head"):
        Unet3D(dim=16, attn_dim_head=48, dim_mults=(1, 2), text_embed_dim=32)


def test_video_config_without_head_settings_builds_16_heads_of_32():
    """`ImagenConfig(video=True)` turns every unet of a config into a Unet3D (configs.py:87-99) and Unet3DConfig defaults to 16 heads x 32
    (configs.py:61-62): a video config (or checkpoint) that leaves the head settings alone has to build.  (NotImplementedError before ABI 12.)"""
    from imagen_pytorch_amd.checkpoint import imagen_from_config

    params = torch.load(os.path.join(GOLDEN, "checkpoint_tiny.pt"), map_location="cpu", weights_only=False)["checkpoint"]["imagen_params"]
    bare = {k: v for k, v in params["unets"][0].items() if k not in ("attn_dim_head", "attn_heads")}
    vid = imagen_from_config("original", {**params, "video": True, "unets": [bare]})
    assert vid.is_video and type(vid.unets[0]).__name__ == "Unet3D"
    ta = _temporal_attentions(vid.unets[0])
    assert ta and all(m.dim_head == 32 and m.heads == 16 for m in ta)
    every = [m for m in vid.unets[0].modules() if type(m).__name__ in ("Attention3dP", "PerceiverAttentionP")]
    assert every and all(m.dim_head == 32 and m.heads == 16 for m in every)


def test_video_checkpoint_without_head_settings_loads(tmp_path):
    """load_imagen_from_checkpoint on a trainer checkpoint of a video model whose config leaves the heads at their defaults."""
    from imagen_pytorch_amd import load_imagen_from_checkpoint, save_checkpoint
    from imagen_pytorch_amd.checkpoint import imagen_from_config

    params = torch.load(os.path.join(GOLDEN, "checkpoint_tiny.pt"), map_location="cpu", weights_only=False)["checkpoint"]["imagen_params"]
    bare = {k: v for k, v in params["unets"][0].items() if k not in ("attn_dim_head", "attn_heads")}
    src = imagen_from_config("original", {**params, "video": True, "unets": [bare]})
    path = tmp_path / "video.pt"
    save_checkpoint(src, path)
    ck = torch.load(str(path), map_location="cpu", weights_only=False)
    for u in ck["imagen_params"]["unets"]:                                  # the case of the issue: a config WITHOUT the head settings
        u.pop("attn_dim_head", None)
        u.pop("attn_heads", None)
    torch.save(ck, str(path))
    got = load_imagen_from_checkpoint(path)
    assert got.is_video and all(m.dim_head == 32 and m.heads == 16 for m in _temporal_attentions(got.unets[0]))
    a, b = src.unets[0].state_dict(), got.unets[0].state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ the reference's surface
def _reference():
    from oracle.ref_shim import load_reference, reference_available

    if not reference_available():
        pytest.skip("the reference's tree is not present")
    return load_reference("imagen_video")


def test_reference_state_dict_loads_strictly_at_head_dim_32():
    iv = _reference()
    from imagen_pytorch_amd import Unet3D

    torch.manual_seed(0)
    ref = iv.Unet3D(**TINY_HD32)
    ours = Unet3D(**TINY_HD32)
    sd = ref.state_dict()
    assert list(sd.keys()) == list(ours.state_dict().keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in ours.state_dict().values()]
    ours.load_state_dict(sd, strict=True)


def test_oracle_matches_live_reference_at_head_dim_32():
    """oracle/unet3d_oracle.py takes the head dim from the constructor kwargs: its forward against the live reference's Unet3D.forward at 4 heads
    x 32, cond and null rows, to the bound of tests/test_oracle_vs_reference.py::test_unet3d_forward_readme_config."""
    iv = _reference()
    from oracle import unet3d_oracle as u3

    torch.manual_seed(0)
    ref = iv.Unet3D(**TINY_HD32).eval()
    _derandomise_unet3d(ref)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    x, t, te = torch.randn(1, 3, 4, 16, 16), torch.tensor([0.3]), torch.randn(1, 9, 32)
    with torch.no_grad():
        for cdp in (0.0, 1.0):
            r = ref(x, t, text_embeds=te, cond_drop_prob=cdp)
            o = u3.unet3d_forward(sd, TINY_HD32, x, t, text_embeds=te, cond_drop_prob=cdp)
            assert r.abs().mean() > 0.05
            assert torch.allclose(r, o, atol=1e-4, rtol=1e-4), (r - o).abs().max()


# ------------------------------------------------------------------------------------------------ planner on the CPU interpreter
def test_unet3d_plan_at_head_dim_32_vs_oracle(reference_weights):
    """The dry-run launch lists of a small head-dim-32 Unet3D (temporal strides, a transformer block, cross-attention, Perceiver pooling: every
    attention site of the video planner), cond and null rows, replayed by the plan interpreter against the fp32 oracle — the bound of
    tests/test_plan_interp.py's video cases."""
    from imagen_pytorch_amd import Unet3D, _abi
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from oracle import unet3d_oracle as u3
    from plan_interp import run_engine

    torch.manual_seed(3)
    u = Unet3D(**TINY_HD32).eval()
    _derandomise_unet3d(u)
    B, Fr, S = 1, 8, 16
    x, t, te = torch.randn(B, 3, Fr, S, S), torch.tensor([0.3]), torch.randn(B, 9, 32)
    out_c, out_n, eng, _ = run_engine(UnetEngine3D(u, 2 * B, B, Fr, S, "cpu", dry=True), x, t, te)
    sd = u.state_dict()
    with torch.no_grad():
        ref_c = u3.unet3d_forward(sd, TINY_HD32, x, t, text_embeds=te)
        ref_n = u3.unet3d_forward(sd, TINY_HD32, x, t, text_embeds=te, cond_drop_prob=1.0)
    assert ref_c.abs().mean() > 0.05
    e_c, e_n = nerr(out_c, ref_c), nerr(out_n, ref_n)
    assert e_c < 5e-3 and e_n < 5e-3, (e_c, e_n)
    kind = _abi.ENUMS["IMAGEN_OP_TEMPORAL_ATTENTION"]
    ta = [p for k, p, _ in eng.step_plan.ops if k == kind]
    assert len(ta) >= 4 and all(p.head_dim == 32 and p.heads == 4 and p.ld == 6 * 32 for p in ta)
    hd = {getattr(p, "head_dim", None) for k, p, _ in eng.step_plan.ops if k in (_abi.ENUMS["IMAGEN_OP_ATTENTION"], _abi.ENUMS["IMAGEN_OP_KV_PREP"], _abi.ENUMS["IMAGEN_OP_QNORM"])}
    assert hd <= {32}, hd            # every other attention site threads the head dim through as well


def _interpreter_abi11():
    """The interpreter with TEMPORAL_ATTENTION as the header stated it before ABI 12: 64-wide heads, no head_dim field read."""
    import torch.nn.functional as F

    from plan_interp import Interpreter, K, f16, f32

    class InterpreterABI11(Interpreter):
        def temporal_attention(self, p):
            m = self.mem
            Fr, P, H = p.F, p.P, p.heads
            rows = m.strided(p.qkv, f16, (p.B, Fr, P, H * 64 + 128), (Fr * P * p.ld, P * p.ld, p.ld, 1)).float()
            q = rows[..., :H * 64].reshape(p.B, Fr, P, H, 64).permute(0, 2, 3, 1, 4)          # b p h i d
            k, v = rows[..., H * 64:H * 64 + 64].permute(0, 2, 1, 3), rows[..., H * 64 + 64:].permute(0, 2, 1, 3)   # b p j d
            nkv = m.view(p.null_kv, f32)[:128].reshape(2, 64)
            k = torch.cat((nkv[0].expand(p.B, P, 1, 64), k), dim=2)
            v = torch.cat((nkv[1].expand(p.B, P, 1, 64), v), dim=2)
            qh = F.normalize(q, dim=-1, eps=1e-12) * m.view(p.q_scale, f32)[:64] * p.scale
            kh = F.normalize(k, dim=-1, eps=1e-12) * m.view(p.k_scale, f32)[:64]
            sim = torch.einsum("bphid,bpjd->bphij", qh, kh) + m.view(p.bias, f32)[:H * Fr * (Fr + 1)].reshape(H, Fr, Fr + 1)
            if p.causal:
                sim = sim.masked_fill(torch.ones(Fr, Fr + 1, dtype=torch.bool).triu(2), -torch.finfo(sim.dtype).max)
            o = torch.einsum("bphij,bpjd->bphid", sim.softmax(-1), v)                       # b p h i d
            o = o.permute(0, 3, 1, 2, 4).reshape(p.B, Fr, P, H * 64)
            m.strided(p.o, f16, (p.B, Fr, P, H * 64), (Fr * P * p.ld_o, P * p.ld_o, p.ld_o, 1)).copy_(o.half())

    InterpreterABI11.DISPATCH = {**Interpreter.DISPATCH, K["IMAGEN_OP_TEMPORAL_ATTENTION"]: InterpreterABI11.temporal_attention}
    return InterpreterABI11


def test_head_dim_64_plan_is_bit_identical_under_the_restated_interpreter(reference_weights):
    """The head-dim-generic contract is a strict generalisation: an existing head-dim-64 video plan (the 'base' clip of
    tests/golden/unet3d_tiny.pt) gives the same bits through the 64-wide statement of before ABI 12 (kept above) and through
    tests/plan_interp.py, and its TEMPORAL_ATTENTION params carry head_dim = 0 as before ABI 12."""
    from imagen_pytorch_amd import Unet3D, _abi
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from plan_interp import Interpreter, run_engine

    g = torch.load(os.path.join(GOLDEN, "unet3d_tiny.pt"), weights_only=False)["runs"]["base"]
    B, _, Fr, S, _ = g["x"].shape
    outs = []
    for interp in (_interpreter_abi11(), Interpreter):
        u = Unet3D(**g["kwargs"]).eval()
        u.load_state_dict(g["state_dict"])
        c, n, eng, _ = run_engine(UnetEngine3D(u, 2 * B, B, Fr, S, "cpu", dry=True), g["x"], g["time"], g["text_embeds"], g["text_mask"], it=interp())
        outs.append((c, n))
        ta = [p for k, p, _ in eng.step_plan.ops if k == _abi.ENUMS["IMAGEN_OP_TEMPORAL_ATTENTION"]]
        assert ta and all(p.head_dim == 0 for p in ta)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert nerr(outs[1][0], g["out_cond"]) < 5e-3 and nerr(outs[1][1], g["out_null"]) < 5e-3


def test_temporal_attention_params_are_unchanged_without_the_keyword():
    """ops.temporal_attention without `head_dim`, and with head_dim = 64: the same params bytes, the new field 0."""
    import ctypes

    from imagen_pytorch_amd import ops

    def params(**kw):
        qkv, o = ops.new_act(1, 1, 24, 2 * 64 + 128, "cpu"), ops.new_act(1, 1, 24, 128, "cpu")
        keep = [torch.zeros(2, 64), torch.ones(64), torch.ones(64), torch.zeros(2, 3, 4)]
        p = ops.temporal_attention(ops.Plan(), qkv, *keep, o, B=2, F=3, P=4, heads=2, causal=True, scale=8.0, **kw)
        for f in ("qkv", "null_kv", "q_scale", "k_scale", "bias", "o"):
            setattr(p, f, 0)
        return p, bytes(ctypes.string_at(ctypes.addressof(p), ctypes.sizeof(p)))

    (a, ba), (b, bb) = params(), params(head_dim=64)
    assert a.head_dim == 0 and ba == bb
    with pytest.raises(AssertionError):
        params(head_dim=32)           # 64-wide buffers are not a head-dim-32 site


# ------------------------------------------------------------------------------------------------ the kernels on the CPU emulation
@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_temporal_attention_head_dim_32():
    """csrc/temporal.hip's MFMA and vector kernels at D = 32 (and the D = 64 regression) executed by tools/emul: the kernel-level tests of
    tests/test_video_headdim32_gpu.py in a child pytest, as tests/test_igemm_emulated.py runs the head-dim-64 ones."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    env = dict(os.environ, IMAGEN_LIB_PATH=os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so"), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_video_headdim32_gpu.py"), "-q", "-m", "gpu", "-k", "temporal_attention",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=2400)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
    assert int(out.split(" passed")[0].split()[-1]) >= 13, out[-800:]
