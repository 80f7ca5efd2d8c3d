"""MI355X tests of the Imagen-Video path at attention head dim 32 — the reference's Unet3DConfig default, 16 heads x 32 (ABI 12:
ImagenTemporalAttentionParams.head_dim; csrc/temporal.hip's two kernels as templates over the head dim).

The kernel-level tests (everything above the whole-denoiser test) also run on the CPU emulation of the kernel library in the CPU suite
(tests/test_video_headdim32.py::test_emulated_temporal_attention_head_dim_32), before anything goes to hardware."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import gpu_device

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.gpu]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DH = 32
KERNEL_TOL = 2e-3     # tests/test_video_gpu.py::test_temporal_attention_kernel_vs_oracle
C5_TOL = 1.0e-3       # north_star's bar (tests/test_video_gpu.py)


def nerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm())


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _oracle_case(Fr, causal, heads, P, dh, seed=4, R=2):
    """The q | k | v rows of one temporal attention site as the oracle projects them (fp32 torch, rounded to the kernel's fp16 storage), the
    oracle's bias table, and attention3d's arithmetic from its l2norm on, restated piece by piece on the ROUNDED projections — checked against
    oracle.unet3d_oracle.attention3d itself on the unrounded ones.  Returns (state dict, packed rows [R*Fr*P, (heads + 2) dh], bias, ref o)."""
    from oracle import unet3d_oracle as u3
    from oracle.unet_oracle import _SD, gain_layernorm

    g = torch.Generator().manual_seed(seed)
    C = heads * dh
    rn = lambda *s: torch.randn(*s, generator=g)
    sd = {"norm.g": 1 + 0.1 * rn(C), "to_q.weight": rn(C, C) / C ** 0.5, "to_kv.weight": rn(2 * dh, C) / C ** 0.5, "null_kv": rn(2, dh),
          "q_scale": torch.rand(dh, generator=g) + 0.5, "k_scale": torch.rand(dh, generator=g) + 0.5, "null_attn_bias": rn(heads),
          "to_out.0.weight": torch.eye(C), "to_out.1.g": 1 + 0.1 * rn(C),
          "rel_pos_bias.mlp.0.0.weight": rn(16, 1), "rel_pos_bias.mlp.0.0.bias": rn(16) * 0.1, "rel_pos_bias.mlp.0.1.g": torch.ones(16),
          "rel_pos_bias.mlp.1.weight": rn(heads, 16) * 0.3, "rel_pos_bias.mlp.1.bias": rn(heads) * 0.1}
    p = _SD(sd)
    seq = rn(R * P, Fr, C)                                                             # one sequence of F frames per (clip, pixel)
    xn = gain_layernorm(seq, sd["norm.g"])
    bias = torch.cat((sd["null_attn_bias"].reshape(heads, 1, 1).expand(heads, Fr, 1), u3.dynamic_position_bias(p.sub("rel_pos_bias"), Fr)), dim=-1)

    def attend(qp, kvp):
        q = qp.reshape(R * P, Fr, heads, dh).permute(0, 2, 1, 3)
        k = torch.cat((sd["null_kv"][0].expand(R * P, 1, dh), kvp[..., :dh]), dim=1)
        v = torch.cat((sd["null_kv"][1].expand(R * P, 1, dh), kvp[..., dh:]), dim=1)
        sim = torch.einsum("bhid,bjd->bhij", F.normalize(q, dim=-1, eps=1e-12) * sd["q_scale"], F.normalize(k, dim=-1, eps=1e-12) * sd["k_scale"]) * 8.0 + bias
        if causal:
            sim = sim.masked_fill(torch.ones(Fr, Fr + 1, dtype=torch.bool).triu(2), -torch.finfo(sim.dtype).max)
        return torch.einsum("bhij,bjd->bhid", sim.softmax(dim=-1), v).permute(0, 2, 1, 3).reshape(R * P, Fr, C)

    q16, kv16 = F.linear(xn, sd["to_q.weight"]).half(), F.linear(xn, sd["to_kv.weight"]).half()
    ref_o = attend(q16.float(), kv16.float())
    full = u3.attention3d(p, seq, None, causal)
    of = attend(F.linear(xn, sd["to_q.weight"]), F.linear(xn, sd["to_kv.weight"]))
    assert nerr(gain_layernorm(of, sd["to_out.1.g"]), full) < 1e-5, "the pieces above must BE the oracle's attention3d"
    packed = torch.cat((q16, kv16), dim=-1).reshape(R, P, Fr, C + 2 * dh).permute(0, 2, 1, 3).reshape(R * Fr * P, C + 2 * dh)
    return sd, packed, bias.contiguous(), ref_o


def _launch(dev, sd, packed, bias, *, R, Fr, P, heads, dh, causal, ld_o=None, head_dim="pass"):
    """Run the kernel on the packed rows; returns the whole o buffer [rows, ld_o] (NaN-free sentinel -7 in every column before the launch)."""
    from imagen_pytorch_amd import ops
    from imagen_pytorch_amd.ops import Act

    C = heads * dh
    rows = R * Fr * P
    ld_o = ld_o or C
    qkv = ops.new_act(1, 1, rows, C + 2 * dh, dev)
    qkv.t.copy_(packed.reshape(qkv.t.shape))
    ot = torch.full((rows, ld_o), -7.0, dtype=torch.float16, device=dev)
    o = Act(ot, 1, 1, rows, C, ld_o, rows * ld_o)
    plan = ops.Plan()
    kw = {} if head_dim == "default" else dict(head_dim=dh)
    p = ops.temporal_attention(plan, qkv, sd["null_kv"].contiguous().to(dev), sd["q_scale"].to(dev), sd["k_scale"].to(dev), bias.to(dev), o,
                               B=R, F=Fr, P=P, heads=heads, causal=causal, scale=8.0, **kw)
    plan.run()
    _sync(dev)
    return ot.float().cpu(), p


# (F, causal) of the head-dim-64 kernel test, P not a multiple of 4, 3 heads (a row count that is no multiple of 32) and 16 (the config default);
# F = 32 does not fit the MFMA kernel's 32-key tile: the vector kernel (its two pixels per wave with an odd pixel count: the last wave's
# second half has no pixel)
@pytest.mark.parametrize("heads", [3, 16])
@pytest.mark.parametrize("Fr,causal", [(4, True), (16, True), (7, False), (32, True)])
def test_temporal_attention_head_dim_32_vs_oracle(Fr, causal, heads):
    """TEMPORAL_ATTENTION at head_dim = 32 alone against the ORACLE's attention3d on identical fp16 inputs, with four sentinel columns behind
    every o row (ld_o = heads * 32 + 4, which keeps the MFMA kernel's 8-byte stores aligned): they must come back untouched."""
    dev = gpu_device()
    R, P = 2, 37
    C = heads * DH
    sd, packed, bias, ref_o = _oracle_case(Fr, causal, heads, P, DH)
    out, p = _launch(dev, sd, packed, bias, R=R, Fr=Fr, P=P, heads=heads, dh=DH, causal=causal, ld_o=C + 4)
    assert p.head_dim == 32
    got = out[:, :C].reshape(R, Fr, P, C).permute(0, 2, 1, 3).reshape(R * P, Fr, C)
    e = nerr(got, ref_o)
    print(f"temporal attention D=32 heads={heads} F={Fr} causal={causal}: {e:.2e}")
    assert e < KERNEL_TOL, e
    assert torch.equal(out[:, C:], torch.full_like(out[:, C:], -7.0)), "padding columns of o were written"


@pytest.mark.parametrize("Fr,causal", [(4, True), (7, False)])
def test_temporal_attention_head_dim_32_vector_kernel_on_unaligned_rows(Fr, causal):
    """An o row stride that is no multiple of 4 halfs keeps a shape off the MFMA kernel: the vector kernel at F <= 31 too (the route
    tools/temporal_attn_bench.py times), sentinels behind every row."""
    dev = gpu_device()
    R, P, heads = 2, 37, 3
    C = heads * DH
    sd, packed, bias, ref_o = _oracle_case(Fr, causal, heads, P, DH, seed=5)
    out, _ = _launch(dev, sd, packed, bias, R=R, Fr=Fr, P=P, heads=heads, dh=DH, causal=causal, ld_o=C + 2)
    got = out[:, :C].reshape(R, Fr, P, C).permute(0, 2, 1, 3).reshape(R * P, Fr, C)
    assert nerr(got, ref_o) < KERNEL_TOL, nerr(got, ref_o)
    assert torch.equal(out[:, C:], torch.full_like(out[:, C:], -7.0)), "padding columns of o were written"


def test_temporal_attention_head_dim_32_null_value_is_not_rounded():
    """tests/test_video_gpu.py::test_temporal_attention_null_value_is_not_rounded at head dim 32: the fp32 null value must not reach the output
    rounded to fp16 — the mean error of the first frame's output channels is the averaged-down rounding noise, not (nv - fp16(nv)) / 2.
    The reference is fp32 torch on the same fp16 rows (the contract of include/imagen_hip.h)."""
    from imagen_pytorch_amd import ops

    dev = gpu_device()
    R, Fr, P, heads = 2, 4, 256, 2
    C = heads * DH
    torch.manual_seed(0)
    rows = R * Fr * P
    qkv = ops.new_act(1, 1, rows, C + 2 * DH, dev)
    qkv.t.copy_(torch.randn(qkv.t.shape).half())
    o = ops.new_act(1, 1, rows, C, dev, zero=True)
    null_kv = torch.randn(2, DH) * 4.0 + 0.37          # (fp16 spacing of 2^-9 .. 2^-8 over most of the vector)
    plan = ops.Plan()
    ops.temporal_attention(plan, qkv, null_kv.to(dev), torch.ones(DH).to(dev), torch.ones(DH).to(dev), torch.zeros(heads, Fr, Fr + 1).to(dev), o,
                           B=R, F=Fr, P=P, heads=heads, causal=True, scale=1.0, head_dim=DH)
    plan.run()
    _sync(dev)
    x = qkv.t.float().cpu().reshape(R, Fr, P, C + 2 * DH)
    q = x[..., :C].reshape(R, Fr, P, heads, DH).permute(0, 2, 3, 1, 4)                  # b p h i d
    k = torch.cat((null_kv[0].expand(R, P, 1, DH), x[..., C:C + DH].permute(0, 2, 1, 3)), dim=2)
    v = torch.cat((null_kv[1].expand(R, P, 1, DH), x[..., C + DH:].permute(0, 2, 1, 3)), dim=2)
    sim = torch.einsum("bphid,bpjd->bphij", F.normalize(q, dim=-1, eps=1e-12), F.normalize(k, dim=-1, eps=1e-12))
    sim = sim.masked_fill(torch.ones(Fr, Fr + 1, dtype=torch.bool).triu(2), -torch.finfo(sim.dtype).max)
    ref = torch.einsum("bphij,bpjd->bphid", sim.softmax(-1), v).permute(0, 3, 1, 2, 4)  # b i p h d
    hip = o.t.float().cpu().reshape(R, Fr, P, heads, DH)
    assert nerr(hip, ref) < 1e-3
    d = (hip - ref)[:, 0].mean(dim=(0, 1, 2))                                          # first frame: keys = null + itself, weights ~ 1/2 each
    lost = null_kv[1] - null_kv[1].half().float()
    assert lost.norm() > 1e-3                                                          # the case does exercise the rounding
    assert float(d.norm() / lost.norm()) < 0.15, float(d.norm() / lost.norm())


def test_temporal_attention_default_head_dim_is_64_bit_for_bit():
    """The head-dim-64 regression: a call without `head_dim` (the params field 0, as every plan of before ABI 12 carries it) and a call with
    head_dim = 64 give the same bits, and both are the 64-wide attention of the oracle."""
    dev = gpu_device()
    R, P, heads, Fr, dh = 2, 37, 3, 16, 64
    sd, packed, bias, ref_o = _oracle_case(Fr, True, heads, P, dh)
    a, pa = _launch(dev, sd, packed, bias, R=R, Fr=Fr, P=P, heads=heads, dh=dh, causal=True, head_dim="default")
    b, pb = _launch(dev, sd, packed, bias, R=R, Fr=Fr, P=P, heads=heads, dh=dh, causal=True)
    assert pa.head_dim == 0 and pb.head_dim == 0          # one value for 64: the launch lists of head-dim-64 plans do not change
    assert torch.equal(a, b)
    C = heads * dh
    assert nerr(a.reshape(R, Fr, P, C).permute(0, 2, 1, 3).reshape(R * P, Fr, C), ref_o) < KERNEL_TOL


def test_temporal_attention_refuses_other_head_dims():
    from imagen_pytorch_amd import _abi, ops

    dev = gpu_device()
    qkv = ops.new_act(1, 1, 8, 3 * 48, dev)
    o = ops.new_act(1, 1, 8, 48, dev)
    with pytest.raises(AssertionError, match="head_dim"):
        ops.temporal_attention(ops.Plan(), qkv, torch.zeros(2, 48), torch.ones(48), torch.ones(48), torch.zeros(1, 2, 3), o, B=1, F=2, P=4, heads=1,
                               causal=True, scale=8.0, head_dim=48)
    qkv = ops.new_act(1, 1, 8, 3 * 32, dev)
    o = ops.new_act(1, 1, 8, 32, dev)
    plan = ops.Plan()
    z = lambda *s: torch.zeros(*s, device=dev)
    p = ops.temporal_attention(plan, qkv, z(2, 32), z(32) + 1, z(32) + 1, z(1, 2, 3), o, B=1, F=2, P=4, heads=1, causal=True, scale=8.0, head_dim=32)
    p.head_dim = 48                                        # the launcher's own check
    with pytest.raises(_abi.ImagenHipError, match="head_dim"):
        plan.run()


def _derandomise_unet3d(unet, seed=1234):
    """As tests/test_video_gpu.py::_derandomise_unet3d: Unet3D starts as an image Unet applied per frame (zero final_conv, dirac temporal convs,
    zero out-norm gain of the temporal attentions) — randomise the three so the temporal paths count."""
    g = torch.Generator().manual_seed(seed)
    for name, prm in unet.named_parameters():
        if name.startswith("final_conv."):
            prm.data.copy_(torch.randn(prm.shape, generator=g) * 0.05)
        elif ".temporal_conv." in name:
            prm.data.add_(torch.randn(prm.shape, generator=g) * (0.5 / (3 * prm.shape[1]) ** 0.5 if prm.ndim > 1 else 0.05))
        elif name.endswith("fn.fn.to_out.1.g"):
            prm.data.copy_(1.0 + 0.2 * torch.randn(prm.shape, generator=g))


C5_HD32 = dict(dim=64, dim_mults=(1, 2, 4, 8), attn_dim_head=32, attn_heads=16)


def c5_hd32_case(seed=0):
    """BASELINE config C5's denoiser with the config-default heads (16 x 32) on one 16 x 64 x 64 clip: (module, kwargs, x, t, text, mask).
    Shared with the CPU pricing of this test on the plan interpreter (tests/test_video_headdim32.py)."""
    from imagen_pytorch_amd import Unet3D

    torch.manual_seed(seed)
    u = Unet3D(**C5_HD32).eval()
    _derandomise_unet3d(u, seed=1234 + seed)
    x, t = torch.randn(1, 3, 16, 64, 64), torch.tensor([0.3])
    te = torch.randn(1, 24, 768)
    mask = torch.ones(1, 24, dtype=torch.bool)
    mask[0, 19:] = False
    return u, C5_HD32, x, t, te, mask


def test_unet3d_forward_vs_oracle_c5_head_dim_32():
    """The C5 shape with the config-default heads — Unet3D(dim=64, dim_mults=(1, 2, 4, 8), attn_dim_head=32, attn_heads=16), one 16 x 64 x 64
    clip, seed 0, cond and null rows — against the fp32 CPU oracle at the project's 1.0e-3 bar.  Priced on the CPU plan interpreter first
    (tests/plan_interp.py, which predicts hardware to 1-2 % on cond rows): cond 9.28e-4, null 9.07e-4."""
    from oracle import unet3d_oracle as u3

    dev = gpu_device()
    u, kw, x, t, te, mask = c5_hd32_case(0)
    sd = {k: v.clone() for k, v in u.state_dict().items()}
    with torch.no_grad():
        ref = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, text_mask=mask)
        ref_null = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, text_mask=mask, cond_drop_prob=1.0)
    u = u.to(dev)
    args = dict(text_embeds=te.to(dev), text_mask=mask.to(dev))
    e = nerr(u(x.to(dev), t.to(dev), **args), ref)
    e_null = nerr(u(x.to(dev), t.to(dev), cond_drop_prob=1.0, **args), ref_null)
    print(f"c5 Unet3D(dim=64, 16 heads x 32) 16x64x64 vs oracle: cond {e:.3e} null {e_null:.3e}")
    from conftest import record_parity
    record_parity("unet3d_forward_vs_oracle_c5_head_dim_32", cond=e, null=e_null, tol=C5_TOL)
    attn = [m for m in u.modules() if type(m).__name__ == "Attention3dP"]
    assert attn and all(m.dim_head == 32 and m.heads == 16 for m in attn)
    assert e < C5_TOL and e_null < C5_TOL, (e, e_null)


def _unpack_state_dict(spec):
    """A stage's weights as the fixture holds them — one flat fp16 tensor + the ordered (key, shape) index — as {key: fp32 tensor}."""
    sd, at = {}, 0
    for key, shape in spec["index"]:
        n = int(torch.Size(shape).numel())
        sd[key] = spec["flat"][at:at + n].float().reshape(shape)
        at += n
    assert at == spec["flat"].numel()
    return sd


def test_video_cascade_sample_head_dim_32_vs_reference_fixture():
    """Imagen.sample(video_frames=4) over two Unet3D stages with 2 heads x 32 vs the recorded run of the live reference (same draws:
    tools/make_video_headdim32_fixture.py); graph == eager.  Tolerance of test_video_cascade_sample_vs_reference_fixture."""
    from imagen_pytorch_amd import Imagen, Unet3D

    dev = gpu_device()
    g = torch.load(os.path.join(GOLDEN, "sample_tiny_video_hd32.pt"), weights_only=False)
    unets = [Unet3D(**spec["kwargs"]).eval() for spec in g["unets"]]
    assert all(spec["kwargs"]["attn_dim_head"] == 32 for spec in g["unets"])
    imagen = Imagen(unets, image_sizes=g["image_sizes"], timesteps=g["timesteps"], text_embed_dim=32, cond_drop_prob=0.1).to(dev)
    for u, spec in zip(imagen.unets, g["unets"]):
        u.load_state_dict(_unpack_state_dict(spec))
    noise_fn = lambda tag, shape: g["noise"][tag].to(dev)
    res = {}
    for use_graph in (False, True):
        outs = imagen.sample(text_embeds=g["text_embeds"].to(dev), video_frames=g["frames"], cond_scale=g["cond_scale"], use_tqdm=False,
                             return_all_unet_outputs=True, noise_fn=noise_fn, use_graph=use_graph)
        errs = [nerr(o, r) for o, r in zip(outs, g["outputs"])]
        print("video cascade (head dim 32)", "graph" if use_graph else "eager", errs)
        assert all(o.shape == r.shape for o, r in zip(outs, g["outputs"])) and max(errs) < 2e-2
        res[use_graph] = outs
    assert all(torch.equal(a, b) for a, b in zip(res[False], res[True]))
