"""MI355X: attention head dim 128 (Unet(attn_dim_head=128)): the kernels behind the unchanged launchers, then the whole unet and the samplers.

Kernels, each against fp64 on identical fp16-rounded inputs, strided operands, a sentinel band around and between the rows of every output:
  * ATTENTION (attention_kernel<128>, fused QNORM as the planner launches it): queries N in {1, 17, 64, 257}, keys J in {1, 33, 255}, 2 heads,
    2 rows; N = 257 shows that the rows >= 256 routing (head dim 64 only) falls through to this kernel.  ImagenAttentionParams carries no
    key mask — masked text tokens are replaced by the null embedding before the projection — so a mask that leaves the null key alone is
    J = 1, and the tile-boundary cases are J = 32 and J = 224 (the last 32-key tile exactly full; a whole tile fewer than 255 rounds up to);
  * QNORM, KV_PREP, KV_PREP_MULTI: rows in {1, 5, 67}, heads in {1, 3}, ld wider than heads * 128, a zero row (the l2norm's epsilon); the
    KV_PREP_MULTI launch mixes a head-dim-128 and a head-dim-64 job, as the planner's does (the mid blocks stay 8 x 64);
  * LINCTX -> LINEAR_XATTN: J in {1, 7, 40} tokens, {1, 64, 300} pixels, 2 heads;
  * refusals: every launcher still refuses head dim 48 with its message; ATTENTION at 128 refuses rows narrower than heads * 128.
Bar of a kernel: in the same run the head-dim-64 kernel of the family is measured against fp64 on the same draws (their first 64 dims);
head dim 128 is allowed 2 x that figure (its l2norm and its PV / k^T v sums are twice as long), never more than the project's per-op 1e-3
(`bar_from`, which also says what stands in for a figure of zero).

Whole unet and samplers: Unet.forward of `hd128` and `hd128_lin` against the recorded reference (tests/golden/headdim128_forward.pt), cond and
null — bar as for the head-dim-32 fixture unet of tests/test_linear_xattn_gpu.py: 1.5 x what the accepted flag-off head-dim-64 twin of
that file measures in the same run; Imagen.sample / ElucidatedImagen.sample over two stages against tests/golden/headdim128_sample.pt at
2e-2 / 3e-2, graph replay == eager bit for bit.

Every test prints its figures before it asserts and keeps them with record_parity.  Measured on MI355X (profiles/headdim128_parity_mi355x.json),
head dim 128 beside head dim 64: ATTENTION 1.97-2.22e-4 / 2.04-2.73e-4, QNORM 2.02-2.20e-4 / 1.91-2.26e-4, KV_PREP 2.04-2.28e-4 / 2.01-2.23e-4,
LINEAR_XATTN 1.99-2.08e-4 / 1.93-2.09e-4, LINCTX 0.78-1.42e-7 / 0.79-1.37e-7; unets 7.4e-4 .. 1.45e-3 under a bar of 2.26e-3; DDPM 7.7e-4 / 5.3e-4,
Karras 9.9e-3 / 1.57e-2."""
import os
import sys

import pytest
import torch

from conftest import gpu_device, record_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_headdim128 as hd  # noqa: E402
from fixtures_headdim128 import attention_contract, l2norm_scale_contract, nerr  # noqa: E402
from plan_interp import linctx_contract, linear_xattn_contract  # noqa: E402

pytestmark = pytest.mark.gpu

OP_CAP = 1e-3         # the project's per-op bar (README: "every HIP op <= 1e-3")
GUARD = 4096          # sentinel halves in front of and behind an output
SENTINEL = -1234.0
Q_MULT = 8.0 * 1.4426950408889634      # engine.SIM_SCALE * LOG2E


def nerr64(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d = ref.norm()
    return ((got - ref).norm() / d).item() if d > 0 else (got - ref).norm().item()


HALF_ULP = {torch.float16: 2.0 ** -12, torch.float32: 2.0 ** -25}


def bar_from(e64, out=torch.float16):
    """2 x the head-dim-64 figure of the same run, capped at the per-op bar.  A case with ONE key or token is exact by construction (o = v,
    M = v, 8 v) and its head-dim-64 figure is zero or the fp64 reference's own noise, which says nothing about a kernel: where that figure is
    below a quarter of the half-ulp of the output's format, the half-ulp stands in for it (one element rounded the other way is already more)."""
    floor = HALF_ULP[out]
    return min(OP_CAP, 2.0 * (e64 if e64 >= floor / 4 else floor))


def _run(plan):
    plan.run()
    if gpu_device().type == "cuda":
        torch.cuda.synchronize()


def guarded(shape, dev, dtype=torch.float16):
    """A sentinel-filled flat buffer with GUARD elements on both sides of a `shape` view; (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 1. ATTENTION

def _attention_case(N, J, D, seed):
    """(error vs fp64 whole, worst (row, head) slice) of one launch: B = 2 rows, H = 2 heads side by side in token rows of q (ld = H D + 2 D, as
    a q | k | v row) and o (ld = H D + 16), K^ rows D + 8 apart, V^T rows Jp + 8 apart.  The draws are made at 128 dims; D = 64 takes the first 64."""
    from imagen_pytorch_amd import ops

    dev = gpu_device()
    B, H, Jp = 2, 2, (J + 31) // 32 * 32
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, N, H, 128, generator=g) * 1.5)[..., :D].half()
    k = torch.randn(B, H, J, 128, generator=g)[..., :D]
    v = torch.randn(B, H, J, 128, generator=g)[..., :D].half()
    q_scale = (1.0 + 0.2 * torch.randn(128, generator=g))[:D].contiguous()
    k_scale = (1.0 + 0.2 * torch.randn(128, generator=g))[:D]
    khat = (torch.nn.functional.normalize(k, dim=-1) * k_scale).half()
    ldq, ldo, krs, vds = H * D + 2 * D, H * D + 16, D + 8, Jp + 8
    qb = torch.full((B, N, ldq), 7.0, dtype=torch.float16)
    qb[..., :H * D] = q.reshape(B, N, H * D)
    kb = torch.full((B, H, Jp, krs), SENTINEL, dtype=torch.float16)
    kb[..., :D] = 0
    kb[:, :, :J, :D] = khat
    vb = torch.full((B, H, D, vds), SENTINEL, dtype=torch.float16)
    vb[..., :Jp] = 0
    vb[..., :J] = v.transpose(-1, -2)
    qd, kd, vd, qs = qb.to(dev), kb.to(dev), vb.to(dev), q_scale.to(dev)
    obuf, o = guarded((B, N, ldo), dev)
    plan = ops.Plan("attention")
    ops.attention(plan, qd, kd, vd, o, B=B, heads=H, rows=N, J=J, q_strides=(N * ldq, D, ldq), k_strides=(H * Jp * krs, Jp * krs, krs),
                  vt_strides=(H * D * vds, D * vds, vds), o_strides=(N * ldo, D, ldo), q_scale=qs, q_mult=Q_MULT, head_dim=D)
    _run(plan)
    oc = o.cpu()
    assert guards_intact(obuf) and bool((oc[..., H * D:] == SENTINEL).all()), "attention wrote outside its o rows"
    got = oc[..., :H * D].reshape(B, N, H, D).permute(0, 2, 1, 3)
    assert torch.isfinite(got).all()
    ref = attention_contract(q.permute(0, 2, 1, 3), khat, v, q_scale, Q_MULT)
    return nerr64(got, ref), max(nerr64(got[b, h], ref[b, h]) for b in range(B) for h in range(H))


def _attention_check(N, J):
    e64, s64 = _attention_case(N, J, 64, seed=1000 * N + J)
    e, s = _attention_case(N, J, 128, seed=1000 * N + J)
    print(f"ATTENTION N {N} J {J}: head dim 128 {e:.2e} (worst slice {s:.2e}); head dim 64 on the same draws {e64:.2e} ({s64:.2e}); "
          f"bars {bar_from(e64):.2e} / {bar_from(s64):.2e}")
    record_parity(f"headdim128_attention[N={N},J={J}]", err=e, worst_slice=s, err_hd64=e64, worst_slice_hd64=s64)
    assert e <= bar_from(e64) and s <= bar_from(s64), (e, e64, s, s64)


@pytest.mark.parametrize("J", [1, 33, 255])
@pytest.mark.parametrize("N", [1, 17, 64, 257])
def test_attention_kernel_vs_fp64(N, J):
    _attention_check(N, J)


@pytest.mark.parametrize("J", [32, 224])
def test_attention_kernel_tile_boundaries(J):
    _attention_check(17, J)


# ------------------------------------------------------------------------------------------------ 2. QNORM / KV_PREP

def _qnorm_case(rows, heads, D, seed):
    from imagen_pytorch_amd import ops

    dev = gpu_device()
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, heads, 128, generator=g) * 2.0)[..., :D].half()
    x[rows // 2, 0] = 0                      # a zero row: 0 / max(0, 1e-12) = 0
    scale = (1.0 + 0.2 * torch.randn(128, generator=g))[:D].contiguous()
    ld = heads * D + 24
    qbuf, qv = guarded((rows, ld), dev)
    qv[:, :heads * D] = x.reshape(rows, heads * D).to(dev)
    plan = ops.Plan("qnorm")
    ops.qnorm(plan, qv, scale.to(dev), rows=rows, heads=heads, ld=ld, mult=Q_MULT, head_dim=D)
    _run(plan)
    out = qv.cpu()
    assert guards_intact(qbuf) and bool((out[:, heads * D:] == SENTINEL).all()), "qnorm wrote outside its head rows"
    got = out[:, :heads * D].reshape(rows, heads, D)
    assert bool((got[rows // 2, 0] == 0).all())
    return nerr64(got, l2norm_scale_contract(x, scale, Q_MULT))


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("rows", [1, 5, 67])
def test_qnorm_kernel_vs_fp64(rows, heads):
    e64 = _qnorm_case(rows, heads, 64, seed=10 * rows + heads)
    e = _qnorm_case(rows, heads, 128, seed=10 * rows + heads)
    print(f"QNORM rows {rows} heads {heads}: head dim 128 {e:.2e}; head dim 64 {e64:.2e}; bar {bar_from(e64):.2e}")
    record_parity(f"headdim128_qnorm[rows={rows},heads={heads}]", err=e, err_hd64=e64)
    assert e <= bar_from(e64), (e, e64)


def _kv_job(ops, plan, rows, heads, D, seed, batch=None):
    """One KV_PREP job: B = 2, source rows (k heads | v heads | 8 spare), key rows [2, 2 + rows) of K^ (row stride D + 8) / V^T (row stride Jp + 8).
    Returns a closure that checks the outputs and gives the error of K^."""
    dev = gpu_device()
    B, r0 = 2, 2
    Jp = (r0 + rows + 31) // 32 * 32
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn(B, rows, heads, 128, generator=g) * 2.0)[..., :D].half()
    v = torch.randn(B, rows, heads, 128, generator=g)[..., :D].half()
    k[0, rows // 2, 0] = 0
    scale = (1.0 + 0.2 * torch.randn(128, generator=g))[:D].contiguous()
    inner, krs, vds = heads * D, D + 8, Jp + 8
    ld = 2 * inner + 8
    src = torch.full((B, rows, ld), 3.0, dtype=torch.float16)
    src[..., :inner], src[..., inner:2 * inner] = k.reshape(B, rows, inner), v.reshape(B, rows, inner)
    srcd, sc = src.to(dev), scale.to(dev)
    kbuf, kh = guarded((B, heads, Jp, krs), dev)
    vbuf, vt = guarded((B, heads, D, vds), dev)
    ops.kv_prep(plan, srcd, srcd, sc, kh, vt, B=B, heads=heads, rows=rows, r0=r0, src_strides=(rows * ld, ld, D), k_strides=(heads * Jp * krs, Jp * krs, krs),
                vt_strides=(heads * D * vds, D * vds, vds), k_off=0, v_off=inner, head_dim=D, batch=batch)

    def check():
        assert guards_intact(kbuf) and guards_intact(vbuf), "kv_prep wrote outside K^ / V^T"
        kc, vc = kh.cpu().clone(), vt.cpu().clone()
        got_k = kc[:, :, r0:r0 + rows, :D].clone()
        kc[:, :, r0:r0 + rows, :D] = SENTINEL
        got_v = vc[:, :, :, r0:r0 + rows].clone()
        vc[:, :, :, r0:r0 + rows] = SENTINEL
        assert bool((kc == SENTINEL).all()) and bool((vc == SENTINEL).all()), "kv_prep wrote outside its key rows"
        assert torch.equal(got_v, v.permute(0, 2, 3, 1)), "V^T is a transposed copy"
        assert bool((got_k[0, 0, rows // 2] == 0).all())
        return nerr64(got_k, l2norm_scale_contract(k.permute(0, 2, 1, 3), scale))
    return check


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("rows", [1, 5, 67])
def test_kv_prep_kernel_vs_fp64(rows, heads):
    from imagen_pytorch_amd import ops

    errs = {}
    for D in (64, 128):
        plan = ops.Plan("kv_prep")
        check = _kv_job(ops, plan, rows, heads, D, seed=20 * rows + heads)
        _run(plan)
        errs[D] = check()
    print(f"KV_PREP rows {rows} heads {heads}: head dim 128 {errs[128]:.2e}; head dim 64 {errs[64]:.2e}; bar {bar_from(errs[64]):.2e}")
    record_parity(f"headdim128_kv_prep[rows={rows},heads={heads}]", err=errs[128], err_hd64=errs[64])
    assert errs[128] <= bar_from(errs[64]), errs


def test_kv_prep_multi_kernel_mixes_head_dims():
    """ONE launch, as the planner's: a 128-wide job of 67 rows x 3 heads (the grid's extent), a 64-wide job of 5 rows x 1 head, a 128-wide job of 1 row."""
    from imagen_pytorch_amd import _abi, ops

    plan, jobs = ops.Plan("kv_prep_multi"), []
    checks = [(D, _kv_job(ops, plan, rows, heads, D, seed=31 + rows, batch=jobs)) for rows, heads, D in ((67, 3, 128), (5, 1, 64), (1, 3, 128))]
    ops.kv_prep_multi(plan, jobs, gpu_device())
    assert [k for k, _, _ in plan.ops] == [_abi.ENUMS["IMAGEN_OP_KV_PREP_MULTI"]]
    _run(plan)
    errs = [(D, c()) for D, c in checks]
    e64 = max(e for D, e in errs if D == 64)
    e128 = max(e for D, e in errs if D == 128)
    print(f"KV_PREP_MULTI mixed launch: head dim 128 jobs {e128:.2e}; the head dim 64 job {e64:.2e}; bar {bar_from(e64):.2e}")
    record_parity("headdim128_kv_prep_multi", err=e128, err_hd64=e64)
    assert e128 <= bar_from(e64), errs


# ------------------------------------------------------------------------------------------------ 3. LINCTX -> LINEAR_XATTN

def _linear_case(J, N, D, seed):
    """LINCTX of R = 2 images x 2 heads, then LINEAR_XATTN of N pixels per image on the M it wrote: (error of M, error of o given that M)."""
    from imagen_pytorch_amd import ops
    from imagen_pytorch_amd.ops import Act

    dev = gpu_device()
    R, H = 2, 2
    inner = H * D
    g = torch.Generator().manual_seed(seed)
    kv = (torch.randn(R, J, 2, H, 128, generator=g) * 2.0)[..., :D].reshape(R, J, 2 * inner).half()
    q = (torch.randn(R, N, H, 128, generator=g) * 1.5)[..., :D].reshape(R, N, inner).half()
    kvd = kv.to(dev)
    Mbuf, M = guarded((R, H, D, D), dev, torch.float32)
    plan, jobs = ops.Plan("linear"), []
    ops.linctx_job(kvd, M, R=R, heads=H, head_dim=D, J=J, kv_bs=J * 2 * inner, kv_rs=2 * inner, batch=jobs)
    ops.linctx(plan, jobs, dev)
    ldq, ldo = inner + 8, inner + 16
    qd = torch.full((R, N, ldq), 5.0, dtype=torch.float16, device=dev)
    qd[..., :inner] = q.to(dev)
    obuf, o = guarded((R, N, ldo), dev)
    ops.linear_xattn(plan, Act(qd, R, 1, N, inner, ldq, N * ldq), M, Act(obuf, R, 1, N, inner, ldo, N * ldo, off=GUARD), heads=H, head_dim=D, rows_per_batch=N)
    _run(plan)
    assert guards_intact(Mbuf) and guards_intact(obuf), "linctx / linear_xattn wrote outside M / o"
    oc, Mc = o.cpu(), M.cpu()
    assert bool((oc[..., inner:] == SENTINEL).all()), "linear_xattn wrote outside its o rows"
    assert torch.isfinite(oc[..., :inner]).all() and torch.isfinite(Mc).all()
    eM = nerr64(Mc, linctx_contract(kv, H, D, dtype=torch.float64))
    eo = nerr64(oc[..., :inner], linear_xattn_contract(q, Mc, H, D, dtype=torch.float64))
    return eM, eo


@pytest.mark.parametrize("N", [1, 64, 300])
@pytest.mark.parametrize("J", [1, 7, 40])
def test_linctx_linear_xattn_kernel_vs_fp64(J, N):
    m64, o64 = _linear_case(J, N, 64, seed=50 * J + N)
    m, o = _linear_case(J, N, 128, seed=50 * J + N)
    print(f"LINCTX J {J}: head dim 128 {m:.2e}, head dim 64 {m64:.2e}, bar {bar_from(m64, torch.float32):.2e};  LINEAR_XATTN N {N}: {o:.2e}, head dim 64 {o64:.2e}, "
          f"bar {bar_from(o64):.2e}")
    record_parity(f"headdim128_linear[J={J},N={N}]", linctx=m, linctx_hd64=m64, linear_xattn=o, linear_xattn_hd64=o64)
    assert m <= bar_from(m64, torch.float32) and o <= bar_from(o64), (m, m64, o, o64)


# ------------------------------------------------------------------------------------------------ 4. refusals

def _refused(ops, struct, fields, keep, match):
    from imagen_pytorch_amd._abi import STRUCTS, ImagenHipError

    p = STRUCTS[struct]()
    for k, v in fields.items():
        setattr(p, k, v)
    plan = ops.Plan("refused")
    plan.add(p, "refused", keep)
    with pytest.raises(ImagenHipError, match=match):
        plan.run()


def test_launchers_still_refuse_head_dim_48():
    from imagen_pytorch_amd import ops
    from imagen_pytorch_amd._abi import ImagenHipError

    dev = gpu_device()
    a = torch.zeros(4096, dtype=torch.float16, device=dev)
    f = torch.zeros(4096, device=dev)
    P = a.data_ptr()
    _refused(ops, "ImagenAttentionParams", dict(q=P, k=P, vt=P, o=P, B=1, heads=1, rows=4, J=4, q_bs=256, q_hs=48, q_rs=48, k_bs=2048, k_hs=2048, k_rs=48,
                                                vt_bs=2048, vt_hs=2048, vt_ds=32, o_bs=256, o_hs=48, o_rs=48, head_dim=48), [a], "attention: head_dim 48")
    _refused(ops, "ImagenQnormParams", dict(q=P, q_scale=f.data_ptr(), rows=4, heads=1, ld=48, mult=1.0, head_dim=48), [a, f], "qnorm: head_dim 48")
    _refused(ops, "ImagenKvPrepParams", dict(k_src=P, v_src=P, k_scale=f.data_ptr(), khat=P, vt=P, B=1, heads=1, rows=4, r0=0, src_bs=512, src_rs=96, src_hs=48,
                                             k_bs=2048, k_hs=2048, k_rs=48, vt_bs=2048, vt_hs=2048, vt_ds=32, head_dim=48), [a, f], "kv_prep: head_dim 48")
    _refused(ops, "ImagenLinearXattnParams", dict(q=P, M=f.data_ptr(), o=P, R=1, heads=1, rows=4, ld_q=48, ld_o=48, head_dim=48), [a, f], "linear_xattn: head_dim 48")
    with pytest.raises(ImagenHipError, match="head_dim 48"):
        ops.linctx_job(a, f[:48 * 48], R=1, heads=1, head_dim=48, J=4, kv_bs=4 * 96, kv_rs=96, batch=[])


def test_attention_launcher_refuses_rows_narrower_than_the_heads():
    from imagen_pytorch_amd import ops

    dev = gpu_device()
    a = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    P = a.data_ptr()
    base = dict(q=P, k=P, vt=P, o=P, B=1, heads=2, rows=4, J=4, q_bs=4096, q_hs=128, q_rs=256, k_bs=8192, k_hs=4096, k_rs=128, vt_bs=8192, vt_hs=4096,
                vt_ds=32, o_bs=4096, o_hs=128, o_rs=256, head_dim=128)
    _refused(ops, "ImagenAttentionParams", dict(base, q_rs=128), [a], "row strides")
    _refused(ops, "ImagenAttentionParams", dict(base, o_rs=128), [a], "row strides")
    plan = ops.Plan("taken")      # the valid form passes the checks
    from imagen_pytorch_amd._abi import STRUCTS
    p = STRUCTS["ImagenAttentionParams"]()
    for k, v in base.items():
        setattr(p, k, v)
    plan.add(p, "taken", [a])
    _run(plan)


# ------------------------------------------------------------------------------------------------ 5. whole Unet.forward

@pytest.fixture(scope="module")
def twin_figures():
    """(cond, null) of the accepted flag-off head-dim-64 twin of tests/test_linear_xattn_gpu.py against its recording, in this run."""
    import fixtures_linxattn as lx

    dev = gpu_device()
    f = lx.unet_record("twin")[0]["forward"]
    u = lx.unet("twin", dev)
    kw = dict(text_embeds=f["text_embeds"].to(dev), text_mask=f["text_mask"].to(dev))
    x, t = f["x"].to(dev), f["time"].to(dev)
    return nerr(u(x, t, **kw).cpu(), f["out_cond"]), nerr(u(x, t, cond_drop_prob=1.0, **kw).cpu(), f["out_null"])


@pytest.mark.parametrize("name", ["hd128", "hd128_lin"])
def test_unet_forward_vs_reference_fixture(twin_figures, name):
    dev = gpu_device()
    f = hd.forward_record(name)
    u = hd.unet(name, dev)
    kw = dict(text_embeds=f["text_embeds"].to(dev), text_mask=f["text_mask"].to(dev))
    x, t = f["x"].to(dev), f["time"].to(dev)
    oc, on = u(x, t, **kw).cpu(), u(x, t, cond_drop_prob=1.0, **kw).cpu()
    e_c, e_n = nerr(oc, f["out_cond"]), nerr(on, f["out_null"])
    bar = 1.5 * max(twin_figures)
    far = min(nerr(oc, f["out_cond_hd64"]), nerr(on, f["out_null_hd64"]))
    print(f"Unet(attn_dim_head=128) [{name}]: cond {e_c:.3e} null {e_n:.3e}; the head-dim-64 twin {twin_figures[0]:.3e} / {twin_figures[1]:.3e}, "
          f"bar {bar:.3e}; from the head-dim-64 recording {far:.3e}")
    record_parity(f"headdim128_unet[{name}]", cond=e_c, null=e_n, tol=bar, twin_cond=twin_figures[0], twin_null=twin_figures[1])
    assert max(e_c, e_n) <= bar, (name, e_c, e_n, bar)
    assert far >= 10 * bar, (far, bar)
    cfg = u.forward_with_cond_scale(x, t, cond_scale=3.0, **kw).cpu()
    want = f["out_null"] + (f["out_cond"] - f["out_null"]) * 3.0
    print(f"forward_with_cond_scale(3) [{name}]: {nerr(cfg, want):.3e}")
    assert nerr(cfg, want) <= 3 * bar       # (cond - null) * 3 carries up to three times the branches' error


# ------------------------------------------------------------------------------------------------ 6. samplers

@pytest.mark.parametrize("kind,bar", [("ddpm", 2e-2), ("edm", 3e-2)])
def test_sample_vs_reference_fixture(kind, bar):
    dev = gpu_device()
    g = hd.sample_fixture()
    run = g["runs"][kind]
    model = hd.sample_model(kind, device=dev)
    common = dict(text_embeds=g["text_embeds"].to(dev), cond_scale=g["cond_scale"], use_tqdm=False, return_all_unet_outputs=True)
    nf = lambda t, shape: run["noise"][t].to(dev)
    outs = model.sample(noise_fn=nf, **common)
    assert [tuple(o.shape) for o in outs] == [tuple(o.shape) for o in run["outputs"]]
    eager = model.sample(noise_fn=nf, use_graph=False, **common)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "graph replay != eager"
    errs = [nerr(o, r) for o, r in zip(outs, run["outputs"])]
    far = [nerr(o, r) for o, r in zip(outs, run["outputs_hd64"])]
    print(f"head dim 128 {kind} sample vs reference per stage: {['%.2e' % e for e in errs]} (bar {bar:.0e}); from the head-dim-64 run {['%.2e' % e for e in far]}")
    record_parity(f"headdim128_sample[{kind}]", stage0=errs[0], stage1=errs[1])
    assert max(errs) < bar and min(far) > 10 * bar, (kind, errs, far)
