"""The per-timestep sampler kernels of csrc/sampler.hip (CFG_X0, QUANTILE, DDPM_UPDATE, RANDN, LOWRES_PREP, LINCOMB) on every branch
that a public Imagen option selects, each called through the C ABI and compared with an fp64 restatement written out here.

Bars: normwise relative error <= 1e-6 against fp64 for the fp32 elementwise ops (a handful of fp32 roundings each); selection and copy
work (the quantile, the nearest-resize indices, |x0|, the Philox draws of two ops on one key) bit-exact.  The Box-Muller transform of
RANDN uses the fast __logf / __sincosf, so its bound is an absolute one (see test_randn_matches_philox4x32_box_muller)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import EMULATED, gpu_device, record_parity

pytestmark = pytest.mark.gpu

TOL = 1e-6


@pytest.fixture(scope="module")
def dev():
    return gpu_device()


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o

    return o


def _run(plan):
    plan.run()
    torch.cuda.synchronize()


def nerr64(got, ref):
    """Normwise relative error of a kernel result against an fp64 reference."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).norm() / ref.norm().clamp(min=1e-300)).item()


def guarded(n, dev, fill=float("nan")):
    """A length-n fp32 buffer followed by 64 sentinel words: (buffer, sentinel view).  A kernel that writes past n shows in the sentinel."""
    t = torch.full((n + 64,), fill, device=dev)
    return t[:n], t[n:]


def untouched(sentinel, fill=float("nan")):
    s = sentinel.cpu()
    return bool(s.isnan().all()) if math.isnan(fill) else bool((s == fill).all())


def cosine_coef(T):
    """The [T, 8] coefficient table of a real cosine schedule (schedules.py), as Imagen._stage uploads it."""
    from imagen_pytorch_amd.schedules import GaussianDiffusionContinuousTimes

    return GaussianDiffusionContinuousTimes(noise_schedule="cosine", timesteps=T).step_coefficients()


# ------------------------------------------------------------------------------------------------ CFG_X0

@pytest.mark.parametrize("objective", ["noise", "x_start", "v"])
@pytest.mark.parametrize("cfg,cond_scale", [(True, 3.0), (True, 7.5), (False, 1.0)], ids=["cfg3", "cfg7.5", "nocfg"])
def test_cfg_x0_objectives(ops, dev, objective, cfg, cond_scale):
    """eps = null + (cond - null) * cond_scale (ip.py:1522; the model output itself without CFG, imagen.py: rows = B), then
    x0 = (x - sigma eps) / max(alpha, 1e-8) (noise, ip.py:314-318), eps (x_start, ip.py:2087-2088), alpha x - sigma eps (v, ip.py:308-312).
    Rows of the cosine table at the first, a middle and the last step, picked by the device counter, plus one row whose alpha lies below
    the 1e-8 clamp.  B * n is not a multiple of the 256-wide block: the last block is partial."""
    torch.manual_seed(31)
    B, n, T = 3, 1001, 10
    coef = torch.cat((cosine_coef(T), cosine_coef(T)[:1]))
    coef[T, 0] = 3e-9                                     # below the clamp: x0 divides by 1e-8, not by alpha
    x = torch.randn(B, n)
    pred = torch.randn((2 if cfg else 1) * B, n) * 1.3
    cd = coef.to(dev)
    xd, pd = x.to(dev), pred.to(dev)
    errs = {}
    for step_i in (0, T // 2, T - 1, T):
        alpha, sigma = coef[step_i, 0].double(), coef[step_i, 1].double()
        p64, x64 = pred.double(), x.double()
        eps = p64[B:] + (p64[:B] - p64[B:]) * cond_scale if cfg else p64
        if objective == "noise":
            ref = (x64 - sigma * eps) / max(alpha.item(), 1e-8)
        elif objective == "x_start":
            ref = eps
        else:
            ref = alpha * x64 - sigma * eps
        x0, x0_tail = guarded(B * n, dev)
        ab, ab_tail = guarded(B * n, dev)
        step = torch.tensor([step_i], dtype=torch.int32, device=dev)
        plan = ops.Plan()
        ops.cfg_x0(plan, xd, pd, cd, step, x0, ab, B=B, n_per_sample=n, cfg=cfg, cond_scale=cond_scale, objective=objective)
        _run(plan)
        got = x0.cpu().view(B, n)
        errs[step_i] = e = nerr64(got, ref)
        assert e <= TOL, (step_i, e)
        assert torch.equal(ab.cpu().view(B, n), got.abs()), "absx0 must be |x0| bit for bit"
        assert untouched(x0_tail) and untouched(ab_tail), "wrote past B * n_per_sample"
        assert int(step.item()) == step_i, "CFG_X0 reads the counter, it does not advance it"
        if objective == "x_start" and not cfg:
            assert torch.equal(got, pred), "x_start without CFG is a copy"
    if objective == "noise":   # the clamp row: dividing by alpha itself would be 3.3x off
        assert errs[T] <= TOL
    record_parity(f"cfg_x0[{objective}-{cfg}-{cond_scale}]", **{f"step{k}": v for k, v in errs.items()})


# ------------------------------------------------------------------------------------------------ DDPM_UPDATE

def _ddpm_ref(x, x0, quant, coef_row, noise, dyn):
    """ip.py:2094-2109 (threshold), 252-270 (posterior), 2160-2164 (noise, nonzero mask) in fp64 from the kernel's fp32 inputs."""
    alpha, _, alpha_n, sigma_n, c, nz = (v.item() for v in coef_row[:6].double())
    x0 = x0.double()
    if dyn:
        s = quant.double().clamp(min=1.0).view(-1, 1)
        x0t = torch.maximum(torch.minimum(x0, s), -s) / s
    else:
        x0t = x0.clamp(-1.0, 1.0)
    mean = alpha_n * (x.double() * (1 - c) / alpha + c * x0t)
    return mean + nz * math.sqrt(max(sigma_n * sigma_n * c, 1e-20)) * noise.double(), x0t


@pytest.mark.parametrize("dyn", [False, True], ids=["clamp", "dynamic"])
@pytest.mark.parametrize("with_thr", [False, True], ids=["no_x0_thr", "x0_thr"])
def test_ddpm_update_branches(ops, dev, dyn, with_thr):
    """Static clamp to [-1, 1] (ip.py:2107) and dynamic thresholding by max(q, 1) (ip.py:2103-2105) with quantile rows below and above 1;
    the thresholded x0 written to x0_thr (self-conditioning) or not; injected noise.  At the last step the nonzero mask removes the noise
    and final_out = (clamp(x, -1, 1) + 1) / 2 (ip.py:2281-2288) is written; at every other step final_out is left alone."""
    torch.manual_seed(32)
    B, n, T = 4, 4 * 251, 10
    coef = cosine_coef(T)
    x = torch.randn(B, n)
    x0 = torch.randn(B, n) * torch.tensor([0.4, 1.5, 3.0, 6.0]).view(B, 1)
    quant = torch.tensor([0.25, 1.0, 2.5, 4.75])        # max(q, 1) clamps the first two rows to 1
    noise = torch.randn(B, n) * 3.0
    errs = {}
    for step_i in (1, T // 2, T - 1):
        xd = x.clone().to(dev)
        final, final_tail = guarded(B * n, dev, 123.0)
        thr, thr_tail = guarded(B * n, dev, 77.0) if with_thr else (None, None)
        step = torch.tensor([step_i], dtype=torch.int32, device=dev)
        plan = ops.Plan()
        ops.ddpm_update(plan, xd, x0.to(dev), quant.to(dev) if dyn else None, coef.to(dev), noise.to(dev), final, step, B=B,
                        n_per_sample=n, dynamic_threshold=dyn, total_steps=T, seed=0, stream_id=0, x0_thr=thr)
        _run(plan)
        ref, x0t = _ddpm_ref(x, x0, quant, coef[step_i], noise, dyn)
        errs[step_i] = e = nerr64(xd, ref)
        assert e <= TOL, (step_i, e)
        assert int(step.item()) == step_i + 1
        if with_thr:
            assert nerr64(thr.view(B, n), x0t) <= TOL and untouched(thr_tail, 77.0)
            assert thr.cpu().abs().max() <= 1.0
        last = step_i == T - 1
        if last:
            assert coef[step_i, 5] == 0
            noiseless, _ = _ddpm_ref(x, x0, quant, coef[step_i], torch.zeros_like(noise), dyn)
            assert nerr64(xd, noiseless) <= TOL, "nonzero = 0 at the last step: no noise"
            want = (xd.cpu().clamp(-1, 1) + 1) * 0.5
            assert torch.equal(final.cpu(), want.view(-1))
        else:
            assert untouched(final, 123.0), "final_out is written at the last step only"
        assert untouched(final_tail, 123.0)
    record_parity(f"ddpm_update[{dyn}-{with_thr}]", **{f"step{k}": v for k, v in errs.items()})


# ------------------------------------------------------------------------------------------------ QUANTILE

QS = (0.0, 0.5, 0.9, 0.95, 0.99, 0.995, 1.0)


def _quantile_rows(B, n, seed):
    """B rows of |x0|-like keys, each from its own distribution: gaussian, mostly exact zeros, heavy ties at the 0.95 rank, values over
    many binades, subnormals, +inf (the x0 of a clamped alpha overflowing), uniform, constant."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        kind = b % 8
        if kind == 0:
            r = torch.randn(n, generator=g).abs() * 0.7
        elif kind == 1:
            r = torch.rand(n, generator=g)
            r[torch.rand(n, generator=g) < 0.97] = 0.0
        elif kind == 2:
            r = torch.rand(n, generator=g) * 2
            r[torch.randperm(n, generator=g)[: max(1, n // 5)]] = 1.375      # a block of ties around the upper ranks
            r[torch.randperm(n, generator=g)[: max(1, n // 8)]] = r.max()
        elif kind == 3:
            r = torch.exp2(torch.rand(n, generator=g) * 250 - 125)
        elif kind == 4:
            bits = torch.randint(1, 1 << 23, (n,), generator=g, dtype=torch.int32)
            r = bits.view(torch.float32).clone()
            r[torch.rand(n, generator=g) < 0.3] = 1e-30
        elif kind == 5:
            r = torch.randn(n, generator=g).abs() * 1e30
            r[torch.rand(n, generator=g) < 0.02] = float("inf")
        elif kind == 6:
            r = torch.rand(n, generator=g) * 5
        else:
            r = torch.full((n,), 2.5)
        rows.append(r)
    return torch.stack(rows).contiguous()


def _same(a, b):
    """Equal values (inf - inf in the interpolation gives NaN for both torch.lerp and the kernel)."""
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("n", [2, 3, 5, 1000, 3 * 24 * 24, 3 * 256 * 256, 3 * 1024 * 1024])
def test_quantile_matches_torch_quantile(ops, dev, n):
    """torch.quantile(a, q, dim=-1) bit for bit (fp32 rank q * (n - 1), torch.lerp), ip.py:2097-2101, at every q the percentile option
    takes and the sizes of every stage; n = 3 * 1024^2 (a 1024^2 SR stage) runs the launcher's capped grid (64 blocks per sample).
    One plan is replayed on dataset A, B, then A again: each answer must be its own data's, so the op re-clears its scratch."""
    if EMULATED and n > 3 * 256 * 256:
        pytest.skip("3 * 1024^2 keys x 8 rows are too slow for the CPU emulation; runs on hardware")
    B = 8 if n < 3 * 1024 * 1024 else 4
    data = [_quantile_rows(B, n, 100 + n), _quantile_rows(B, n, 200 + n)]
    data[1] = data[1][torch.randperm(B)]                   # a different distribution in every row slot
    refs = [torch.stack([torch.quantile(d[b], torch.tensor(QS), dim=-1) for b in range(B)], dim=1) for d in data]   # [len(QS), B]
    W = ops.ENUMS["IMAGEN_QUANTILE_SCRATCH_WORDS"]
    src = torch.empty(B, n, device=dev)
    scratch = torch.empty(B * W, dtype=torch.int32, device=dev)
    outs = torch.empty(len(QS), B, device=dev)
    plan = ops.Plan()
    for j, q in enumerate(QS):
        ops.quantile(plan, src, outs[j], scratch, B=B, n=n, q=q)
    for which in (0, 1, 0):
        src.copy_(data[which].to(dev))
        outs.fill_(-1.0)
        _run(plan)
        got = outs.cpu()
        for j, q in enumerate(QS):
            assert _same(got[j], refs[which][j]), (which, q, got[j], refs[which][j])
    assert not _same(refs[0], refs[1])


# ------------------------------------------------------------------------------------------------ Philox4x32-10 + Box-Muller

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123): 10 rounds of the (0xD2511F53, 0xCD9E8D57) multiply-xor S-box, key bumped by
    (0x9E3779B9, 0xBB67AE85) after each round."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_normal_ref(B, n_per_sample, *, seed, tag, stream_id, sample_offset):
    """fp64 Box-Muller of the kernel's philox_normal4: counter (i / 4, tag, stream_id, sample_offset + b), key = seed (lo, hi);
    u = (float(c) + 0.5) * 2^-32 in fp32 as the kernel forms it, then r = sqrt(-2 log max(u, 1e-12)) paired with cos / sin of 2 pi u."""
    f = np.float32
    out = np.empty((B, n_per_sample), dtype=np.float64)
    key = (seed & M32, (seed >> 32) & M32)
    for b in range(B):
        for g in range(n_per_sample // 4):
            c = philox4x32_10((g, tag, stream_id, (sample_offset + b) & M32), key)
            u = [float((f(v) + f(0.5)) * f(2.3283064365386963e-10)) for v in c]
            r0, r1 = (math.sqrt(-2.0 * math.log(max(v, 1e-12))) for v in (u[0], u[2]))
            out[b, 4 * g:4 * g + 4] = (r0 * math.cos(2 * math.pi * u[1]), r0 * math.sin(2 * math.pi * u[1]),
                                       r1 * math.cos(2 * math.pi * u[3]), r1 * math.sin(2 * math.pi * u[3]))
    return torch.from_numpy(out)


def test_philox_reference_known_answers():
    """The restatement above against the Random123 known-answer vectors of philox4x32_10 (kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((M32,) * 4, (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert philox4x32_10(ctr, key) == want


# The kernel's fast __logf / __sincosf against fp64 log / sin / cos: measured worst |kernel - fp64| 1.14e-6 on the CPU emulation and
# 1.08e-6 on the MI355X (3 * 1000 draws).  A swapped output pair, a counter word off by one or a wrong key word moves a draw by O(1).
RANDN_ABS = 1e-5

SEED64 = 0x9E3779B97F4A7C15   # high word nonzero (and above 2^31)


def _randn(ops, dev, B, n, **kw):
    out = torch.full((B, n), float("nan"), device=dev)
    plan = ops.Plan()
    ops.randn(plan, out, **kw)
    _run(plan)
    return out.cpu()


def test_randn_matches_philox4x32_box_muller(ops, dev):
    """IMAGEN_OP_RANDN (the init and low-res augmentation noise of every non-injected sample) against the fp64 Box-Muller of the
    Philox restatement, B > 1 with a nonzero sample offset and a 64-bit key; shard invariance bit for bit."""
    B, n = 3, 1000
    kw = dict(seed=SEED64, stream_id=5, tag=0x7FFF0002, sample_offset=11)
    got = _randn(ops, dev, B, n, **kw)
    ref = philox_normal_ref(B, n, **kw)
    worst = (got.double() - ref).abs().max().item()
    record_parity("randn_vs_fp64_box_muller", max_abs=worst, normwise=nerr64(got, ref))
    assert worst <= RANDN_ABS, worst
    # the bound does tell a wrong generator apart: each of these misses by O(1) somewhere
    for wrong in (dict(kw, seed=SEED64 ^ (1 << 32)), dict(kw, sample_offset=12), dict(kw, tag=kw["tag"] + 1)):
        assert (got.double() - philox_normal_ref(B, n, **wrong)).abs().max() > 0.5
    assert (got.double() - ref.view(B, -1, 2).flip(-1).reshape(B, n)).abs().max() > 0.5
    # shard invariance: samples 2..3 of a batch of 4 are what a batch of 2 starting at global sample 2 draws
    full = _randn(ops, dev, 4, 64, seed=SEED64, stream_id=1, tag=3, sample_offset=0)
    part = _randn(ops, dev, 2, 64, seed=SEED64, stream_id=1, tag=3, sample_offset=2)
    assert torch.equal(full[2:], part)


def test_ddpm_update_draws_the_randn_stream(ops, dev):
    """DDPM_UPDATE without injected noise draws exactly RANDN's numbers for tag = step, the same stream_id, sample index and key (the
    seed_lo/hi and the device seed_ptr forms alike): with mean 0 and unit variance the step writes the draw itself."""
    B, n, step_i = 3, 4 * 65, 6
    coef = torch.tensor([[1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]] * 8)   # alpha = alpha_next = sigma_next = c = nonzero = 1: x' = z
    want = _randn(ops, dev, B, n, seed=SEED64, stream_id=9, tag=step_i, sample_offset=4)
    for use_ptr in (False, True):
        x = torch.zeros(B, n, device=dev)
        step = torch.tensor([step_i], dtype=torch.int32, device=dev)
        seed_ptr = torch.tensor([SEED64 & M32, SEED64 >> 32], dtype=torch.int64).to(torch.int32).to(dev) if use_ptr else None
        plan = ops.Plan()
        ops.ddpm_update(plan, x, torch.zeros(B, n, device=dev), None, coef.to(dev), None, None, step, B=B, n_per_sample=n,
                        dynamic_threshold=False, total_steps=8, seed=0 if use_ptr else SEED64, stream_id=9, sample_offset=4, seed_ptr=seed_ptr)
        _run(plan)
        assert torch.equal(x.cpu(), want), use_ptr
    assert (want.double() - philox_normal_ref(B, n, seed=SEED64, tag=step_i, stream_id=9, sample_offset=4)).abs().max() <= RANDN_ABS


# ------------------------------------------------------------------------------------------------ LOWRES_PREP

LOWRES_SIZES = [((16, 16), (64, 64)), ((64, 64), (256, 256)), ((32, 32), (32, 32)), ((24, 24), (64, 64)), ((64, 64), (16, 16)),
                ((14, 14), (46, 46)), ((6, 6), (74, 74)), ((16, 16), (328, 328)), ((14, 6), (46, 74))]


@pytest.mark.parametrize("src,dst", LOWRES_SIZES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in LOWRES_SIZES])
def test_lowres_prep_matches_interpolate_nearest(ops, dev, src, dst):
    """alpha * (F.interpolate(img, size, mode='nearest') * 2 - 1) + sigma * noise (ip.py:2443-2449, 272-284).  Torch's nearest takes
    source row floor(dst * float(in / out)) in fp32; for 14 -> 46, 6 -> 74 and 16 -> 328 that differs from the integer dst * in // out,
    so the in-kernel indices must be torch's fp32 ones.  With alpha = 1, sigma = 0 the result is the resize itself, bit for bit."""
    torch.manual_seed(33)
    B, C = 2, 3
    img = torch.rand(B, C, *src)
    noise = torch.randn(B, C, *dst)
    up = F.interpolate(img, dst, mode="nearest")
    imgd = img.to(dev)
    for alpha, sigma, nz in ((1.0, 0.0, torch.zeros_like(noise)), (1.0, 0.0, noise), (0.9797959, 0.2, noise), (0.6, 0.8, noise)):
        out, tail = guarded(B * C * dst[0] * dst[1], dev)
        out = out.view(B, C, *dst)
        plan = ops.Plan()
        ops.lowres_prep(plan, imgd, nz.to(dev), out, alpha=alpha, sigma=sigma)
        _run(plan)
        got = out.cpu()
        assert untouched(tail)
        if sigma == 0.0:
            assert torch.equal(got, up * 2 - 1), "nearest source indices differ from torch's"
        else:
            a, s = torch.tensor(alpha).double(), torch.tensor(sigma).double()   # the kernel's fp32 scalars, exactly
            e = nerr64(got, a * (up.double() * 2 - 1) + s * nz.double())
            assert e <= TOL, e


# ------------------------------------------------------------------------------------------------ LINCOMB

@pytest.mark.parametrize("final", [False, True])
def test_lincomb_threshold_terms_and_final(ops, dev, final):
    """ElucidatedImagen's state update: out = w0 t0 + w1 thr(t1) + w2 t2 + w3 thr(t3), thr(t) = clamp(t, -s, s) / s with s = max(q, 1)
    per sample (thr_mode 1: the dynamic threshold of its x0 estimates, ip.py:2094-2105 via elucidated_imagen.py), out2 = w5 * out,
    final_out = (clamp(out, -1, 1) + 1) / 2 only when `final` is set; the weight row is the device counter's."""
    torch.manual_seed(34)
    B, n = 4, 4 * 125
    t0, t1, t2, t3 = (torch.randn(B, n) * s for s in (1.0, 2.5, 0.7, 4.0))
    q1, q3 = torch.tensor([0.5, 1.0, 1.8, 3.2]), torch.tensor([2.7, 0.9, 1.25, 0.1])
    coef = torch.zeros(3, 8)
    coef[1, :6] = torch.tensor([0.83, -0.41, 0.27, 0.64, 0.0, -1.7])
    out, out2 = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
    fin, fin_tail = guarded(B * n, dev, 55.0)
    step = torch.tensor([1], dtype=torch.int32, device=dev)
    plan = ops.Plan()
    ops.lincomb(plan, t0.to(dev), out, coef.to(dev), step, B=B, n_per_sample=n, t1=t1.to(dev), t2=t2.to(dev), t3=t3.to(dev),
                q1=q1.to(dev), q3=q3.to(dev), out2=out2, final_out=fin, thr_mode=1, final=final)
    _run(plan)
    w = coef[1].double()

    def thr(t, q):
        s = q.double().clamp(min=1.0).view(-1, 1)
        return torch.maximum(torch.minimum(t.double(), s), -s) / s

    ref = w[0] * t0.double() + w[1] * thr(t1, q1) + w[2] * t2.double() + w[3] * thr(t3, q3)
    e = nerr64(out, ref)
    assert e <= TOL, e
    assert nerr64(out2, w[5] * ref) <= TOL
    # without thresholding (thr_mode 0) the same terms enter as they are: the clamp does bite on this data
    assert nerr64(out, w[0] * t0 + w[1] * t1 + w[2] * t2 + w[3] * t3) > 1e-2
    if final:
        assert torch.equal(fin.cpu().view(B, n), (out.cpu().clamp(-1, 1) + 1) * 0.5)
    else:
        assert untouched(fin, 55.0)
    assert untouched(fin_tail, 55.0) and int(step.item()) == 1
    record_parity(f"lincomb_thr[{final}]", out=e)


def test_lincomb_noise_keys(ops, dev):
    """LINCOMB's Philox column: the device seed_ptr and the seed_lo/hi fields give the same draws for one key, and they are RANDN's
    draws for tag = step (one generator for every sampler op)."""
    B, n, step_i = 2, 4 * 70, 2
    coef = torch.zeros(4, 8)
    coef[step_i, 4] = 1.0                                   # out = 0 * t0 + 1 * z
    zeros = torch.zeros(B, n, device=dev)
    seed_ptr = torch.tensor([SEED64 & M32, SEED64 >> 32], dtype=torch.int64).to(torch.int32).to(dev)
    got = []
    for kw in (dict(seed=SEED64), dict(seed_ptr=seed_ptr)):
        out = torch.empty(B, n, device=dev)
        step = torch.tensor([step_i], dtype=torch.int32, device=dev)
        plan = ops.Plan()
        ops.lincomb(plan, zeros, out, coef.to(dev), step, B=B, n_per_sample=n, stream_id=0x301, sample_offset=7, **kw)
        _run(plan)
        got.append(out.cpu())
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0], _randn(ops, dev, B, n, seed=SEED64, stream_id=0x301, tag=step_i, sample_offset=7))
