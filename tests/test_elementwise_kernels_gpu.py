"""The glue kernels of csrc/elementwise.hip (ROWSTAT, GATE_RESIDUAL, LN_RESIDUAL, QNORM, KV_PREP / KV_PREP_MULTI, SELECT_ROWS, MEAN_ROWS,
MEMSET32, ROWS_COPY, PACK_IMAGE, TIME_EMBED, SCALE_SHIFT, ACT_PREP with and without self_stat, STEP_SLICE) on every branch that an engine
call site selects, each called through the C ABI and compared with an fp64 restatement written out here from the values the kernel reads.

Bars (derived from the arithmetic, not measured; u = 2^-24 is the unit roundoff of fp32, ulp32 = 2^-23 its relative spacing):
 * copies and selections: bit-exact.
 * fp32 row statistics: per row, `sum_bound` (the summation tree) plus 2 ulp32 for sqrt / rsqrt / the division.
 * fp16 outputs of fp32 arithmetic: per element |got - ref64| <= ulp16(ref64) + d, d = k u sum|terms| of the final expression (k counted
   in a comment at each use): the stored value is one of the two fp16 neighbours of the exact result.  The share of elements that differ
   from round_fp16(ref64) at all is recorded, not asserted.
 * statistics of stored rows: the reference is computed from the fp16 rows the kernel stored, at the fp32-statistics bar.
Every output lies inside a larger allocation whose other words (64 before, 64 after, the gaps between strided rows) hold a sentinel that must
survive the launch; the gaps of every strided INPUT hold NaN, so a read beside a row shows as well."""
import math

import pytest
import torch

from conftest import EMULATED, gpu_device, record_parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
ULP32 = 2.0 ** -23      # relative spacing of fp32 (one ulp of a hardware rcp / rsq / exp2 / sqrt / division)
LOG2E = 1.4426950408889634

SENT = {torch.float16: (torch.int16, 0x7E7B), torch.float32: (torch.int32, 0x7FC0DEAD), torch.int32: (torch.int32, 0x5A5A5A5B)}   # NaNs; an odd word
GUARD_BYTES = 256       # 64 32-bit words on either side


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


# ------------------------------------------------------------------------------------------------ helpers

class guarded:
    """An output of `numel` elements of `dtype` inside a larger allocation: 64 sentinel words before it, 64 after it, and the output itself
    pre-filled with the sentinel too, so that with a strided output (ld > C, channel slices, token slices, the J..Jp padding of K-hat / V^T)
    the gaps between the rows are sentinels as well.  `.t` is the device view the kernel gets; `check(mask)` asserts that every word outside
    `mask` (a bool tensor over the numel elements: where the kernel is meant to write; None = everywhere) still holds the sentinel bits."""

    def __init__(self, numel, dev, dtype=torch.float16):
        self.idt, self.word = SENT[dtype]
        self.pad = GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
        self.numel = numel
        self.full = torch.full((numel + 2 * self.pad,), self.word, dtype=self.idt).view(dtype).to(dev)
        self.t = self.full[self.pad:self.pad + numel]

    def cpu(self):
        return self.full.cpu()[self.pad:self.pad + self.numel].clone()

    def act(self, ops, B, R, C, ld=None, bs=None, lead=0):
        ld = C if ld is None else ld
        bs = R * ld if bs is None else bs
        return ops.Act(self.full, B, 1, R, C, ld, bs, self.pad + lead)

    def check(self, mask=None):
        bits = self.full.cpu().view(self.idt)
        free = torch.ones(bits.numel(), dtype=torch.bool)
        if mask is None:
            free[self.pad:self.pad + self.numel] = False
        else:
            free[self.pad:self.pad + self.numel] = ~mask.reshape(-1)
        bad = (bits[free] != self.word).nonzero()
        assert bad.numel() == 0, f"{bad.numel()} sentinel words overwritten, first at free-word index {int(bad[0])}"


def span(B, R, C, ld, bs, lead=0):
    """Elements that rows [B, R, C] at b * bs + r * ld + lead occupy, first to last."""
    return lead + (B - 1) * bs + (R - 1) * ld + C


def rows_mask(numel, B, R, C, ld, bs, lead=0):
    m = torch.zeros(numel, dtype=torch.bool)
    m.as_strided((B, R, C), (bs, ld, 1), lead).fill_(True)
    return m


def rows_read(flat, B, R, C, ld, bs, lead=0):
    return flat.as_strided((B, R, C), (bs, ld, 1), flat.storage_offset() + lead).clone()


def strided16(ops, vals, ld, bs, dev, lead=0):
    """fp16 rows [B, R, C] as an Act at b * bs + r * ld + lead of a buffer whose every other element is NaN."""
    B, R, C = vals.shape
    buf = torch.full((span(B, R, C, ld, bs, lead) + 8,), float("nan"), dtype=torch.float16)
    buf.as_strided((B, R, C), (bs, ld, 1), lead).copy_(vals)
    return ops.Act(buf.to(dev), B, 1, R, C, ld, bs, lead)


def h16(t):
    return t.to(torch.float16)


def ulp16(x):
    """The spacing of fp16 at |x|: 2^(floor(log2 |x|) - 10), and 2^-24 below 2^-14 (subnormals and zero)."""
    _, e = torch.frexp(x.double().abs().clamp(min=2.0 ** -30))   # |x| = m 2^e, m in [0.5, 1); frexp(0) would answer e = 0
    return torch.exp2((e - 1).clamp(min=-14).double() - 10)


def test_ulp16_is_the_fp16_spacing():
    """The yardstick of every fp16 bar against torch's own fp16: the distance to the next representable value, at zero, in the subnormals,
    at the first normal binade, at powers of two and just below them, at the largest finite value."""
    x = torch.tensor([0.0, 2.0 ** -24, 3e-6, 2.0 ** -14, 2.0 ** -14 * 1.5, 2.0 ** -13, 0.999, 1.0, 1.5, 2.0, 1000.0, 65504.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -24] * 5 + [2.0 ** -23, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 32.0], dtype=torch.float64)
    assert torch.equal(ulp16(x), want) and torch.equal(ulp16(-x), want)
    h = x[:-1].to(torch.float16)                                     # (representable values: the next fp16 above each is ulp16 away)
    nxt = (h.view(torch.int16) + 1).view(torch.float16)
    assert torch.equal(nxt.double() - h.double(), ulp16(h))


def row_err(got, ref, scale=None):
    """Per-row relative error in fp64: (maximum over rows, index of the worst row).  Rows of values: |got - ref|_2 / |ref|_2 of each row;
    one statistic per row: |got - ref| / scale (scale: what the bound is relative to; |ref| by default)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if got.ndim > 1:
        e = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1).clamp(min=1e-300)
    else:
        e = (got - ref).abs() / (ref.abs() if scale is None else scale.double()).clamp(min=1e-300)
    e = torch.nan_to_num(e, nan=float("inf"))
    i = int(e.argmax())
    return float(e[i]), i


def host_lpr(groups):
    l = 1
    while l < groups and l < 64:
        l <<= 1
    return l


def sum_bound(groups_per_lane, lpr, extra=4):
    """A-priori relative error (against the sum of |terms|) of the kernels' row sums.  A lane adds the 8 values of each of its groups one
    after the other (8 * groups_per_lane additions, the first onto 0), then log2(lpr) butterfly additions follow; a chain of n fp32 additions
    is off by at most n u sum|terms| to first order.  The squares of fp16 values are exact in fp32 (11 x 11 bits), so the terms themselves
    carry no rounding.  `extra` = 4 more roundings for what surrounds the sum (the w2 product and the s1 + w2 s2 addition, or a 1 / C)."""
    return (8 * groups_per_lane + int(math.log2(lpr)) + extra) * U


def lane_groups(C1, C2=0):
    """(groups a lane walks, lanes per row) for a row of C1 (+ C2) channels.  The kernels walk x1 and x2 in two loops of their own, so a lane
    takes ceil(g1 / lpr) + ceil(g2 / lpr) groups: one more than ceil((g1 + g2) / lpr) where neither count divides (C1 = 8 with C2 = 40: 2 groups,
    23 u, where a single loop over both would give 15 u).  With one tensor the two counts are the same."""
    lpr = host_lpr((C1 + C2) // 8)
    return -(-(C1 // 8) // lpr) + -(-(C2 // 8) // lpr), lpr


def ln_stat_bounds(x, eps, C1, C2=0):
    """Bounds for the two-pass LayerNorm statistics of rows x (fp64 [rows, C]): (|mean error|, relative error of rstd).
    mean = sum / C: sum_bound against sum|x|, one more rounding for the division (inside sum_bound's extra).  The variance pass adds
    d^2 with d = x - mean_computed: d carries one rounding and the square one (3 u per term, to first order), the chain sum_bound, and the error
    dm of the mean enters only in second order because sum(x - mean) = 0:  sum (x - m - dm)^2 = q + C dm^2.  Then var + eps (one rounding),
    rsqrt (half the relative error of its argument, 1 ulp32 of its own)."""
    n, lpr = lane_groups(C1, C2)
    C = x.shape[-1]
    dm = sum_bound(n, lpr) * x.abs().sum(-1) / C
    var = x.var(-1, unbiased=False)
    dvar = (sum_bound(n, lpr) + 3 * U) * var + dm * dm
    rho = 0.5 * (dvar / (var + eps) + 2 * U) + 2 * ULP32
    return dm, rho


FIGS = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    """One parity record per kernel, written when the module's last test has run."""
    yield
    for kernel, rec in FIGS.items():
        record_parity("elementwise." + kernel, **{k: v for k, v in rec.items() if not k.startswith("_")})


def note(kernel, **figs):
    """Keep the worst of each figure of a kernel over the cases run (`differs` = (elements that differ from round_fp16(ref64), elements
    compared) is summed into a share)."""
    rec = FIGS.setdefault(kernel, {})
    for k, v in figs.items():
        if k == "differs":
            a, b = rec.get("_differs", (0, 0))
            rec["_differs"] = (a + v[0], b + v[1])
            rec["differs_from_nearest_share"] = (a + v[0]) / max(b + v[1], 1)
        else:
            rec[k] = max(rec.get(k, 0.0), v)


def check16(kernel, got, ref, d, what=""):
    """fp16 output of fp32 arithmetic: every element within ulp16(ref) + d of the fp64 reference, i.e. one of the two fp16 neighbours of the
    exact result (d: the fp32 evaluation's own error bound).  Records the worst per-row error and the share that is not the nearest fp16."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (what, "non-finite output")
    over = (got - ref).abs() - (ulp16(ref) + d)
    worst, row = row_err(got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]))
    differs = int((got != ref.to(torch.float16).double()).sum())
    note(kernel, worst_row_err=worst, differs=(differs, got.numel()))
    i = int(over.argmax())
    assert float(over.flatten()[i]) <= 0, (what, f"element {i} (row {i // got.shape[-1]}): got {got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r} "
                                           f"over the bar by {over.flatten()[i].item():.3e}; worst row {row}: {worst:.3e}")


def check_stat(kernel, name, got, ref, bound, scale=None):
    """One fp32 statistic per row against fp64: |got - ref| <= bound * scale (scale = |ref| when the bound is relative to the result)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs() if scale is None else scale
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, bound)
    worst, row = row_err(got, ref, scale)
    note(kernel, **{name + "_worst_row_err": worst})
    ok = (got - ref).abs() <= bound * scale
    assert bool(ok.all()), (name, f"row {int((~ok).nonzero()[0])}: got {got[~ok][0].item()!r} ref {ref[~ok][0].item()!r}; worst row {row}: {worst:.3e} "
                                  f"(bound {bound[row].item():.3e})")


def silu64(v):
    return v * torch.sigmoid(v)


def silu_d(v):
    """silu_f = v * rcp(1 + exp2(-log2e v)): the product with log2e is one rounding of the exponent (u |v| log2e ln2 = u |v| relative on
    exp2), v_exp 1 ulp32 (2 u), the addition u, v_rcp 1 ulp32 (2 u), the last product u: (6 + |v|) u relative to the result."""
    return (6 + v.abs()) * U * silu64(v).abs()


def gelu64(v):
    return 0.5 * v * torch.erfc(-v / math.sqrt(2.0))


def gelu_d(v):
    """gelu_f = 0.5 v (2 - ec | ec), ec = poly(t) exp2(-log2e x^2), t = rcp(1 + 0.3275911 x), x = |v| / sqrt 2: the approximation is off by at
    most 1.5e-7 absolute in ec (common.h).  Rounding of ec, absolute: t carries 4 u + 1 ulp32 (6 u) and moves poly by at most sum k |a_k| = 14.1
    times that (85 u); the five Horner steps round twice each on partial values below sum |a_k| = 4.5 (45 u); exp2 1 ulp32 plus its argument's
    three roundings, 3 u x^2 exp(-x^2) <= 1.2 u; the product u: below 136 u in all.  The two outer products: 2 u relative to the result."""
    return 0.5 * v.abs() * (1.5e-7 + 136 * U) + 2 * U * gelu64(v).abs()


# ------------------------------------------------------------------------------------------------ ROWSTAT

def _stat_rows(B, HW, C, seed):
    """fp16 rows [B, HW, C]: gaussian rows, one all-zero row, two rows of mean 30 and sd 0.05 (the two-pass variance), one row of large values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, C, generator=g) * 0.8 + 0.2
    x[0, 4] = 0.0
    x[1, 2] = 30.0 + 0.05 * torch.randn(C, generator=g)
    x[1, 3] = 30.0 + 0.05 * torch.randn(C, generator=g)
    x[2, 0] = torch.randn(C, generator=g) * 40.0
    return h16(x)


@pytest.mark.parametrize("form", ["x1", "x2_w0.5", "x2_w1"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C1", [8, 16, 24, 32, 64, 96, 256, 512, 520, 1024, 4096])
def test_rowstat(ops, dev, C1, mode, form):
    """B = 3 images of H * W = 5 pixels (15 rows: no multiple of the 4 .. 256 rows of a block, rows of several images in one block), x1 and x2
    channel slices of wider buffers (ld > C, bs > rows * ld), C2 = 40 channels of a second tensor weighted by w2."""
    B, HW = 3, 5
    two = form != "x1"
    w2 = 0.5 if form == "x2_w0.5" else 1.0
    C2 = 40 if two else 0
    x1 = _stat_rows(B, HW, C1, 1000 + C1)
    x2 = _stat_rows(B, HW, C2, 2000 + C1) if two else None
    a1 = strided16(ops, x1, C1 + 16, HW * (C1 + 16) + 24, dev, lead=8)
    a2 = strided16(ops, x2, C2 + 8, HW * (C2 + 8) + 40, dev, lead=16) if two else None
    rs, mu = guarded(B * HW, dev, torch.float32), guarded(B * HW, dev, torch.float32)
    plan = ops.Plan()
    ops.rowstat(plan, a1, mode=mode, rs=rs.t, mu=mu.t if mode == 1 else None, x2=a2, w2=w2, eps=1e-5)
    _run(plan)
    rs.check()
    mu.check(None if mode == 1 else torch.zeros(B * HW, dtype=torch.bool))
    n, lpr = lane_groups(C1, C2)
    v1 = x1.double().reshape(B * HW, C1)
    v2 = x2.double().reshape(B * HW, C2) if two else torch.zeros(B * HW, 0, dtype=torch.float64)
    got = rs.cpu()
    if mode == 1:
        v = torch.cat((v1, v2), -1)
        dm, rho = ln_stat_bounds(v, 1e-5, C1, C2)
        check_stat("rowstat", "mu", mu.cpu(), v.mean(-1), dm + U * v.mean(-1).abs(), scale=torch.ones(B * HW, dtype=torch.float64))
        check_stat("rowstat", "rs_ln", got, torch.rsqrt(v.var(-1, unbiased=False) + 1e-5), rho)
        assert got[4].item() == pytest.approx(1e-5 ** -0.5, rel=1e-6)           # the all-zero row: rsqrt(eps)
    else:
        tot = (v1 * v1).sum(-1) + float(torch.tensor(w2)) * (v2 * v2).sum(-1)
        if mode == 2:
            check_stat("rowstat", "ssq", got, tot, sum_bound(n, lpr))
            assert got[4].item() == 0.0
        else:
            check_stat("rowstat", "rs_rms", got, 1.0 / tot.sqrt().clamp(min=1e-12), 0.5 * sum_bound(n, lpr) + 2 * ULP32)
            assert got[4].item() == pytest.approx(1e12, rel=1e-6)               # the 1e-12 clamp of the norm


# ------------------------------------------------------------------------------------------------ GATE_RESIDUAL

@pytest.mark.parametrize("C", [8, 96, 512, 1024])
@pytest.mark.parametrize("stat", ["none", "inv_norm", "raw_ssq"])
@pytest.mark.parametrize("gated", [False, True], ids=["nogate", "gate"])
def test_gate_residual(ops, dev, gated, stat, C):
    """out = fp16(h * gate[b] + res) on B = 3 images of 7 rows (21 rows: the gate index r / rows_per_batch changes inside a block, the last
    block is partial), every operand with its own row stride > C; rs_out absent, 1 / max(|out|, 1e-12) or the raw sum of squares of the
    STORED row.  Per element k = 2: the product and the addition round once each, relative to |h gate| + |res|."""
    torch.manual_seed(3000 + C)
    B, R = 3, 7
    h, res = h16(torch.randn(B, R, C)), h16(torch.randn(B, R, C) * 1.5)
    res[1, 3] = -h[1, 3]                                   # a cancelling row (gate 1: exactly zero)
    gate = torch.rand(B, C) if gated else None
    ah = strided16(ops, h, C + 8, R * (C + 8), dev)
    ar = strided16(ops, res, C + 16, R * (C + 16), dev)
    ld_o = C + 24
    out = guarded(B * R * ld_o, dev)
    rso = guarded(B * R, dev, torch.float32)
    plan = ops.Plan()
    ops.gate_residual(plan, ah, gate.to(dev) if gated else None, ar, out.act(ops, B, R, C, ld_o), rs_out=None if stat == "none" else rso.t,
                      raw_ssq=stat == "raw_ssq")
    _run(plan)
    out.check(rows_mask(out.numel, B, R, C, ld_o, R * ld_o))
    rso.check(torch.zeros(B * R, dtype=torch.bool) if stat == "none" else None)
    g64 = gate.double().view(B, 1, C) if gated else torch.ones(B, 1, C, dtype=torch.float64)
    got = rows_read(out.cpu(), B, R, C, ld_o, R * ld_o)
    check16("gate_residual", got, h.double() * g64 + res.double(), 2 * U * ((h.double() * g64).abs() + res.double().abs()), (gated, stat, C))
    if stat != "none":
        n, lpr = lane_groups(C)
        tot = (got.double() ** 2).sum(-1).reshape(-1)
        if stat == "raw_ssq":
            check_stat("gate_residual", "ssq_out", rso.cpu(), tot, sum_bound(n, lpr))
        else:
            check_stat("gate_residual", "rs_out", rso.cpu(), 1.0 / tot.sqrt().clamp(min=1e-12), 0.5 * sum_bound(n, lpr) + 2 * ULP32)


# ------------------------------------------------------------------------------------------------ LN_RESIDUAL

@pytest.mark.parametrize("C", [8, 64, 200, 1024])
@pytest.mark.parametrize("stats", ["none", "ssq", "ln", "ssq+ln"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("with_beta", [False, True], ids=["nobeta", "beta"])
def test_ln_residual(ops, dev, with_beta, with_res, stats, C):
    """out = fp16((y - mean) rstd g (+ beta) (+ res)) in the token-slice form of the engine's text-token assembly: the 5 rows of each of B = 3
    batch elements go to tokens 1 .. 5 of a [B, 7, ld] buffer (bs_out > rows_per_batch * ld_out, ld_out > C), the neighbouring tokens and the
    row gaps guarded; y and res with batch strides of their own.  Statistics of the stored rows with eps_out = 1e-3 != eps = 1e-5.
    Per element: the mean's error dm (ln_stat_bounds) scaled by |rstd g|, then relative to |(y - mean) rstd g| + |beta| + |res|: rstd's error
    rho, the subtraction, two products and two additions (k = 5), one more for a contraction that rounds differently (k = 6)."""
    torch.manual_seed(4000 + C)
    B, R, T, eps, eps_out = 3, 5, 7, 1e-5, 1e-3
    y = h16(torch.randn(B, R, C) * 1.2 + 0.4)
    y[2, 1] = h16(30.0 + 0.05 * torch.randn(C))            # large mean, small variance
    res = h16(torch.randn(B, R, C)) if with_res else None
    g, beta = 1 + 0.2 * torch.randn(C), (0.3 * torch.randn(C) if with_beta else None)
    if "ln" in stats:   # stored rows with a variance near eps_out = 1e-3, so that eps_out (and not eps) decides rs_out
        g, beta, res = g * 0.03, (beta * 0.03 if with_beta else None), (h16(res * 0.03) if with_res else None)
    ay = strided16(ops, y, C + 8, R * (C + 8) + 16, dev, lead=8)
    ar = strided16(ops, res, C + 16, R * (C + 16) + 8, dev) if with_res else None
    ld_o = C + 8
    out = guarded(B * T * ld_o, dev)
    ssq, mu_o, rs_o = (guarded(B * R, dev, torch.float32) for _ in range(3))
    plan = ops.Plan()
    ops.ln_residual(plan, ay, g.to(dev), out.act(ops, B, R, C, ld_o, T * ld_o, lead=ld_o), beta=beta.to(dev) if with_beta else None, res=ar, eps=eps,
                    ssq_out=ssq.t if "ssq" in stats else None, ln_stats_out=(mu_o.t, rs_o.t) if "ln" in stats else None, eps_out=eps_out)
    _run(plan)
    out.check(rows_mask(out.numel, B, R, C, ld_o, T * ld_o, ld_o))
    none = torch.zeros(B * R, dtype=torch.bool)
    ssq.check(None if "ssq" in stats else none)
    mu_o.check(None if "ln" in stats else none)
    rs_o.check(None if "ln" in stats else none)
    y64, g64 = y.double(), g.double()
    mean, var = y64.mean(-1, keepdim=True), y64.var(-1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    main = (y64 - mean) * rstd * g64
    ref = main + (beta.double() if with_beta else 0.0) + (res.double() if with_res else 0.0)
    dm, rho = ln_stat_bounds(y64, eps, C)
    terms = main.abs() + (beta.double().abs() if with_beta else 0.0) + (res.double().abs() if with_res else 0.0)
    d = (rstd * g64).abs() * dm.unsqueeze(-1) + (rho.unsqueeze(-1) + 6 * U) * terms
    got = rows_read(out.cpu(), B, R, C, ld_o, T * ld_o, ld_o)
    check16("ln_residual", got, ref, d, (with_beta, with_res, stats, C))
    st = got.double().reshape(B * R, C)
    n, lpr = lane_groups(C)
    if "ssq" in stats:
        check_stat("ln_residual", "ssq_out", ssq.cpu(), (st * st).sum(-1), sum_bound(n, lpr))
    if "ln" in stats:
        dmo, rho_o = ln_stat_bounds(st, eps_out, C)
        check_stat("ln_residual", "mu_out", mu_o.cpu(), st.mean(-1), dmo + U * st.mean(-1).abs(), scale=torch.ones(B * R, dtype=torch.float64))
        check_stat("ln_residual", "rs_out", rs_o.cpu(), torch.rsqrt(st.var(-1, unbiased=False) + eps_out), rho_o)
        assert float(st.var(-1, unbiased=False).max()) < 0.1                     # rows on the scale of eps_out: eps in its place is far outside the bar


# ------------------------------------------------------------------------------------------------ QNORM / KV_PREP

# l2norm(v) * scale (* mult): 7 additions of (exact, for fp16 sources) squares and 3 butterfly additions (10 u on the sum, 5 u after the
# square root), sqrt 1 ulp32 (2 u), the division 1 ulp32 (2 u), two products (2 u): k = 11; fp32 sources round their squares too (+ 1 u / 2);
# one spare for a contraction that rounds differently: k = 13
K_NORM = 13


def _l2norm64(v):
    return v / v.norm(dim=-1, keepdim=True).clamp(min=1e-12)


@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("D", [64, 32])
def test_qnorm(ops, dev, D, heads):
    """q[r, h, :] = l2norm * q_scale * mult in place, 37 rows (rows * heads = 37 | 296: the last block is partial for both head dims),
    ld = heads * D + 16 with the 16 columns beside every row guarded, one all-zero head row, mult = 8 log2(e)."""
    torch.manual_seed(5000 + D + heads)
    rows, ld, mult = 37, heads * D + 16, 8 * LOG2E
    q = h16(torch.randn(rows, heads, D) * 2)
    q[5, heads - 1] = 0.0
    qs = torch.rand(D) + 0.5
    buf = guarded(rows * ld, dev)
    mask = rows_mask(buf.numel, 1, rows, heads * D, ld, rows * ld)
    flat = buf.cpu().clone()
    flat.as_strided((rows, heads * D), (ld, 1), 0).copy_(q.reshape(rows, heads * D))
    buf.t.copy_(flat.to(dev))
    plan = ops.Plan()
    ops.qnorm(plan, buf.t, qs.to(dev), rows=rows, heads=heads, ld=ld, mult=mult, head_dim=D)
    _run(plan)
    buf.check(mask)
    got = rows_read(buf.cpu(), 1, rows, heads * D, ld, rows * ld).view(rows, heads, D)
    ref = _l2norm64(q.double()) * qs.double() * float(torch.tensor(mult))
    check16("qnorm", got, ref, K_NORM * U * ref.abs(), (D, heads))
    assert got[5, heads - 1].abs().sum() == 0


def _kv_job(ops, dev, B, heads, J, Jp, D, dt, r0, seed):
    """One KV_PREP job on fused kv rows [B, J, 2 * heads * D] (k at column 0, v at column heads * D): returns (kwargs, checker)."""
    g = torch.Generator().manual_seed(seed)
    src = (torch.randn(B, J, 2 * heads * D, generator=g) * 1.7).to(dt)
    src[B - 1, J - 1, :D] = 0.0                                                   # a zero k row (head 0)
    ks = torch.rand(D, generator=g) + 0.5
    khat, vt = guarded(B * heads * Jp * D, dev), guarded(B * heads * D * Jp, dev)
    W = 2 * heads * D
    kw = dict(k_src=src.to(dev), v_src=None, k_scale=ks.to(dev), khat=khat.t, vt=vt.t, B=B, heads=heads, rows=J, r0=r0, src_strides=(J * W, W, D),
              k_strides=(heads * Jp * D, Jp * D, D), vt_strides=(heads * D * Jp, D * Jp, Jp), k_off=0, v_off=heads * D, head_dim=D)
    kw["v_src"] = kw["k_src"]

    def verify(tag):
        km = torch.zeros(B, heads, Jp, D, dtype=torch.bool)
        km[:, :, r0:r0 + J] = True
        khat.check(km)                                                            # rows below r0 and the r0 + J .. Jp padding untouched
        vt.check(km.transpose(2, 3))
        k64 = src[..., :heads * D].double().view(B, J, heads, D).permute(0, 2, 1, 3)
        v = src[..., heads * D:].view(B, J, heads, D).permute(0, 2, 1, 3)
        ref = _l2norm64(k64) * ks.double()
        got_k = khat.cpu().view(B, heads, Jp, D)[:, :, r0:r0 + J]
        check16("kv_prep", got_k, ref, K_NORM * U * ref.abs(), tag)
        assert got_k[B - 1, 0, J - 1].abs().sum() == 0
        got_v = vt.cpu().view(B, heads, D, Jp)[:, :, :, r0:r0 + J]
        assert torch.equal(got_v, v.to(torch.float16).transpose(2, 3)), (tag, "V^T is a transposed copy (fp32 sources: rounded to nearest)")

    return kw, verify


@pytest.mark.parametrize("r0", [0, 3])
@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("dt", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_kv_prep(ops, dev, dt, D, r0):
    """K-hat = l2norm(k) * k_scale and V^T against fp64 for fp16 and fp32 sources, J = 37 keys (no multiple of the 32 | 64 rows of a block) at
    key offset r0 of Jp = 48, k / v columns inside a fused kv row, 3 heads, B = 2."""
    kw, verify = _kv_job(ops, dev, 2, 3, 37, 48, D, dt, r0, 6000 + D + r0)
    plan = ops.Plan()
    ops.kv_prep(plan, kw.pop("k_src"), kw.pop("v_src"), kw.pop("k_scale"), kw.pop("khat"), kw.pop("vt"), **kw)
    _run(plan)
    verify((str(dt), D, r0))


def test_kv_prep_multi(ops, dev):
    """Jobs of different B * heads, rows, source types and head dims in one launch: each against fp64, and the blocks beyond a job's own extent
    (the grid is the maximum over the jobs) write nothing."""
    specs = [(2, 1, 2, 16, 64, torch.float16, 3), (3, 8, 37, 48, 64, torch.float16, 0), (1, 4, 5, 8, 32, torch.float32, 3), (2, 2, 33, 40, 32, torch.float16, 3)]
    plan, jobs, checks = ops.Plan(), [], []
    for i, (B, heads, J, Jp, D, dt, r0) in enumerate(specs):
        kw, verify = _kv_job(ops, dev, B, heads, J, Jp, D, dt, r0, 6100 + i)
        ops.kv_prep(plan, kw.pop("k_src"), kw.pop("v_src"), kw.pop("k_scale"), kw.pop("khat"), kw.pop("vt"), batch=jobs, **kw)
        checks.append(verify)
    ops.kv_prep_multi(plan, jobs, dev)
    assert len(plan) == 1
    _run(plan)
    for i, verify in enumerate(checks):
        verify(("multi", i))


# ------------------------------------------------------------------------------------------------ SELECT_ROWS / MEAN_ROWS / MEMSET32 / ROWS_COPY

@pytest.mark.parametrize("C", [8, 512, 768])
@pytest.mark.parametrize("L", [1, 37, 256])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_select_rows(ops, dev, masked, L, C):
    """R = 6 output rows drawn from 3 sources with repeats (the CFG rows), keep mixed, mask with ragged true-prefixes and one all-false
    source: dst[r, l] = keep[r] & mask[src[r], l] ? a[src[r], l] : nul[l], bit for bit."""
    torch.manual_seed(7000 + L + C)
    R, S = 6, 3
    a, nul = h16(torch.randn(S, L, C)), h16(torch.randn(L, C))
    src = torch.tensor([0, 2, 1, 0, 2, 1], dtype=torch.int32)
    keep = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.uint8)
    lens = [L, (L + 1) // 3, 0]
    mask = torch.stack([torch.arange(L) < n for n in lens]).to(torch.uint8) if masked else None
    dst = guarded(R * L * C, dev)
    plan = ops.Plan()
    ops.select_rows(plan, a.to(dev), nul.to(dev), mask.to(dev) if masked else None, src.to(dev), keep.to(dev), dst.t, R=R, L=L, C=C)
    _run(plan)
    dst.check()
    take = keep.bool().view(R, 1) & (mask.bool()[src.long()] if masked else torch.ones(R, L, dtype=torch.bool))
    want = torch.where(take.unsqueeze(-1), a[src.long()], nul.unsqueeze(0).expand(R, L, C))
    assert torch.equal(dst.cpu().view(R, L, C), want)
    assert bool(take.any()) and not bool(take.all())
    note("select_rows", mismatches=0.0)


@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("rows", [1, 2, 37, 256])
def test_mean_rows(ops, dev, rows, C):
    """out[b] = fp16(mean over the rows of x[b]), B = 3, ld_x > C, bs_x > rows * ld_x, ld_out > C.  A thread adds the rows one after the other
    (rows roundings), 1 / rows and the product round once each: k = rows + 2 relative to sum|x| / rows."""
    torch.manual_seed(8000 + rows + C)
    B = 3
    x = h16(torch.randn(B, rows, C) + 0.5)
    ax = strided16(ops, x, C + 8, rows * (C + 8) + 16, dev, lead=8)
    ld_o = C + 16
    out = guarded(B * ld_o, dev)
    plan = ops.Plan()
    ops.mean_rows(plan, ax, out.act(ops, 1, B, C, ld_o))
    _run(plan)
    out.check(rows_mask(out.numel, 1, B, C, ld_o, B * ld_o))
    got = rows_read(out.cpu(), 1, B, C, ld_o, B * ld_o)[0]
    check16("mean_rows", got, x.double().mean(1), (rows + 2) * U * x.double().abs().sum(1) / rows, (rows, C))


@pytest.mark.parametrize("value", [0, 0x3C003C00])
@pytest.mark.parametrize("count", [1, 255, 256, 257, 70001])
def test_memset32(ops, dev, count, value):
    """count words of a longer buffer (count < numel): the tail and both guards untouched."""
    buf = guarded(count + 37, dev, torch.int32)
    plan = ops.Plan()
    ops.memset32(plan, buf.t, value, count=count)
    _run(plan)
    buf.check(torch.arange(count + 37) < count)
    assert bool((buf.cpu()[:count] == value).all())
    note("memset32", mismatches=0.0)


ROWS_COPY_CASES = {
    # name: (B, rows, C, (src shape B | 1, rows | 1, width), src_bs, src_rs, src_off, (dst rows, dst width), dst_bs, dst_rs, dst_off)
    "batch_broadcast": (3, 5, 64, (1, 5, 64), 0, 64, 0, (9, 64), 9 * 64, 64, 2 * 64),
    "row_broadcast": (2, 6, 32, (2, 1, 32), 32, 0, 0, (6, 32), 6 * 32, 32, 0),
    "one_row_98304": (2, 1, 98304, (1, 1, 98304), 0, 0, 0, (1, 98304), 98304, 0, 0),
    "slice_dst": (2, 7, 24, (2, 7, 24), 7 * 24, 24, 0, (7, 64), 7 * 64, 64, 16),
    "slice_src": (2, 7, 24, (2, 7, 80), 7 * 80, 80, 40, (7, 24), 7 * 24, 24, 0),
    "c8": (3, 11, 8, (3, 11, 8), 11 * 8, 8, 0, (11, 16), 11 * 16, 16, 8),
}


@pytest.mark.parametrize("case", list(ROWS_COPY_CASES))
def test_rows_copy(ops, dev, case):
    """dst[b, r, :C] = src[b | 0, r | 0, :C] bit for bit: broadcast over the batch (src_bs = 0) and over the rows (src_rs = 0), the
    rows = 1 / C = 98304 form of the video engine, channel slices as destination (dst_rs > C, dst_off inside a row) and as source, C = 8."""
    B, rows, C, sshape, src_bs, src_rs, src_off, (drows, dwidth), dst_bs, dst_rs, dst_off = ROWS_COPY_CASES[case]
    torch.manual_seed(9000 + C)
    src = h16(torch.randn(*sshape))
    dst = guarded(B * drows * dwidth, dev)
    plan = ops.Plan()
    ops.rows_copy(plan, src.to(dev), dst.t, B=B, rows=rows, C=C, src_bs=src_bs, src_rs=src_rs, dst_bs=dst_bs, dst_rs=dst_rs, src_off=src_off, dst_off=dst_off)
    _run(plan)
    dst.check(rows_mask(dst.numel, B, rows, C, dst_rs, dst_bs, dst_off))
    want = src.reshape(-1).as_strided((B, rows, C), (src_bs, src_rs, 1), src_off)
    assert torch.equal(rows_read(dst.cpu(), B, rows, C, dst_rs, dst_bs, dst_off), want)
    note("rows_copy", mismatches=0.0)


def test_rows_copy_inside_one_tensor(ops, dev):
    """The engine's copy of the conditional half of a token buffer to its null half: source and destination are disjoint regions of ONE tensor."""
    torch.manual_seed(9100)
    B, rows, C, ld = 2, 5, 40, 48
    buf = guarded(2 * B * rows * ld, dev)
    vals = h16(torch.randn(B, rows, C))
    flat = buf.cpu().clone()
    flat.as_strided((B, rows, C), (rows * ld, ld, 1), 0).copy_(vals)
    buf.t.copy_(flat.to(dev))
    plan = ops.Plan()
    ops.rows_copy(plan, buf.t, buf.t, B=B, rows=rows, C=C, src_bs=rows * ld, src_rs=ld, dst_bs=rows * ld, dst_rs=ld, dst_off=B * rows * ld + 8)
    _run(plan)
    buf.check(rows_mask(buf.numel, B, rows, C, ld, rows * ld) | rows_mask(buf.numel, B, rows, C, ld, rows * ld, B * rows * ld + 8))
    assert torch.equal(rows_read(buf.cpu(), B, rows, C, ld, rows * ld, B * rows * ld + 8), vals)
    assert torch.equal(rows_read(buf.cpu(), B, rows, C, ld, rows * ld), vals)


# ------------------------------------------------------------------------------------------------ PACK_IMAGE

@pytest.mark.parametrize("H,W", [(5, 7), (24, 40)])
@pytest.mark.parametrize("brep", [1, 2])
@pytest.mark.parametrize("Ca,Cb,Cpad", [(3, 0, 8), (3, 3, 8), (3, 5, 8), (3, 6, 16)])
def test_pack_image(ops, dev, Ca, Cb, Cpad, brep, H, W):
    """fp32 NCHW x (+ lowres image) -> fp16 NHWC [B * brep, H, W, Cpad]: channel placement, zero padding, the brep copies.  A conversion
    fp32 -> fp16 rounds to nearest, so the values are bit-exact too (d = 0).  H * W = 35 | 960: B * brep * H * W is no multiple of 256."""
    torch.manual_seed(10000 + Cb + H)
    B = 3
    a = torch.randn(B, Ca, H, W) * 1.3
    b = torch.randn(B, Cb, H, W) if Cb else None
    out = guarded(B * brep * H * W * Cpad, dev)
    act = out.act(ops, B * brep, H * W, Cpad)
    act.H, act.W = H, W
    plan = ops.Plan()
    ops.pack_image(plan, a.to(dev), b.to(dev) if Cb else None, act, brep=brep)
    _run(plan)
    out.check()
    want = torch.zeros(B, H, W, Cpad, dtype=torch.float16)
    want[..., :Ca] = a.permute(0, 2, 3, 1).to(torch.float16)
    if Cb:
        want[..., Ca:Ca + Cb] = b.permute(0, 2, 3, 1).to(torch.float16)
    got = out.cpu().view(brep, B, H, W, Cpad)
    for k in range(brep):
        assert torch.equal(got[k], want), k
    note("pack_image", mismatches=0.0)


# ------------------------------------------------------------------------------------------------ TIME_EMBED / SCALE_SHIFT

TIMES = (0.0, 1e-4, 0.5, 0.999, 1.0)


@pytest.mark.parametrize("table", [False, True], ids=["direct", "table"])
@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("out_dim", [128, 300, 2048])
def test_time_embed(ops, dev, out_dim, B, table):
    """hid[b] = fp16(silu(bias + w0 x + sum_k ws_k sin(2 pi x f_k) + wc_k cos(2 pi x f_k))), half_dim 8, hidden rows ld = out_dim + 8 apart,
    x from times[b] or from row *step_ptr of the coefficient table, at x in {0, 1e-4, 0.5, 0.999, 1}.
    Error of the pre-activation a: the phase x f 2 pi carries three roundings (3 u |phase| absolute on the sine's argument), sinf / cosf 2 ulp32
    (4 u), each product one rounding and the chain of 2 half_dim + 1 additions u each relative to the sum of |terms|.  SiLU's slope is below 1.1."""
    torch.manual_seed(11000 + out_dim)
    half = 8
    freqs = torch.randn(half)
    w, bias = torch.randn(out_dim, 2 * half + 1) / 4, torch.randn(out_dim) * 0.1
    ld = out_dim + 8
    fd, wd, bd = freqs.to(dev), w.to(dev), bias.to(dev)
    runs = []
    if table:
        coef = torch.randn(len(TIMES), 8)
        coef[:, 6] = torch.tensor(TIMES)
        runs = [(torch.full((B,), t), dict(times=None, coef=coef.to(dev), step_ptr=torch.tensor([i], dtype=torch.int32, device=dev))) for i, t in enumerate(TIMES)]
    elif B == 1:
        runs = [(torch.tensor([t]), None) for t in TIMES]
    else:
        runs = [(torch.tensor([TIMES[i % len(TIMES)] for i in range(B)]), None)]
    for times, kw in runs:
        kw = kw or dict(times=times.to(dev), coef=None, step_ptr=None)
        hid = guarded(B * ld, dev)
        plan = ops.Plan()
        ops.time_embed(plan, freqs=fd, w=wd, bias=bd, hid=hid.act(ops, 1, B, out_dim, ld), **kw)
        _run(plan)
        hid.check(rows_mask(hid.numel, 1, B, out_dim, ld, B * ld))
        x = times.double().view(B, 1)
        ph = x * freqs.double().view(1, half) * float(torch.tensor(2 * math.pi, dtype=torch.float32))
        w64 = w.double()
        t_lin = x * w64[:, 0].view(1, out_dim)                                                         # [B, out]
        t_sin = ph.sin().unsqueeze(1) * w64[:, 1:1 + half].unsqueeze(0)                                # [B, out, half]
        t_cos = ph.cos().unsqueeze(1) * w64[:, 1 + half:].unsqueeze(0)
        a = bias.double() + t_lin + t_sin.sum(-1) + t_cos.sum(-1)
        mag = bias.double().abs() + t_lin.abs() + t_sin.abs().sum(-1) + t_cos.abs().sum(-1)
        trig = ((3 * U * ph.abs() + 4 * U).unsqueeze(1) * (w64[:, 1:1 + half].abs() + w64[:, 1 + half:].abs()).unsqueeze(0)).sum(-1)
        da = (2 * half + 2 + 1) * U * mag + trig
        got = rows_read(hid.cpu(), 1, B, out_dim, ld, B * ld)[0]
        check16("time_embed", got, silu64(a), 1.1 * da + silu_d(a), (out_dim, B, table, times[0].item()))


@pytest.mark.parametrize("f32", [False, True], ids=["f16rows", "f32rows"])
def test_scale_shift(ops, dev, f32):
    """pa[b, i] = gamma_s[i] (ss[b, idx_scale[i]] + 1), ps[b, i] = ss[b, idx_shift[i]] with index vectors that interleave, repeat and run
    backwards; fp16 rows with ld > width (the columns beside the rows NaN).  ps is a copy; pa rounds the addition and the product (k = 2)."""
    torch.manual_seed(12000)
    B, width, n = 5, 96, 85
    ss = torch.randn(B, width)
    ss = ss if f32 else h16(ss)
    idx_scale = torch.cat((torch.arange(0, width, 2), torch.arange(width - 1, -1, -3), torch.tensor([7, 7, 7, 0, 95])))[:n].int()
    idx_shift = torch.cat((torch.arange(1, width, 2), torch.tensor([95, 0, 0, 41, 41]), torch.arange(width - 2, -1, -3)))[:n].int()
    assert idx_scale.numel() == n and idx_shift.numel() == n
    gam = torch.randn(n)
    pa, ps = guarded(B * n, dev, torch.float32), guarded(B * n, dev, torch.float32)
    src = ss.to(dev) if f32 else strided16(ops, ss.view(1, B, width), width + 24, B * (width + 24), dev, lead=8)
    plan = ops.Plan()
    ops.scale_shift(plan, src, gam.to(dev), idx_scale.to(dev), idx_shift.to(dev), pa.t, ps.t)
    _run(plan)
    pa.check()
    ps.check()
    sc, sh = ss.double()[:, idx_scale.long()], ss.float()[:, idx_shift.long()]
    assert torch.equal(ps.cpu().view(B, n), sh)
    ref = gam.double() * (sc + 1)
    err = (pa.cpu().view(B, n).double() - ref).abs()
    assert bool((err <= 2 * U * gam.double().abs() * (sc.abs() + 1)).all())
    note("scale_shift", pa_worst_row_err=row_err(pa.cpu().view(B, n), ref)[0])


# ------------------------------------------------------------------------------------------------ ACT_PREP

def _act64(v, d_lin, act):
    """(reference, bound) of act(v) for a pre-activation v known to d_lin: SiLU's slope is below 1.1, GELU's below 1.13."""
    if act == "silu":
        return silu64(v), 1.1 * d_lin + silu_d(v)
    if act == "gelu":
        return gelu64(v), 1.13 * d_lin + gelu_d(v)
    return v, d_lin


ACTS = {"none": 0, "silu": 1, "gelu": 2}


@pytest.mark.parametrize("act", ["none", "silu", "gelu"])
@pytest.mark.parametrize("affine", ["none", "pa", "pa+ps_batch", "ps"])
@pytest.mark.parametrize("stat", ["rs+mu", "rs", "ssq", "none"])
def test_act_prep(ops, dev, stat, affine, act):
    """y = fp16(act((concat(x1, x2) - mu) * rs * pa + ps)) on a two-tensor input of 40 + 24 channels (the boundary on no 16- or 32-channel
    line), B = 2 images of 11 pixels, x1 / x2 / y channel slices of wider rows; rs from rs, from ssq_a + ssq_wb * ssq_b, or 1; pa per channel
    (pstride = 0) or pa + ps per batch element.  Rounding: the subtraction, two products and the addition (k = 4 relative to
    |(x - mu) rs pa| + |ps|); the ssq form adds a product, an addition and v_rsq's 1 ulp32 on half the argument's error (k + 3)."""
    torch.manual_seed(13000)
    B, R, C1, C2 = 2, 11, 40, 24
    C = C1 + C2
    x1, x2 = h16(torch.randn(B, R, C1) * 1.5 + 0.3), h16(torch.randn(B, R, C2) * 0.7)
    x1[0, 3], x2[0, 3] = 0.0, 0.0                                                   # an all-zero pixel: with ssq_a = ssq_b = 0 the 1e-24 clamp, y = act(ps)
    a1 = strided16(ops, x1, C1 + 8, R * (C1 + 8) + 16, dev, lead=8)
    a2 = strided16(ops, x2, C2 + 16, R * (C2 + 16) + 8, dev)
    ld_y = C + 8
    y = guarded(B * R * ld_y + 16, dev)
    kw, k = {}, 4
    x = torch.cat((x1, x2), -1).double().reshape(B * R, C)
    mu64, sc64 = torch.zeros(B * R, dtype=torch.float64), torch.ones(B * R, dtype=torch.float64)
    if stat in ("rs+mu", "rs"):
        rs = torch.rand(B * R) + 0.5
        kw["rs"], sc64 = rs.to(dev), rs.double()
        if stat == "rs+mu":
            mu = torch.randn(B * R) * 0.3
            kw["mu"], mu64 = mu.to(dev), mu.double()
    elif stat == "ssq":
        qa, qb, wb = torch.rand(B * R) * 50 + 1, torch.rand(B * R) * 20, 0.25
        qa[3], qb[3] = 0.0, 0.0
        kw.update(ssq_a=qa.to(dev), ssq_b=qb.to(dev), ssq_wb=wb)
        sc64, k = torch.rsqrt((qa.double() + wb * qb.double()).clamp(min=float(torch.tensor(1e-24)))), k + 3
    per_batch = affine == "pa+ps_batch"
    pa64 = torch.ones(B, C, dtype=torch.float64)
    ps64 = torch.zeros(B, C, dtype=torch.float64)
    if "pa" in affine:
        pa = torch.randn(B if per_batch else 1, C) * 0.5 + 1
        kw["pa"], pa64 = pa.to(dev), pa.double().expand(B, C)
    if "ps" in affine:
        ps = torch.randn(B if (per_batch or affine == "ps") else 1, C) * 0.4
        kw["ps"], ps64 = ps.to(dev), ps.double().expand(B, C)
    kw["pstride"] = C if (per_batch or affine == "ps") else 0
    plan = ops.Plan()
    ops.act_prep(plan, a1, y.act(ops, B, R, C, ld_y, R * ld_y + 16, lead=8), x2=a2, act_in=ACTS[act], **kw)
    _run(plan)
    y.check(rows_mask(y.numel, B, R, C, ld_y, R * ld_y + 16, 8))
    prod = (x - mu64.view(-1, 1)) * sc64.view(-1, 1) * pa64.repeat_interleave(R, 0)
    sh = ps64.repeat_interleave(R, 0)
    ref, d = _act64(prod + sh, k * U * (prod.abs() + sh.abs()), act)
    got = rows_read(y.cpu(), B, R, C, ld_y, R * ld_y + 16, 8).reshape(B * R, C).double()
    check16("act_prep", got, ref, d, (stat, affine, act))


def test_act_prep_above_the_grid_cap(ops, dev):
    """2 x 192 x 192 pixels of 256 channels = 2 359 296 eight-channel groups: above the launcher's 2048 blocks x 256 threads x 4 items, so the
    grid-stride loop runs a second, ragged pass.  ChanRMSNorm statistics (ssq_a) -> pa -> SiLU, every element checked.  Hardware only."""
    if EMULATED:
        pytest.skip("604 M fp16 values through the CPU emulation take minutes; runs on hardware")
    torch.manual_seed(13500)
    B, HW, C = 2, 192 * 192, 256
    x = h16(torch.randn(B, HW, C))
    qa = (x.float() ** 2).sum(-1).reshape(-1)
    pa = torch.randn(1, C) * 0.5 + 4
    y = guarded(B * HW * C, dev)
    plan = ops.Plan()
    ops.act_prep(plan, ops.Act(x.to(dev), B, 1, HW, C, C, HW * C), y.act(ops, B, HW, C), ssq_a=qa.to(dev), pa=pa.to(dev), pstride=0, act_in=1)
    _run(plan)
    y.check()
    got = y.cpu().view(B * HW, C)
    worst = 0.0
    for r0 in range(0, B * HW, 8192):                                               # fp64 in slabs
        xs = x.reshape(B * HW, C)[r0:r0 + 8192].double()
        prod = xs * torch.rsqrt(qa[r0:r0 + 8192].double().clamp(min=1e-24)).view(-1, 1) * pa.double()
        ref, d = _act64(prod, 7 * U * prod.abs(), "silu")
        g = got[r0:r0 + 8192].double()
        over = (g - ref).abs() - (ulp16(ref) + d)
        assert float(over.max()) <= 0, (r0 + int(over.argmax()) // C, float(over.max()))
        worst = max(worst, row_err(g, ref)[0])
    note("act_prep", above_cap_worst_row_err=worst)


def _split(C, second):
    if C == 64:
        return (40, 24) if second else (64, 0)
    return (C - 24, 24) if (second and C > 24) else (C, 0)


@pytest.mark.parametrize("pa_form", ["channel", "batch"])
@pytest.mark.parametrize("second", [False, True], ids=["x1", "x2+ssq_b"])
@pytest.mark.parametrize("C", [8, 64, 128, 136, 256, 264, 512])
def test_act_prep_self_stat(ops, dev, C, second, pa_form):
    """self_stat: the launch reduces sum x1^2 over the lanes of a pixel itself (16 / 32 / 64 lanes; 8 .. 512 channels: exactly 16 / 32 / 64
    groups, one group more than each, fewer groups than lanes) and scales by rsqrt(that + ssq_wb * ssq_b).  B = 3 images of 7 pixels: 21 rows =
    16 + 5, dead rows in the last block for every lane count.  With x2 (24 channels, the boundary inside a 16-lane team) x2's squares must
    stay out of the sum.  Rounding: 7 + log2(lanes) additions of exact squares, the ssq_b product and addition, v_rsq (half of that, + 1 ulp32),
    then two products and the addition of ps."""
    torch.manual_seed(14000 + C)
    B, R = 3, 7
    C1, C2 = _split(C, second)
    x1 = h16(torch.randn(B, R, C1) * 1.3)
    x1[1, 2] = 0.0
    x2 = h16(torch.randn(B, R, C2) * 3.0) if C2 else None
    a1 = strided16(ops, x1, C1 + 8, R * (C1 + 8) + 16, dev, lead=8)
    a2 = strided16(ops, x2, C2 + 16, R * (C2 + 16), dev) if C2 else None
    qb, wb = (torch.rand(B * R) * 9 + 0.5, 0.25) if second else (None, 1.0)
    nb = B if pa_form == "batch" else 1
    pa, ps = torch.randn(nb, C) * 0.5 + 2, torch.randn(nb, C) * 0.3
    ld_y = C + 8
    y = guarded(B * R * ld_y, dev)
    plan = ops.Plan()
    ops.act_prep(plan, a1, y.act(ops, B, R, C, ld_y), x2=a2, pa=pa.to(dev), ps=ps.to(dev), pstride=C if pa_form == "batch" else 0, act_in=1,
                 ssq_b=qb.to(dev) if second else None, ssq_wb=wb, self_stat=True)
    _run(plan)
    y.check(rows_mask(y.numel, B, R, C, ld_y, R * ld_y))
    x = (torch.cat((x1, x2), -1) if C2 else x1).double().reshape(B * R, C)
    tot = (x1.double() ** 2).sum(-1).reshape(-1) + (wb * qb.double() if second else 0.0)
    sc = torch.rsqrt(tot.clamp(min=float(torch.tensor(1e-24))))
    L = 16 if C <= 128 else 32 if C <= 256 else 64
    k = 0.5 * (7 + math.log2(L) + 2) + 2 + 3
    prod = x * sc.view(-1, 1) * pa.double().expand(B, C).repeat_interleave(R, 0)
    sh = ps.double().expand(B, C).repeat_interleave(R, 0)
    ref, d = _act64(prod + sh, k * U * (prod.abs() + sh.abs()), "silu")
    got = rows_read(y.cpu(), B, R, C, ld_y, R * ld_y).reshape(B * R, C)
    check16("act_prep_self_stat", got, ref, d, (C, second, pa_form))


# ------------------------------------------------------------------------------------------------ STEP_SLICE

@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_step_slice(ops, dev, dt):
    """Four segments of 5, 300, 17 and 1030 sixteen-byte words (the boundaries fall inside a 256-thread block), the counter at the first, a
    middle and the last step and clamped from above and from below: row for row bit-exact, nothing written beside any destination."""
    torch.manual_seed(15000)
    T, words = 4, (5, 300, 17, 1030)
    per = 16 // torch.empty(0, dtype=dt).element_size()
    tabs = [torch.randn(T, w * per).to(dt) for w in words]
    dsts = [guarded(w * per, dev, dt) for w in words]
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    plan = ops.Plan()
    p = ops.step_slice(plan, [(t.to(dev), d.t) for t, d in zip(tabs, dsts)], step)
    assert p.steps == T
    for s, row in ((0, 0), (2, 2), (T - 1, T - 1), (T + 5, T - 1), (-3, 0)):
        step.fill_(s)
        _run(plan)
        for t, d in zip(tabs, dsts):
            d.check()
            assert torch.equal(d.cpu(), t[row]), (s, row)
    note("step_slice", mismatches=0.0)


def test_step_slice_above_the_grid_cap(ops, dev):
    """Two segments of 300 000 + 224 301 words: more than the 2048 x 256 threads of the capped grid, so the kernel loops and the segment
    boundary falls inside the second pass; 8.4 MB per step, 3 steps."""
    torch.manual_seed(15100)
    T, words = 3, (300000, 224301)
    assert sum(words) > 2048 * 256
    tabs = [torch.randn(T, w * 4) for w in words]
    dsts = [guarded(w * 4, dev, torch.float32) for w in words]
    step = torch.tensor([1], dtype=torch.int32, device=dev)
    plan = ops.Plan()
    ops.step_slice(plan, [(t.to(dev), d.t) for t, d in zip(tabs, dsts)], step)
    for s in (1, 2):
        step.fill_(s)
        _run(plan)
        for t, d in zip(tabs, dsts):
            d.check()
            assert torch.equal(d.cpu(), t[s]), s


# ------------------------------------------------------------------------------------------------ launcher refusals (host side: nothing is launched)

def _poked(build, **fields):
    """The op `build` appends (a valid one), with params fields overwritten afterwards."""
    def f(plan):
        p = build(plan)
        for k, v in fields.items():
            setattr(p, k, v)
        return p
    return f


def _refusals(ops, dev):
    """name -> (a builder that appends ONE op whose launcher must refuse it, a fragment of the message of the check that must fire).  Every
    tensor is a valid allocation large enough for the aligned form of the same call; IMAGEN_CHECK returns before the launch."""
    f16 = lambda *s: torch.zeros(*s, dtype=torch.float16, device=dev)
    f32 = lambda *s: torch.zeros(*s, device=dev)
    A = lambda t, B, R, C, ld, bs, off=0: ops.Act(t, B, 1, R, C, ld, bs, off)
    big = f16(4096)
    i32 = torch.zeros(8, dtype=torch.int32, device=dev)
    u8 = torch.ones(64, dtype=torch.uint8, device=dev)
    kvk = dict(B=1, heads=1, rows=2, r0=0, src_strides=(256, 128, 64), k_strides=(1024, 1024, 64), vt_strides=(1024, 1024, 16))
    ok = A(big, 1, 2, 16, 16, 32)
    rowstat = lambda p: ops.rowstat(p, ok, mode=0, rs=f32(8))
    gate = lambda p: ops.gate_residual(p, ok, None, ok, ok)
    ln = lambda p: ops.ln_residual(p, ok, f32(16), ok)
    qn = lambda p: ops.qnorm(p, big, f32(64), rows=2, heads=1, ld=64, mult=1.0)
    kv = lambda p: ops.kv_prep(p, big, big, f32(64), big, big, **kvk)
    mean = lambda p: ops.mean_rows(p, A(big, 2, 2, 16, 16, 32), A(big, 1, 2, 16, 16, 32))
    sel = lambda p: ops.select_rows(p, big, big, None, i32, u8, big, R=2, L=2, C=16)
    cp = lambda p: ops.rows_copy(p, big, big, B=1, rows=2, C=16, src_bs=0, src_rs=16, dst_bs=0, dst_rs=16, dst_off=2048)
    pack = lambda p: ops.pack_image(p, torch.zeros(1, 3, 1, 1, device=dev), None, ops.new_act(1, 1, 1, 8, dev), brep=1)
    te = lambda p: ops.time_embed(p, times=f32(2), coef=None, step_ptr=None, freqs=f32(4), w=f32(16, 9), bias=f32(16), hid=A(big, 1, 2, 16, 16, 32))
    ss = lambda p: ops.scale_shift(p, A(big, 1, 2, 16, 16, 32), f32(8), i32, i32, f32(16), f32(16))
    ms = lambda p: ops.memset32(p, i32, 0, count=8)
    return {
        "rowstat_ld2": (lambda p: ops.rowstat(p, ok, mode=0, rs=f32(8), x2=A(big, 1, 2, 16, 20, 40)), "rowstat: strides must be multiples of 8"),
        "rowstat_bs1": (lambda p: ops.rowstat(p, A(big, 2, 2, 16, 16, 36), mode=0, rs=f32(8)), "rowstat: strides must be multiples of 8"),
        "rowstat_x2_offset": (lambda p: ops.rowstat(p, ok, mode=2, rs=f32(8), x2=A(big, 1, 2, 16, 16, 32, off=4)), "rowstat: strides must be multiples of 8"),
        "rowstat_empty": (_poked(rowstat, rows=0), "rowstat: empty"),
        "rowstat_mode1_without_mu": (_poked(rowstat, mode=1), "rowstat: null x1 / rs"),
        "rowstat_mode": (_poked(rowstat, mode=3), "rowstat: null x1 / rs"),
        "rowstat_null_rs": (_poked(rowstat, rs=None), "rowstat: null x1 / rs"),
        "gate_residual_ld": (lambda p: ops.gate_residual(p, A(big, 1, 2, 16, 20, 40), None, ok, ok), "gate_residual: row strides must be multiples of 8"),
        "gate_residual_null": (_poked(gate, res=None), "gate_residual: null tensors"),
        "gate_residual_empty": (_poked(gate, rows=0), "gate_residual: null tensors"),
        "ln_residual_ld_y": (lambda p: ops.ln_residual(p, A(big, 1, 2, 16, 20, 40), f32(16), ok), "ln_residual: strides must be multiples of 8"),
        "ln_residual_bs_out": (lambda p: ops.ln_residual(p, A(big, 2, 2, 16, 16, 32), f32(16), A(big, 2, 2, 16, 16, 36)), "ln_residual: strides must be multiples of 8"),
        "ln_residual_ld_res": (lambda p: ops.ln_residual(p, ok, f32(16), ok, res=A(big, 1, 2, 16, 12, 24)), "ln_residual: strides must be multiples of 8"),
        "ln_residual_mu_without_rs": (_poked(ln, mu_out=f32(8).data_ptr()), "mu_out and rs_out come together"),
        "ln_residual_null_g": (_poked(ln, g=None), "ln_residual: null tensors"),
        "qnorm_ld": (lambda p: ops.qnorm(p, big, f32(64), rows=2, heads=1, ld=68, mult=1.0), "qnorm: row stride 68"),
        "qnorm_ld_below_heads": (lambda p: ops.qnorm(p, big, f32(64), rows=2, heads=2, ld=64, mult=1.0), "covering the 2 heads"),
        "qnorm_head_dim": (_poked(qn, head_dim=48), "qnorm: head_dim 48"),
        "qnorm_null_scale": (_poked(qn, q_scale=None), "qnorm: null tensors"),
        "qnorm_int": (_poked(qn, rows=1 << 16, heads=1 << 15, ld=1 << 21), "qnorm: rows * heads does not fit"),
        "kv_prep_k_rs": (lambda p: ops.kv_prep(p, big, big, f32(64), big, big, **dict(kvk, k_strides=(1024, 1024, 68))), "kv_prep: K-hat strides"),
        "kv_prep_src_rs": (lambda p: ops.kv_prep(p, big, big, f32(64), big, big, **dict(kvk, src_strides=(256, 132, 64))), "kv_prep: fp16 source strides"),
        "kv_prep_v_off": (lambda p: ops.kv_prep(p, big, big, f32(64), big, big, v_off=4, **kvk), "kv_prep: fp16 source strides"),
        "kv_prep_head_dim": (_poked(kv, head_dim=16), "kv_prep: head_dim 16"),
        "kv_prep_grid": (_poked(kv, B=4096, heads=16), "exceeds the grid"),
        "kv_prep_empty": (_poked(kv, rows=0), "kv_prep: empty"),
        "kv_prep_negative_r0": (_poked(kv, r0=-1), "kv_prep: empty"),
        "kv_prep_null_vt": (_poked(kv, vt=None), "kv_prep: null pointer"),
        "mean_rows_ld_x": (lambda p: ops.mean_rows(p, A(big, 1, 2, 16, 20, 40), A(big, 1, 1, 16, 16, 16)), "mean_rows: strides must be multiples of 8"),
        "mean_rows_ld_out": (lambda p: ops.mean_rows(p, A(big, 2, 2, 16, 16, 32), A(big, 1, 2, 16, 20, 40)), "mean_rows: strides must be multiples of 8"),
        "mean_rows_empty": (_poked(mean, rows=0), "mean_rows: bad shape"),
        "mean_rows_null_out": (_poked(mean, out=None), "mean_rows: null tensors"),
        "select_rows_dst_offset": (lambda p: ops.select_rows(p, big, big, None, i32, u8, big[4:], R=2, L=2, C=16), "select_rows: rows must be 16-byte aligned"),
        "select_rows_int": (lambda p: ops.select_rows(p, big, big, None, i32, u8, big, R=1 << 15, L=1 << 15, C=64), "select_rows: R * L * C / 8 does not fit"),
        "select_rows_null_keep": (_poked(sel, keep=None), "select_rows: null tensors"),
        "rows_copy_src_rs": (lambda p: ops.rows_copy(p, big, big, B=1, rows=2, C=16, src_bs=0, src_rs=20, dst_bs=0, dst_rs=16, dst_off=2048), "rows_copy: strides and offsets"),
        "rows_copy_dst_off": (lambda p: ops.rows_copy(p, big, big, B=1, rows=2, C=16, src_bs=0, src_rs=16, dst_bs=0, dst_rs=16, dst_off=2052), "rows_copy: strides and offsets"),
        "rows_copy_int": (lambda p: ops.rows_copy(p, big, big, B=1 << 16, rows=1 << 16, C=8, src_bs=0, src_rs=0, dst_bs=0, dst_rs=0), "rows_copy: B * rows * C / 8 does not fit"),
        "rows_copy_empty": (_poked(cp, rows=0), "rows_copy: null tensors"),
        "pack_image_int": (_poked(pack, B=1 << 10, Brep=1 << 10, H=1 << 10, W=4), "pack_image: B * Brep * H * W does not fit"),
        "pack_image_channels": (_poked(pack, Ca=9), "pack_image: bad shape"),
        "pack_image_null_b": (_poked(pack, Cb=3), "pack_image: null pointer"),
        "time_embed_null_times": (_poked(te, times=None), "time_embed: null pointer"),
        "time_embed_step_without_coef": (_poked(te, step_ptr=i32.data_ptr()), "time_embed: null pointer"),
        "time_embed_ld_hid": (_poked(te, ld_hid=8), "time_embed: bad shape"),
        "time_embed_int": (_poked(te, B=1 << 16, out_dim=1 << 16, ld_hid=1 << 16), "time_embed: bad shape"),
        "scale_shift_null_idx": (_poked(ss, idx_shift=None), "scale_shift: null pointer"),
        "scale_shift_empty": (_poked(ss, total_c=0), "scale_shift: bad shape"),
        "scale_shift_int": (_poked(ss, B=1 << 16, total_c=1 << 16), "scale_shift: bad shape"),
        "memset32_int": (_poked(ms, count=(1 << 31) - 100), "memset32: null dst or a count"),
        "memset32_empty": (_poked(ms, count=0), "memset32: null dst or a count"),
        "memset32_null": (_poked(ms, dst=None), "memset32: null dst or a count"),
    }


REFUSALS = ["rowstat_ld2", "rowstat_bs1", "rowstat_x2_offset", "rowstat_empty", "rowstat_mode1_without_mu", "rowstat_mode", "rowstat_null_rs",
            "gate_residual_ld", "gate_residual_null", "gate_residual_empty", "ln_residual_ld_y", "ln_residual_bs_out", "ln_residual_ld_res",
            "ln_residual_mu_without_rs", "ln_residual_null_g", "qnorm_ld", "qnorm_ld_below_heads", "qnorm_head_dim", "qnorm_null_scale", "qnorm_int",
            "kv_prep_k_rs", "kv_prep_src_rs", "kv_prep_v_off", "kv_prep_head_dim", "kv_prep_grid", "kv_prep_empty", "kv_prep_negative_r0", "kv_prep_null_vt",
            "mean_rows_ld_x", "mean_rows_ld_out", "mean_rows_empty", "mean_rows_null_out", "select_rows_dst_offset", "select_rows_int",
            "select_rows_null_keep", "rows_copy_src_rs", "rows_copy_dst_off", "rows_copy_int", "rows_copy_empty", "pack_image_int", "pack_image_channels",
            "pack_image_null_b", "time_embed_null_times", "time_embed_step_without_coef", "time_embed_ld_hid", "time_embed_int", "scale_shift_null_idx",
            "scale_shift_empty", "scale_shift_int", "memset32_int", "memset32_empty", "memset32_null"]


@pytest.mark.parametrize("name", REFUSALS)
def test_launcher_refuses(ops, dev, name):
    """Strides / offsets that a 16-byte access cannot take, null pointers, empty problems, unsupported head dims and work-item counts that do
    not fit the kernels' int arithmetic are refused by the launcher's checks on the host: the call reports the error of THAT check and no
    kernel runs."""
    from imagen_pytorch_amd._abi import ImagenHipError

    table = _refusals(ops, dev)
    assert sorted(table) == sorted(REFUSALS)
    build, fragment = table[name]
    plan = ops.Plan()
    build(plan)
    assert len(plan) == 1
    with pytest.raises(ImagenHipError) as e:
        plan.run()
    assert fragment in str(e.value), str(e.value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", ["k_rs", "v_off", "head_dim", "empty"])
def test_kv_prep_multi_refuses_a_bad_job(ops, dev, bad):
    """The jobs of a multi launch reach the launcher in device memory, so ops.kv_prep_multi applies launch_kv_prep's checks to each job on the
    host while it still holds them: the plan is never built."""
    from imagen_pytorch_amd._abi import ImagenHipError

    big, ks = torch.zeros(4096, dtype=torch.float16, device=dev), torch.zeros(64, device=dev)
    kvk = dict(B=1, heads=1, rows=2, r0=0, src_strides=(256, 128, 64), k_strides=(1024, 1024, 64), vt_strides=(1024, 1024, 16))
    plan, jobs = ops.Plan(), []
    ops.kv_prep(plan, big, big, ks, big, big, batch=jobs, **kvk)
    p = ops.kv_prep(plan, big, big, ks, big, big, batch=jobs, v_off=4 if bad == "v_off" else 0, **dict(kvk, k_strides=(1024, 1024, 68 if bad == "k_rs" else 64)))
    if bad == "head_dim":
        p.head_dim = 48
    if bad == "empty":
        p.rows = 0
    with pytest.raises(ImagenHipError) as e:
        ops.kv_prep_multi(plan, jobs, dev)
    assert "kv_prep_multi: job 1" in str(e.value) and len(plan) == 0, str(e.value)
