"""MI355X (-m gpu; also on the CPU emulation, IMAGEN_EMUL_TESTS=1: tests/test_guide_cpu.py keeps the file in the CPU suite): GUIDE_X0 of
csrc/sampler.hip per element against its contract evaluated in fp64 (tests/plan_interp_guide.py), on sentinel-guarded buffers.

Shapes: B in {1, 3}; n in {48 (less than a workgroup), 1200 (ragged tail: no multiple of 256), 1203 (no multiple of 4: the scalar path),
12288 (two workgroups per sample), 524289 = 64 * 8192 + 1 (the smallest n that needs more than IMAGEN_GUIDE_MAX_BLOCKS workgroups of 8192:
the per-sample grid cap; also odd)}; the three objectives; cfg 1 and 2 (under 2 the immediate is a decoy); scales {0, 1, 3, 7.5, -1}.
The large n runs at one scale per (objective, cfg) — the paths it adds (the cap, the strided loop) do not depend on the scale.

Bar: TOL = 1e-6 normwise against fp64, the bar of CFG_X0 and LINCOMB (tests/test_sampler_kernels_gpu.py).  Inputs: x, pred standard normal,
alpha, sigma in [0.05, 0.95] as those tests draw them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import gpu_device, record_parity  # noqa: E402
from plan_interp_guidance import cfg_x0_contract  # noqa: E402
from plan_interp_guide import APG, RESCALE, guide_x0_contract  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
DECOY = 123.0
OBJECTIVES = ("noise", "x_start", "v")
SCALES = (0.0, 1.0, 3.0, 7.5, -1.0)
SMALL_N = (48, 1200, 1203, 12288)
CAP_N = 64 * 8192 + 1
SENTINEL = -77.25


def nerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o
    return o


class Case:
    """Inputs of one (B, n): drawn once, on the host and on the device; the outputs sit inside larger sentinel-filled buffers."""

    def __init__(self, B, n, seed, dev, steps=3):
        g = torch.Generator().manual_seed(seed)
        self.B, self.n, self.dev = B, n, dev
        self.x, self.pred = torch.randn(B, n, generator=g), torch.randn(2 * B, n, generator=g)
        self.coef = torch.rand(steps, 8, generator=g) * 0.9 + 0.05
        self.coef[:, 7] = torch.tensor([3.0, 7.5, -1.0])[:steps]
        self.xd, self.pd, self.cd = self.x.to(dev), self.pred.to(dev), self.coef.to(dev)

    def guarded(self, numel, dtype=torch.float32, pad=16):
        """(whole buffer, the view a kernel may write): `pad` sentinel elements on either side (16 floats: the view stays 16-byte aligned)."""
        whole = torch.full((numel + 2 * pad,), SENTINEL, dtype=dtype, device=self.dev)
        return whole, whole[pad:pad + numel]

    def run(self, ops, *, mode, cfg, scale, objective, step=0, avg=None, coef=None, **kw):
        """One GUIDE_X0 (reduce + apply) through ops.  Returns x0, |x0| on the host; asserts the sentinels around x0, |x0|, avg, partials."""
        B, n = self.B, self.n
        words = ops.ENUMS["IMAGEN_GUIDE_PARTIAL_DOUBLES"]
        w0, x0 = self.guarded(B * n)
        w1, ab = self.guarded(B * n)
        wp, part = self.guarded(B * words, torch.float64, pad=2)
        wa = None
        if avg is not None:
            wa, av = self.guarded(B * n)
            av.copy_(avg.reshape(-1).to(self.dev))
        step_ptr = torch.tensor([step], dtype=torch.int32, device=self.dev)
        plan = ops.Plan("guide_x0")
        ops.guide_x0(plan, self.xd, self.pd, self.cd if coef is None else coef.to(self.dev), step_ptr, x0, ab, B=B, n_per_sample=n, cfg=cfg,
                     cond_scale=DECOY if cfg == 2 else scale, mode=mode, objective=objective, avg=av if avg is not None else None, partials=part, **kw)
        assert [l for _, _, l in plan.ops] == ["guide_x0.reduce", "guide_x0.apply"]
        plan.run()
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        assert int(step_ptr.item()) == step, "GUIDE_X0 reads the counter, it does not advance it"
        for w, name, pad in ((w0, "x0", 16), (w1, "absx0", 16), (wp, "partials", 2)) + (((wa, "avg", 16),) if wa is not None else ()):
            assert bool((w[:pad] == SENTINEL).all()) and bool((w[-pad:] == SENTINEL).all()), f"{name}: written outside [B, n]"
        bps = min((n + 8191) // 8192, 64)
        pv = part.reshape(B, words)
        assert bool((pv[:, 4 * bps:] == SENTINEL).all()), "partials beyond the sample's workgroups were written"
        assert bool(torch.isfinite(pv[:, :4 * bps]).all())
        x0h, abh = x0.cpu().reshape(B, n), ab.cpu().reshape(B, n)
        assert torch.equal(abh, x0h.abs())
        return (x0h, abh) if avg is None else (x0h, abh, av.cpu().reshape(B, n))

    def cfg_x0(self, ops, *, cfg, scale, objective, step=0, rows=None):
        """CFG_X0 on the same inputs (rows: 'cond' = unguided on the cond rows)."""
        B, n = self.B, self.n
        x0, ab = torch.empty(B * n, device=self.dev), torch.empty(B * n, device=self.dev)
        step_ptr = torch.tensor([step], dtype=torch.int32, device=self.dev)
        plan = ops.Plan("cfg_x0")
        ops.cfg_x0(plan, self.xd, self.pd, self.cd, step_ptr, x0, ab, B=B, n_per_sample=n, cfg=0 if rows == "cond" else cfg,
                   cond_scale=DECOY if cfg == 2 else scale, objective=objective)
        plan.run()
        return x0.cpu().reshape(B, n)

    def want(self, *, mode, cfg, scale, objective, step=0, avg=None, coef=None, **kw):
        m = dict(rescale=RESCALE, apg=APG)[mode]
        thr = kw.pop("norm_threshold", None) or 0.0
        return guide_x0_contract(self.x, self.pred, (self.coef if coef is None else coef)[step], cfg=cfg, cond_scale=scale, objective=OBJECTIVES.index(objective),
                                 mode=m, norm_threshold=thr, avg=avg, dtype=torch.float64, **kw)


_CASES = {}


def case(B, n, draw=0):
    """The inputs of a shape, drawn once for the module (draw: further independent draws of the same shape)."""
    key = (B, n, draw, str(gpu_device()))
    if key not in _CASES:
        _CASES[key] = Case(B, n, 900 + 7 * B + n % 101 + 1000 * draw, gpu_device())
    return _CASES[key]


def _grid(n):
    """(cfg, step, scale) of a shape: every scale at cfg 1 and, through the table's column 7, cfg 2 — for the large n one of each."""
    if n == CAP_N:
        return [(1, 0, 7.5), (2, 2, -1.0)]
    return [(1, 0, s) for s in SCALES] + [(2, st, s) for st, s in ((0, 3.0), (1, 7.5), (2, -1.0))]


# ------------------------------------------------------------------------------------------------ rescale

@pytest.mark.parametrize("n", SMALL_N + (CAP_N,))
@pytest.mark.parametrize("B", [1, 3])
def test_rescale_against_fp64(ops, B, n):
    """phi {0, 0.7, 1} x objectives x cfg x scales per element against fp64; phi = 0 bit-equal to CFG_X0; two runs bit-equal."""
    c = case(B, n)
    worst = 0.0
    for objective in OBJECTIVES:
        for cfg, step, scale in _grid(n):
            for phi in (0.0, 0.7, 1.0):
                got, _ = c.run(ops, mode="rescale", cfg=cfg, scale=scale, objective=objective, step=step, phi=phi)
                want, _ = c.want(mode="rescale", cfg=cfg, scale=scale, objective=objective, step=step, phi=phi)
                err = nerr(got, want)
                worst = max(worst, err)
                assert err < TOL, (B, n, objective, cfg, scale, phi, err)
                if phi == 0.0:
                    assert torch.equal(got, c.cfg_x0(ops, cfg=cfg, scale=scale, objective=objective, step=step)), (objective, cfg, scale, "phi = 0 is CFG_X0")
                if phi == 0.7 and scale in (7.5, -1.0):
                    again, _ = c.run(ops, mode="rescale", cfg=cfg, scale=scale, objective=objective, step=step, phi=phi)
                    assert torch.equal(got, again), "two runs differ"
    print(f"rescale B={B} n={n}: worst normwise error vs fp64 {worst:.2e}")
    record_parity(f"guide_rescale[B{B}-n{n}]", worst=worst)


@pytest.mark.parametrize("n", [48, 1203, 12288])
def test_rescale_of_a_constant_sample_stays_finite(ops, n):
    """pred constant per sample and branch: var(g) == 0 exactly (dyadic values: every fp64 sum is exact), so the factor is 1 and the result is
    plain guidance's, finite; a sample whose cond alone is constant (var(cond) == 0, var(g) > 0) gets factor 0 at phi = 1: x0 of a zero output."""
    c = Case(3, n, 5, gpu_device())
    c.pred[:3] = torch.tensor([0.5, -0.25, 2.0])[:, None]
    c.pred[3:] = torch.tensor([0.25, 0.75, 2.0])[:, None]
    c.pred[5] = torch.randn(n, generator=torch.Generator().manual_seed(6))       # sample 2: cond constant, null not
    c.pd = c.pred.to(c.dev)
    for objective in OBJECTIVES:
        for phi in (0.7, 1.0):
            got, _ = c.run(ops, mode="rescale", cfg=1, scale=3.0, objective=objective, phi=phi)
            assert bool(torch.isfinite(got).all())
            plain = c.cfg_x0(ops, cfg=1, scale=3.0, objective=objective)
            assert nerr(got[:2], plain[:2]) < TOL, "factor 1 where var(g) == 0"
            want, _ = c.want(mode="rescale", cfg=1, scale=3.0, objective=objective, phi=phi)
            assert nerr(got, want) < TOL
            if phi == 1.0 and objective == "x_start":
                assert float(got[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ projected guidance

def _thresholds(c, objective, step):
    """none, binding (half the norm of the smallest sample's update), slack (twice the largest's) — from the fp64 contract's own D."""
    from plan_interp_guide import x0_of
    row = c.coef[step].double()
    o = OBJECTIVES.index(objective)
    d = x0_of(c.x.double(), c.pred[:c.B].double(), row[0], row[1], o) - x0_of(c.x.double(), c.pred[c.B:].double(), row[0], row[1], o)
    norms = d.norm(dim=1)
    return (None, float(norms.min()) * 0.5, float(norms.max()) * 2.0)


@pytest.mark.parametrize("n", SMALL_N + (CAP_N,))
@pytest.mark.parametrize("B", [1, 3])
def test_apg_against_fp64(ops, B, n):
    """eta {0, 1} x threshold {none, binding, slack} x objectives x cfg x scales, no momentum, per element against fp64; s = 1 bit-equal to
    the cond branch's x0; eta = 1 without threshold against plain CFG; two runs bit-equal."""
    c = case(B, n)
    worst = 0.0
    for objective in OBJECTIVES:
        for cfg, step, scale in _grid(n):
            for eta in (0.0, 1.0):
                for thr in _thresholds(c, objective, step):
                    kw = dict(mode="apg", cfg=cfg, scale=scale, objective=objective, step=step, eta=eta, norm_threshold=thr)
                    got, _ = c.run(ops, **kw)
                    want, _ = c.want(**kw)
                    err = nerr(got, want)
                    worst = max(worst, err)
                    assert err < TOL, (B, n, objective, cfg, scale, eta, thr, err)
                    if scale == 1.0:
                        assert torch.equal(got, c.cfg_x0(ops, cfg=cfg, scale=scale, objective=objective, step=step, rows="cond")), "s = 1 is the cond branch's x0"
                    if eta == 1.0 and thr is None:
                        plain = cfg_x0_contract(c.x.reshape(-1), c.pred.reshape(-1), c.coef[step], cfg=cfg, cond_scale=scale, objective=OBJECTIVES.index(objective),
                                                dtype=torch.float64).reshape(B, n)
                        assert nerr(got, plain) < TOL, "eta = 1 without threshold and momentum is plain guidance"
                    if eta == 0.0 and thr is not None and scale == 7.5:
                        again, _ = c.run(ops, **kw)
                        assert torch.equal(got, again), "two runs differ"
    print(f"apg B={B} n={n}: worst normwise error vs fp64 {worst:.2e}")
    record_parity(f"guide_apg[B{B}-n{n}]", worst=worst)


@pytest.mark.parametrize("n", [48, 1200, 1203, 12288])
@pytest.mark.parametrize("momentum", [0.0, -0.5])
def test_apg_momentum_over_three_steps(ops, n, momentum):
    """Three consecutive steps (table rows 0, 1, 2 at cfg 2: scales 3, 7.5, -1) on one running average that starts at zero: x0 and the
    average itself against the fp64 contract carried alongside; the threshold binds on some steps.  momentum 0 with a buffer: avg = D.
    Every step has its own draw of x and pred, as a sampler's steps have: with ONE pred for all steps the v objective's update is
    -sigma_i (cond - nul), and D_1 - 0.5 D_0 cancels to a few percent of its terms where sigma_1 ~ sigma_0 / 2 — the fp32 restatement alone then
    misses the bar on the average (9.5e-6 measured), which says nothing about the kernel."""
    B = 3
    draws = [case(B, n, k) for k in range(3)]
    for objective in OBJECTIVES:
        avg_k, avg_w = torch.zeros(B, n), torch.zeros(B, n, dtype=torch.float64)
        thr = _thresholds(draws[0], objective, 0)[1] * 2.5
        for step in range(3):
            c = draws[step]
            kw = dict(mode="apg", cfg=2, scale=0.0, objective=objective, step=step, eta=0.0, norm_threshold=thr, momentum=momentum)
            got, _, avg_k = c.run(ops, avg=avg_k, **kw)
            want, avg_w = c.want(avg=avg_w, **kw)
            assert nerr(got, want) < TOL and nerr(avg_k, avg_w) < TOL, (n, objective, step, nerr(got, want), nerr(avg_k, avg_w))
        assert momentum == 0.0 or nerr(avg_k, c.want(avg=torch.zeros(B, n, dtype=torch.float64), **kw)[1]) > 1e3 * TOL, "the average carries the earlier steps"


def test_apg_zero_cond_row_stays_finite(ops):
    """A sample whose cond prediction makes Dc == 0 everywhere (x_start objective, cond = 0): <Dc, Dc> == 0, the coefficient is 0, x0 = (s - 1) r D."""
    c = Case(3, 1203, 9, gpu_device())
    c.pred[1] = 0.0
    c.pd = c.pred.to(c.dev)
    for eta in (0.0, 1.0):
        for thr in (None, 5.0):
            kw = dict(mode="apg", cfg=1, scale=7.5, objective="x_start", eta=eta, norm_threshold=thr)
            got, _ = c.run(ops, **kw)
            want, _ = c.want(**kw)
            assert bool(torch.isfinite(got).all()) and nerr(got, want) < TOL
            r = 1.0 if thr is None else min(1.0, thr / float(c.pred[4].double().norm()))
            assert nerr(got[1], 6.5 * r * (-c.pred[4])) < TOL
    # every row zero on both branches: D == 0 too, the cap's 0 / 0 never happens (r = 1), x0 = 0
    c.pred.zero_()
    c.pd = c.pred.to(c.dev)
    got, _ = c.run(ops, mode="apg", cfg=1, scale=7.5, objective="x_start", eta=0.0, norm_threshold=5.0)
    assert float(got.abs().max()) == 0.0


def test_launcher_refuses_bad_fields(ops):
    """The C side validates what the Python side would (a caller binding the ABI directly): nothing is launched."""
    import ctypes
    from imagen_pytorch_amd import _abi

    c = case(1, 48)
    lib = _abi.load_library()
    for field, value, msg in (("mode", 3, b"mode"), ("phase", 2, b"phase"), ("cfg", 0, b"cfg"), ("objective", 3, b"objective"), ("phi", 1.5, b"phi"),
                              ("momentum", -0.5, b"running average"), ("partials", None, b"required")):
        plan = ops.Plan()
        x0, ab = torch.empty(48, device=c.dev), torch.empty(48, device=c.dev)
        p = ops.guide_x0(plan, c.xd, c.pd, c.cd, torch.zeros(1, dtype=torch.int32, device=c.dev), x0, ab, B=1, n_per_sample=48, cfg=1, cond_scale=3.0,
                         mode="apg" if field == "momentum" else "rescale")[0]
        setattr(p, field, value)
        assert lib.imagen_launch(_abi.ENUMS["IMAGEN_OP_GUIDE_X0"], ctypes.addressof(p), ctypes.sizeof(p), ops.current_stream_handle()) != 0
        assert msg in lib.imagen_last_error(), (field, lib.imagen_last_error())
