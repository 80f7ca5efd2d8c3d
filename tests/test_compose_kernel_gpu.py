"""MI355X (-m gpu; also on the CPU emulation, IMAGEN_EMUL_TESTS=1: tests/test_compose_cpu.py keeps the file in the CPU suite): COMPOSE_X0 of
csrc/sampler.hip per element against its contract evaluated in fp64 (tests/plan_interp_compose.py), on sentinel-guarded output buffers.

Shapes: B in {1, 3}; K in {1, 2, 4}; (C, hw) in {(3, 16), (3, 400), (3, 401), (3, 4096), (1, 524289)}, i.e. n = 48 (less than a workgroup), 1200 (a
partial last workgroup), 1203 (n and hw no multiples of 4: the scalar path, where a group of 4 elements straddles two channel planes), 12288
(several workgroups per sample), 524289 (one large sample, odd).  The three objectives; weights from {0, 1, 3, 7.5, -1}, differing per sample and
prompt; masks none, binary, fractional.  The large n runs one (K, objective, mask kind) per K — the paths it adds do not depend on them.
One case has `pred` and `masks` 4 bytes off a 16-byte boundary (n, hw multiples of 4): it must take the scalar path and meet the bar.

Bar: TOL = 1e-6 normwise against fp64, the project's bar of the sampler kernels (tests/test_guide_kernel_gpu.py, tests/test_sampler_kernels_gpu.py).
Inputs: x, pred standard normal, alpha, sigma in [0.05, 0.95] as those tests draw them.

Identities (torch.equal): K = 1 without masks == CFG_X0 at cfg = 1; a mask of ones == no mask; a prompt at weight 0 or under a mask of zeros ==
the composition without it.  (K = 2 with identical rows at weights (a, b) is NOT the one prompt at a + b: fp32 sums do not regroup.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import gpu_device, record_parity  # noqa: E402
from plan_interp_compose import compose_x0_contract  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
OBJECTIVES = ("noise", "x_start", "v")
WEIGHTS = (0.0, 1.0, 3.0, 7.5, -1.0)
KS = (1, 2, 4)
SHAPES = ((3, 16), (3, 400), (3, 401), (3, 4096), (1, 524289))
LARGE = 524289
MASKS = ("none", "binary", "fractional")
SENTINEL = -77.25
KMAX = 4


def nerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o
    return o


class Case:
    """Inputs of one (B, C, hw), drawn once for KMAX prompts (a smaller K reads the first K prompt branches and the null rows, restacked)."""

    def __init__(self, B, C, hw, seed, dev):
        g = torch.Generator().manual_seed(seed)
        self.B, self.C, self.hw, self.n, self.dev = B, C, hw, C * hw, dev
        self.x = torch.randn(B, self.n, generator=g)
        self.branches = torch.randn(KMAX + 1, B, self.n, generator=g)           # [KMAX] is the null branch
        self.coef = torch.rand(3, 8, generator=g) * 0.9 + 0.05
        self.binary = (torch.rand(KMAX, B, hw, generator=g) > 0.5).float()
        self.fractional = torch.rand(KMAX, B, hw, generator=g)
        self.xd, self.cd = self.x.to(dev), self.coef.to(dev)

    def pred(self, K):
        return torch.cat([self.branches[:K], self.branches[KMAX:]]).reshape((K + 1) * self.B, self.n).contiguous()

    def weights(self, K, shift=0):
        w = torch.tensor([[WEIGHTS[(2 * k + b + shift) % len(WEIGHTS)] for b in range(self.B)] for k in range(K)], dtype=torch.float32)
        return w

    def masks(self, K, kind):
        return None if kind == "none" else getattr(self, kind)[:K].contiguous()

    def off16(self, t, off):
        """`t` on the device at `off` floats past a 16-byte boundary."""
        buf = torch.empty(t.numel() + 4, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + t.numel()].view(t.shape)
        view.copy_(t)
        return view

    def run(self, ops, pred, weights, masks, objective, step=0, off=0):
        """One COMPOSE_X0 through ops.  Returns x0 on the host; asserts the sentinels around x0 and |x0|, and |x0| == abs(x0)."""
        B, n = self.B, self.n
        outs = []
        for _ in range(2):
            whole = torch.full((B * n + 32,), SENTINEL, device=self.dev)
            outs.append((whole, whole[16:16 + B * n]))
        (w0, x0), (w1, ab) = outs
        step_ptr = torch.tensor([step], dtype=torch.int32, device=self.dev)
        pd, wd = self.off16(pred, off), weights.to(self.dev)
        md = None if masks is None else self.off16(masks, off)
        assert pd.data_ptr() % 16 == 4 * off and pd.is_contiguous()
        plan = ops.Plan("compose_x0")
        ops.compose_x0(plan, self.xd, pd, self.cd, step_ptr, x0, ab, B=B, n_per_sample=n, hw=self.hw, weights=wd, masks=md, objective=objective)
        assert [l for _, _, l in plan.ops] == ["compose_x0"]
        plan.run()
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        assert int(step_ptr.item()) == step, "COMPOSE_X0 reads the counter, it does not advance it"
        for w, name in ((w0, "x0"), (w1, "absx0")):
            assert bool((w[:16] == SENTINEL).all()) and bool((w[-16:] == SENTINEL).all()), f"{name}: written outside [B, n]"
        x0h, abh = x0.cpu().reshape(B, n), ab.cpu().reshape(B, n)
        assert torch.equal(abh, x0h.abs())
        return x0h

    def want(self, pred, weights, masks, objective, step=0):
        return compose_x0_contract(self.x, pred, self.coef[step], weights, masks, objective=OBJECTIVES.index(objective), dtype=torch.float64)

    def cfg_x0(self, ops, pred, scale, objective, step=0):
        B, n = self.B, self.n
        x0, ab = torch.empty(B * n, device=self.dev), torch.empty(B * n, device=self.dev)
        step_ptr = torch.tensor([step], dtype=torch.int32, device=self.dev)
        plan = ops.Plan("cfg_x0")
        ops.cfg_x0(plan, self.xd, pred.to(self.dev), self.cd, step_ptr, x0, ab, B=B, n_per_sample=n, cfg=1, cond_scale=scale, objective=objective)
        plan.run()
        return x0.cpu().reshape(B, n)


_CASES = {}


def case(B, C, hw):
    key = (B, C, hw, str(gpu_device()))
    if key not in _CASES:
        _CASES[key] = Case(B, C, hw, 700 + 11 * B + hw % 97, gpu_device())
    return _CASES[key]


def _grid(hw):
    if hw == LARGE:
        return [(1, "noise", "none"), (2, "x_start", "binary"), (4, "v", "fractional")]
    return [(K, o, m) for K in KS for o in OBJECTIVES for m in MASKS]


@pytest.mark.parametrize("C,hw", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_compose_against_fp64(ops, B, C, hw):
    """K x objectives x masks per element against fp64; two runs bit-equal."""
    c = case(B, C, hw)
    worst = 0.0
    for i, (K, objective, kind) in enumerate(_grid(hw)):
        pred, w, m = c.pred(K), c.weights(K, shift=i), c.masks(K, kind)
        got = c.run(ops, pred, w, m, objective, step=i % 3)
        err = nerr(got, c.want(pred, w, m, objective, step=i % 3))
        worst = max(worst, err)
        assert err < TOL, (B, C, hw, K, objective, kind, err)
        if K == 4 and kind == "fractional":
            assert torch.equal(got, c.run(ops, pred, w, m, objective, step=i % 3)), "two runs differ"
    print(f"compose B={B} n={C * hw} hw={hw}: worst normwise error vs fp64 {worst:.2e}")
    record_parity(f"compose_kernel[B{B}-n{C * hw}]", worst=worst)


def test_unaligned_pred_and_masks_take_the_scalar_path(ops):
    """n = 1200, hw = 400 (both multiples of 4), but pred and masks start 4 bytes past a 16-byte boundary: 16-byte loads would be misaligned,
    so the launcher must pick the scalar kernel; the result equals the aligned run's bits (the same fp32 expressions) and meets the bar."""
    c = case(3, 3, 400)
    for K, objective, kind in ((2, "noise", "fractional"), (4, "v", "binary"), (1, "x_start", "none")):
        pred, w, m = c.pred(K), c.weights(K, shift=1), c.masks(K, kind)
        got = c.run(ops, pred, w, m, objective, off=1)
        err = nerr(got, c.want(pred, w, m, objective))
        print(f"unaligned K={K} {objective} {kind}: {err:.2e}")
        assert err < TOL
        assert torch.equal(got, c.run(ops, pred, w, m, objective, off=0)), "scalar and vector paths differ"


@pytest.mark.parametrize("C,hw", SHAPES[:4])
@pytest.mark.parametrize("B", [1, 3])
def test_identities(ops, B, C, hw):
    c = case(B, C, hw)
    ones, zeros = torch.ones(KMAX, B, hw), torch.zeros(KMAX, B, hw)
    for objective in OBJECTIVES:
        # K = 1 without masks and weights[0][b] = s: the bits of CFG_X0 at cfg = 1, cond_scale = s
        for s in WEIGHTS:
            got = c.run(ops, c.pred(1), torch.full((1, B), s), None, objective)
            assert torch.equal(got, c.cfg_x0(ops, c.pred(1), s, objective)), (objective, s, "K = 1 is CFG_X0")
        for K in (2, 4):
            pred, w = c.pred(K), c.weights(K, shift=2)
            plain = c.run(ops, pred, w, None, objective)
            assert torch.equal(plain, c.run(ops, pred, w, ones[:K].contiguous(), objective)), "a mask of ones is no mask"
            # the last prompt at weight 0, or under a mask of zeros: the composition of the first K - 1 prompts
            less = c.run(ops, c.pred(K - 1), w[:K - 1].contiguous(), None, objective)
            w0 = w.clone()
            w0[K - 1] = 0.0
            assert torch.equal(c.run(ops, pred, w0, None, objective), less), "a prompt at weight 0 drops out"
            m = ones[:K].clone()
            m[K - 1] = zeros[0]
            assert torch.equal(c.run(ops, pred, w, m, objective), less), "a prompt under a mask of zeros drops out"
            # ... and the FIRST prompt dropped is the composition of the others
            rest = torch.cat([c.branches[1:K], c.branches[KMAX:]]).reshape(K * B, c.n).contiguous()
            w0 = w.clone()
            w0[0] = 0.0
            assert torch.equal(c.run(ops, pred, w0, None, objective), c.run(ops, rest, w[1:].contiguous(), None, objective))


def test_launcher_refuses_bad_fields(ops):
    """The C side validates what the Python side would (a caller binding the ABI directly): nothing is launched."""
    import ctypes
    from imagen_pytorch_amd import _abi

    c = case(1, 3, 16)
    lib = _abi.load_library()
    kind = _abi.ENUMS["IMAGEN_OP_COMPOSE_X0"]
    for field, value, msg in (("K", 0, b"K outside"), ("K", 5, b"K outside"), ("hw", 0, b"hw <= 0"), ("hw", -4, b"hw <= 0"), ("hw", 5, b"no multiple of hw"),
                              ("objective", 3, b"objective"), ("weights", None, b"required"), ("n_per_sample", 0, b"n_per_sample")):
        x0, ab = torch.empty(48, device=c.dev), torch.empty(48, device=c.dev)
        p = ops.compose_x0(ops.Plan(), c.xd, c.pred(2).to(c.dev), c.cd, torch.zeros(1, dtype=torch.int32, device=c.dev), x0, ab, B=1, n_per_sample=48,
                           hw=16, weights=c.weights(2).to(c.dev))
        setattr(p, field, value)
        assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p), ops.current_stream_handle() if c.dev.type == "cuda" else None) != 0
        assert msg in lib.imagen_last_error(), (field, lib.imagen_last_error())
