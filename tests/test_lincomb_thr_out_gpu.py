"""LINCOMB's two optional outputs (ABI 13: ImagenLincombParams.thr1_out / thr3_out) branch by branch against fp64: each receives
thr(t1, q1) / thr(t3, q3), exactly the value that enters the sum, whatever the weight of its term and whatever the mask; with both NULL the
launch is the one of before.  thr_mode 0 / 1 / 2 with quantiles below and above 1, each output set or NULL, mask set or not; three sizes:
B = 3 samples of 3 * 16 * 16, of 4 (one 4-element group per sample), and of 4 * 171 (513 groups: three blocks of 256 threads, the last one
with a single live thread).  Sentinels in front of and behind both outputs.

Bar: tests/test_sampler_kernels_gpu.py's for LINCOMB — normwise 1e-6 against fp64; the emitted operands are one clamp and one division of
an fp32 input, and are held bit-exact against the same fp32 arithmetic as well.  Every case runs once with w1 = 0 and once with
w3 = 0, so each output is checked both with its term out of the sum and in it.  Measured on MI355X over the 144 cases: out <= 4.4e-8,
thr outputs <= 1.1e-8 (0 wherever thr_mode != 1: no division); the same file on the CPU emulation of the kernel
(tests/test_selfcond_cpu.py::test_emulated_lincomb_thr_outputs) passes the same assertions."""
import itertools

import pytest
import torch

from conftest import gpu_device, record_parity

pytestmark = pytest.mark.gpu

TOL = 1e-6
# weight rows w0..w5 (w4 = 0: no noise), at table row 2: an output is written whatever the weight of its term — once with that weight 0,
# once with it in the sum while the other one's is 0
WEIGHTS = {"w1=0": [0.83, 0.0, 0.27, 0.64, 0.0, -1.7], "w3=0": [-0.41, 1.3, 0.55, 0.0, 0.0, 0.9]}
SIZES = {"3x16x16": 3 * 16 * 16, "one-group": 4, "ragged-grid": 4 * 171}
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    return gpu_device()


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o

    return o


@pytest.fixture(scope="module")
def data():
    """Inputs per size, drawn once: t1 / t3 wide enough that every clamp bites, quantiles on both sides of 1."""
    out = {}
    for name, n in SIZES.items():
        g = torch.Generator().manual_seed(1000 + n)
        B = 3
        t = [torch.randn(B, n, generator=g) * s for s in (1.0, 2.5, 0.7, 4.0)]
        out[name] = dict(B=B, n=n, t=t, q1=torch.tensor([0.5, 1.8, 3.2]), q3=torch.tensor([2.7, 0.9, 1.0]),
                         mask=(torch.rand(B, n, generator=g) > 0.4).float(), keep=torch.randn(B, n, generator=g))
    return out


def nerr64(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).norm() / ref.norm().clamp(min=1e-300)).item()


def guarded(n, dev, fill):
    """GUARD sentinel words, an n-word buffer, GUARD sentinel words: (buffer, front, back)."""
    t = torch.full((n + 2 * GUARD,), fill, device=dev)
    return t[GUARD:GUARD + n], t[:GUARD], t[GUARD + n:]


def thr64(t, q, mode):
    t = t.double()
    if mode == 1:
        s = q.double().clamp(min=1.0).view(-1, 1)
        return torch.maximum(torch.minimum(t, s), -s) / s
    return t.clamp(-1.0, 1.0) if mode == 2 else t


def thr32(t, q, mode):
    """The kernel's own fp32 arithmetic: fminf(fmaxf(t, -s), s) / s."""
    if mode == 0:
        return t
    s = q.clamp(min=1.0).view(-1, 1) if mode == 1 else torch.ones(t.shape[0], 1)
    return torch.minimum(torch.maximum(t, -s), s) / s


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("emit", list(itertools.product([False, True], repeat=2)), ids=lambda e: f"thr1_{'set' if e[0] else 'null'}-thr3_{'set' if e[1] else 'null'}")
@pytest.mark.parametrize("thr_mode", [0, 1, 2])
@pytest.mark.parametrize("weights", list(WEIGHTS))
def test_lincomb_thr_outputs(ops, dev, data, weights, thr_mode, emit, masked, size):
    d = data[size]
    B, n = d["B"], d["n"]
    t0, t1, t2, t3 = d["t"]
    coef = torch.zeros(3, 8)
    coef[2, :6] = torch.tensor(WEIGHTS[weights])
    step = torch.tensor([2], dtype=torch.int32, device=dev)
    q = dict(q1=d["q1"].to(dev), q3=d["q3"].to(dev)) if thr_mode == 1 else {}
    mk = dict(mask=d["mask"].to(dev), mask_else=d["keep"].to(dev)) if masked else {}
    ins = [t.to(dev) for t in (t0, t1, t2, t3)]

    def launch(**outs):
        out, out2 = torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
        plan = ops.Plan()
        ops.lincomb(plan, ins[0], out, coef.to(dev), step, B=B, n_per_sample=n, t1=ins[1], t2=ins[2], t3=ins[3], out2=out2, thr_mode=thr_mode,
                    **q, **mk, **outs)
        plan.run()
        torch.cuda.synchronize()
        return out.cpu(), out2.cpu()

    o1, f1, b1 = guarded(B * n, dev, 55.0)
    o3, f3, b3 = guarded(B * n, dev, -77.0)
    out, out2 = launch(thr1_out=o1 if emit[0] else None, thr3_out=o3 if emit[1] else None)
    w = coef[2].double()
    a, c = thr64(t1, d["q1"], thr_mode), thr64(t3, d["q3"], thr_mode)
    ref = w[0] * t0.double() + w[1] * a + w[2] * t2.double() + w[3] * c
    if masked:
        ref = torch.where(d["mask"] != 0, ref, d["keep"].double())
    e = nerr64(out, ref)
    print(f"lincomb[{weights}, {thr_mode}, {emit}, mask={masked}, {size}]: out {e:.2e}")
    assert e <= TOL and nerr64(out2, w[5] * ref) <= TOL, e
    errs = {}
    for name, set_, buf, front, back, fill, want64, want32 in (("thr1", emit[0], o1, f1, b1, 55.0, a, thr32(t1, d["q1"], thr_mode)),
                                                               ("thr3", emit[1], o3, f3, b3, -77.0, c, thr32(t3, d["q3"], thr_mode))):
        assert bool((front.cpu() == fill).all()) and bool((back.cpu() == fill).all()), f"{name}_out: a store outside the buffer"
        got = buf.cpu().view(B, n)
        if not set_:
            assert bool((got == fill).all()), f"{name}_out is NULL: nothing may be written"
            continue
        errs[name] = nerr64(got, want64)
        print(f"    {name}_out {errs[name]:.2e}")
        assert errs[name] <= TOL, (name, errs[name])
        assert torch.equal(got, want32), f"{name}_out is not the value that enters the sum"      # mask or not, weight or not
    # both NULL == a launch whose params omit the two fields (the call of before ABI 13), bit for bit
    if emit == (False, False):
        again, again2 = launch()
        assert torch.equal(again, out) and torch.equal(again2, out2)
    else:
        plain, plain2 = launch()
        assert torch.equal(plain, out) and torch.equal(plain2, out2), "emitting the operands must not change out / out2"
    assert int(step.item()) == 2
    record_parity(f"lincomb_thr_out[{weights}-{thr_mode}-{emit}-{masked}-{size}]", out=e, **errs)
