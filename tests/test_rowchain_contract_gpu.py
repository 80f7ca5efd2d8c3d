"""ROWCHAIN (csrc/rowchain.hip) against an fp64 restatement of its contract (the ROWCHAIN block of include/imagen_hip.h), mode by mode, at the
shapes the launcher takes and tests/test_rowchain_gpu.py does not reach: every K-split of make_part() (exact, uneven, clamped by the K steps),
two cout tiles per wave, one tile per image with several images, key counts of one tile / one key past a tile / many tiles, a row maximum
that arrives in the last key tile, ln_stats given and computed, gate / request_prep present and absent, prep_C2 that is no multiple of 32.

The reference rounds every INTERMEDIATE to fp16 where the header writes fp16(...) and keeps the softmax weights in fp64; the last fp16(...) of an
output is left out.  Against the rounded value the error of a row is the count of its elements that landed on the other fp16 neighbour: zero for
most rows of a correct plan, one ulp of one element for a few, so that the worst row of two correct plans differs by whichever element
happened to flip (2.5e-4 against 5.4e-5 from ONE flipped element of RESPREP's `out`, and 0 for a whole tensor, were seen on the emulation).
Against the unrounded value every element carries its own rounding error of up to half an ulp, the same for both plans, and a flip moves it
from just under to just over that.  Weights are fp16-representable (what pack_weight stores), gains and scales fp32 values, inputs
fp16-representable.

What a case asserts:
 * per ROW, e_r = |got_r - ref_r| / |ref_r|: the worst row of the chain is at most twice the worst row of the launch-per-op plan it replaces
   (IGEMM, LN_RESIDUAL, ROWSTAT, ATTENTION, KV_PREP, ACT_PREP on the same inputs against the same reference).  The header claims the same
   rounding points for both, so what legitimately differs is the fp32 summation order and the occasional one-ulp flip of an intermediate fp16
   rounding: a factor 2.  A dropped K step, another image's gate row or a wrong head is 100 x beyond it, and in one row it is not diluted by
   the other rows as in a whole-tensor norm.  The whole-tensor figure of both plans stays under the project's per-op bar (TOL).
 * RESPREP's `out` has no intermediate rounding, so it is also checked per ELEMENT: |got - exact| <= ulp16(exact) + (K + 4) ulp32 sum|terms|
   (the stored value is a neighbour of the exact one; K products and the bias / addend terms added in any order, a full ulp32 granted per
   addition because the matrix pipe's additions are not specified to round to nearest).
 * ssq_out per row against the sum of squares of the fp16 row the kernel stored, at `sum_bound`: C / 8 / LPR groups of 8 per lane, then
   row_sum<LPR>, LPR = 16 at 32-row tiles and 8 at 64-row tiles.
 * every output (out, ssq_out, prep_out, QKV's K^ and V^T) lies in a `guarded` allocation: the sentinels around it, in the gaps of strided rows,
   in the K^ rows / V^T columns outside [r0, r0 + N) and in columns inner .. inner + 127 of QKV's output rows survive.  The gaps of strided
   inputs hold NaN.
Strides: the wrappers ask for bs == N * ld on every tensor (any ld % 8 == 0), and request_prep for a dense `out` and allocates a dense
prep_out itself, so ld_prep > C + prep_C2 and ld_out > C together with a prep request (both of which the launcher takes) are not reachable
here; the test moves prep_out into a guarded allocation of the same layout by rewriting the pointer of the params struct.

Runs on MI355X (-m gpu) and on the CPU emulation (IMAGEN_EMUL_TESTS=1; tests/test_igemm_emulated.py keeps it in the CPU suite)."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import gpu_device, record_parity
from test_elementwise_kernels_gpu import ULP32, guarded, rows_mask, strided16, sum_bound, ulp16

pytestmark = pytest.mark.gpu

TOL = 1e-3              # the project's per-op bar on the whole-tensor figure (tests/test_rowchain_gpu.py)
EPS = 1e-5
HEADS, DH, INNER = 8, 64, 512


# ------------------------------------------------------------------------------------------------ helpers

def r16(t):
    """fp16(...) of the contract on fp64 values."""
    return t.to(torch.float16).double()


def rnd16(*shape, scale=1.0):
    return r16(torch.randn(*shape, dtype=torch.float64) * scale)


def w16(cout, cin):
    """A weight pack_weight stores without rounding: (fp32 for the packer, fp64 for the reference)."""
    w = (torch.randn(cout, cin) / math.sqrt(cin)).half().float()
    return w, w.double()


def gain(n):
    g = (1 + 0.1 * torch.randn(n)).float()
    return g, g.double()


def ln64(x, g):
    mu = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * g


def dense(ops, vals, dev):
    B, N, C = vals.shape
    return strided16(ops, vals, C, N * C, dev)


def rows_of(flat, B, N, C, ld):
    return flat.as_strided((B, N, C), (N * ld, ld, 1)).clone()


def with_tiles(cases, n_at=1):
    """(case..., tile64) for both tile heights where the rows of an image allow 64."""
    out = []
    for c in cases:
        for t64 in (False, True) if c[n_at] % 64 == 0 else (False,):
            out.append(pytest.param(*c, t64, id="-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c) + ("-tile64" if t64 else "-tile32")))
    return out


def set_tiles(monkeypatch, ops, t64):
    monkeypatch.setattr(ops, "CHAIN_TILE64_MIN_ROWS", 1 if t64 else 1 << 30)


def figures(got, ref):
    """(worst per-row relative error, whole-tensor relative error) of rows [..., C] in fp64; a NaN (an unwritten sentinel) counts as inf."""
    got, ref = got.detach().cpu().double(), ref.double()
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    d = got - ref
    e = torch.nan_to_num(d.norm(dim=-1) / ref.norm(dim=-1).clamp(min=1e-300), nan=float("inf"))
    return float(e.max()), float(torch.nan_to_num(d.norm() / ref.norm(), nan=float("inf")))


class Verdict:
    """The figures and failures of one case: everything is measured and recorded before anything is asserted."""

    def __init__(self, test_id):
        self.id, self.figs, self.fail = test_id, {}, []

    def rows(self, name, chain, unfused, ref):
        wc, tc = figures(chain, ref)
        wu, tu = figures(unfused, ref)
        self.figs.update({f"{name}.chain_row": wc, f"{name}.unfused_row": wu, f"{name}.chain_all": tc, f"{name}.unfused_all": tu})
        if not wc <= 2 * wu:
            self.fail.append(f"{name}: worst row of the chain {wc:.3e} > 2 x that of the launch-per-op plan {wu:.3e}")
        if not tc < TOL:
            self.fail.append(f"{name}: whole-tensor figure of the chain {tc:.3e} >= {TOL}")
        if not tu < TOL:
            self.fail.append(f"{name}: whole-tensor figure of the launch-per-op plan {tu:.3e} >= {TOL}")

    def ssq(self, name, got, stored, C, t64):
        lpr = 8 if t64 else 16
        want = (stored.double() ** 2).sum(-1).reshape(-1)
        e = (got.detach().cpu().double().reshape(-1) - want).abs() / want.clamp(min=1e-300)
        e = float(torch.nan_to_num(e, nan=float("inf")).max())
        bar = sum_bound(max(1, -(-(C // 8) // lpr)), lpr)
        self.figs[f"{name}.ssq_row"] = e
        if not e <= bar:
            self.fail.append(f"{name}: ssq_out off by {e:.3e} of its row's sum (bar {bar:.3e})")

    def guard(self, name, g, mask=None):
        try:
            g.check(mask)
        except AssertionError as ex:
            self.fail.append(f"{name}: {ex}")

    def check(self, name, ok, msg=""):
        if not ok:
            self.fail.append(f"{name}: {msg}")

    def done(self):
        record_parity(self.id, **self.figs)
        print(self.id, " ".join(f"{k}={v:.3e}" for k, v in self.figs.items()))
        assert not self.fail, "\n".join(self.fail)


def out_buffer(ops, B, N, C, ld, dev):
    g = guarded(B * N * ld, dev)
    return g, g.act(ops, B, N, C, ld, N * ld), rows_mask(B * N * ld, B, N, C, ld, N * ld)


# ------------------------------------------------------------------------------------------------ mode 1: FF

#            B, N,   C,   hidden, strided
FF_CASES = [(2, 64, 32, 512, False),      # two cout tiles per wave (lin1: 16 tiles) with the narrowest C
            (2, 64, 256, 32, False),      # lin1: one cout tile, its 16 K steps over 8 waves; lin2 with 2 K steps
            (3, 32, 64, 64, False),       # one tile per image
            (1, 128, 128, 512, True),
            (2, 64, 32, 32, False)]       # lin1 / lin2: 2 K steps, wk = 8 clamped to 2


@pytest.mark.parametrize("B,N,C,hidden,strided,t64", with_tiles(FF_CASES))
def test_ff(B, N, C, hidden, strided, t64, monkeypatch):
    """x1 = fp16(LN(fp16(o W_out^T)) g0 + res); hid = fp16(gelu(fp16(LN(x1) g1) W1^T)); out = fp16(fp16(LN(hid) g2) W2^T + x1)."""
    from imagen_pytorch_amd import ops
    dev = gpu_device()
    set_tiles(monkeypatch, ops, t64)
    torch.manual_seed(10)
    o, tok = rnd16(B, N, INNER), rnd16(B, N, C)
    (w_out, w_out64), (w1, w1_64), (w2, w2_64) = w16(C, INNER), w16(hidden, C), w16(C, hidden)
    (g_out, g_out64), (g0, g0_64), (g1, g1_64) = gain(C), gain(C), gain(hidden)
    x1 = r16(ln64(r16(o @ w_out64.t()), g_out64) + tok)
    hid = r16(F.gelu(r16(ln64(x1, g0_64)) @ w1_64.t()))
    ref = r16(ln64(hid, g1_64)) @ w2_64.t() + x1
    pw_out, pw1, pw2 = ops.pack_weight(w_out, None, dev), ops.pack_weight(w1, None, dev), ops.pack_weight(w2, None, dev)
    gd = [t.to(dev) for t in (g_out, g0, g1)]
    assert ops.rowchain_ok(C, N, HEADS, DH, pw_out, pw1, pw2, hidden=hidden)
    # the launch-per-op plan
    oa, toka = dense(ops, o, dev), dense(ops, tok, dev)
    plan = ops.Plan("unfused")
    y = ops.new_act(B, 1, N, C, dev)
    ops.igemm(plan, oa, pw_out, y)
    x1a = ops.new_act(B, 1, N, C, dev)
    st = (torch.empty(B * N, device=dev), torch.empty(B * N, device=dev))
    ops.ln_residual(plan, y, gd[0], x1a, res=toka, ln_stats_out=st)
    hida = ops.new_act(B, 1, N, hidden, dev)
    ops.igemm(plan, x1a, pw1, hida, mu=st[0], rs=st[1], pa=gd[1], act_out=ops.ACT_GELU)
    mu2, rs2 = torch.empty(B * N, device=dev), torch.empty(B * N, device=dev)
    ops.rowstat(plan, hida, mode=1, rs=rs2, mu=mu2)
    outa = ops.new_act(B, 1, N, C, dev)
    ops.igemm(plan, hida, pw2, outa, mu=mu2, rs=rs2, pa=gd[2], res=x1a)
    plan.run()
    # one ROWCHAIN launch
    pad = 8 if strided else 0
    ob = strided16(ops, o, INNER + pad, N * (INNER + pad), dev)
    tokb = strided16(ops, tok, C + 2 * pad, N * (C + 2 * pad), dev)
    ld_out = C + 3 * pad
    g_o, outb, mask = out_buffer(ops, B, N, C, ld_out, dev)
    g_s = guarded(B * N, dev, torch.float32)
    chain = ops.Plan("chain")
    ops.rowchain_ff(chain, ob, tokb, outb, pw_out, gd[0], pw1, gd[1], pw2, gd[2], rows_per_batch=N, ssq_out=g_s.t)
    chain.run()
    torch.cuda.synchronize()
    v = Verdict(f"rowchain_contract.ff[{B}x{N}x{C} hidden {hidden} tile{64 if t64 else 32}{' strided' if strided else ''}]")
    got = rows_of(g_o.cpu(), B, N, C, ld_out)
    v.rows("out", got, outa.t.reshape(B, N, C), ref)
    v.ssq("out", g_s.cpu(), got, C, t64)
    v.guard("out", g_o, mask)
    v.guard("ssq_out", g_s)
    v.done()


# ------------------------------------------------------------------------------------------------ mode 2: XATTN

#            B, N,  C,  J,  kind,  strided     kind: "rand" | "stats" (also with the caller's LayerNorm statistics) | ("late", dominant key, opposite key)
XA_CASES = [(2, 64, C, J, "rand", False) for C in (32, 256) for J in (1, 32, 64, 97, 292)] + [
    (2, 64, 32, 33, "rand", True),
    (2, 64, 256, 33, "stats", False),
    (2, 64, 256, 97, ("late", 96, 50), False),     # every query's maximum arrives with key 96, alone in the last tile: alpha rescales everything before it
    (2, 64, 256, 97, ("late", 0, 96), False)]      # ... with key 0: the later tiles only add small weights, the last one the smallest there is


def _xa_id(c):
    kind = c[4] if isinstance(c[4], str) else "late%d" % c[4][1]
    return f"{c[0]}-{c[1]}-{c[2]}-J{c[3]}-{kind}" + ("-strided" if c[5] else "")


@pytest.mark.parametrize("B,N,C,J,kind,strided", [pytest.param(*c, id=_xa_id(c)) for c in XA_CASES])
def test_xattn(B, N, C, J, kind, strided, monkeypatch):
    """q = fp16(fp16(LN(x) g0) Wq^T); o_h = fp16(softmax_j(q^_h . K^[b, h, j]) @ V[b, h]) with q^ = fp16(q / |q| q_scale q_mult), the softmax
    weights unrounded; out = fp16(LN(fp16(o W_out^T)) g1 + x).  Always 32-row tiles (the launcher ignores tile64 here)."""
    from imagen_pytorch_amd import ops
    dev = gpu_device()
    set_tiles(monkeypatch, ops, False)
    torch.manual_seed(11)
    late = kind if isinstance(kind, tuple) else None
    x = rnd16(B, N, C)
    if late:   # the rows of an image are one row at 64 different lengths: LayerNorm gives every query of the image (nearly) the same direction
        x = r16(x[:, :1] * (1 + torch.rand(B, N, 1, dtype=torch.float64)))
    (wq, wq64), (w_out, w_out64) = w16(INNER, C), w16(C, INNER)
    (g_n, g_n64), (g_o, g_o64) = gain(C), gain(C)
    q_scale, k_scale = ((torch.ones(DH), torch.ones(DH)) if late else ((1 + 0.1 * torch.randn(DH)).float(), (1 + 0.1 * torch.randn(DH)).float()))
    q_mult = 8.0 * ops.LOG2E
    q = r16(r16(ln64(x, g_n64)) @ wq64.t()).reshape(B, N, HEADS, DH).permute(0, 2, 1, 3)
    k = torch.randn(B, HEADS, J, DH, dtype=torch.float64)
    khat = r16(F.normalize(k, dim=-1) * k_scale.double())
    if late:   # unit scales: the key along the queries sits at +8 |q_scale . k_scale| / 64 = +8 (natural units), the one against them at -8
        _, dom, opp = late
        khat[:, :, dom] = r16(F.normalize(q[:, :, 0], dim=-1))
        khat[:, :, opp] = -khat[:, :, dom]
    vv = rnd16(B, HEADS, J, DH)
    qh = r16(q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12) * q_scale.double() * float(torch.tensor(q_mult, dtype=torch.float32)))
    s = torch.einsum("bhid,bhjd->bhij", qh, khat)      # log2 units: q_mult carries log2(e)
    if late:
        assert (s.argmax(-1) == late[1]).all() and (s.argmin(-1) == late[2]).all()
        assert (s.max(-1).values > 7.5 * ops.LOG2E).all() and (s.min(-1).values < -7.5 * ops.LOG2E).all()
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    o = r16(torch.einsum("bhij,bhjd->bhid", p, vv)).permute(0, 2, 1, 3).reshape(B, N, INNER)
    ref = ln64(r16(o @ w_out64.t()), g_o64) + x
    Jp = ops._round_up(J, 32)
    kbuf = torch.zeros(B, HEADS, Jp, DH, dtype=torch.float16)
    vbuf = torch.zeros(B, HEADS, DH, Jp, dtype=torch.float16)
    kbuf[:, :, :J] = khat.half()
    vbuf[:, :, :, :J] = vv.half().transpose(2, 3)
    kbuf, vbuf = kbuf.to(dev), vbuf.to(dev)
    k0, v0 = kbuf.cpu().clone(), vbuf.cpu().clone()
    ks, vs = (HEADS * Jp * DH, Jp * DH, DH), (HEADS * DH * Jp, DH * Jp, Jp)
    pwq, pwo = ops.pack_weight(wq, None, dev), ops.pack_weight(w_out, None, dev)
    gn, go, qs = g_n.to(dev), g_o.to(dev), q_scale.to(dev)
    assert ops.rowchain_ok(C, N, HEADS, DH, pwq, pwo)
    # the launch-per-op plan
    xa = dense(ops, x, dev)
    plan = ops.Plan("unfused")
    mu, rs = torch.empty(B * N, device=dev), torch.empty(B * N, device=dev)
    ops.rowstat(plan, xa, mode=1, rs=rs, mu=mu)
    qa = ops.new_act(B, 1, N, INNER, dev)
    ops.igemm(plan, xa, pwq, qa, mu=mu, rs=rs, pa=gn)
    oa = ops.new_act(B, 1, N, INNER, dev)
    ops.attention(plan, qa.t, kbuf, vbuf, oa.t, B=B, heads=HEADS, rows=N, J=J, q_strides=(N * INNER, DH, INNER), k_strides=ks, vt_strides=vs,
                  o_strides=(N * INNER, DH, INNER), q_scale=qs, q_mult=q_mult, head_dim=DH)
    ya = ops.new_act(B, 1, N, C, dev)
    ops.igemm(plan, oa, pwo, ya)
    outa = ops.new_act(B, 1, N, C, dev)
    ops.ln_residual(plan, ya, go, outa, res=xa)
    plan.run()
    torch.cuda.synchronize()
    # one ROWCHAIN launch (kind "stats": a second one with the statistics of the ROWSTAT launch above)
    pad = 8 if strided else 0
    xb = strided16(ops, x, C + pad, N * (C + pad), dev)
    ld_out = C + 2 * pad
    v = Verdict(f"rowchain_contract.xattn[{B}x{N}x{C} J{J} {_xa_id((B, N, C, J, kind, strided)).split('-')[4]}{' strided' if strided else ''}]")
    outs = []
    for stats in (None, (mu, rs)) if kind == "stats" else (None,):
        g_o_, outb, mask = out_buffer(ops, B, N, C, ld_out, dev)
        g_s = guarded(B * N, dev, torch.float32)
        chain = ops.Plan("chain")
        ops.rowchain_xattn(chain, xb, outb, pwq, gn, pwo, go, kbuf, vbuf, heads=HEADS, J=J, k_strides=ks, vt_strides=vs, q_scale=qs, q_mult=q_mult,
                           rows_per_batch=N, ln_stats=stats, ssq_out=g_s.t)
        chain.run()
        torch.cuda.synchronize()
        name = "out" if stats is None else "out_stats"
        got = rows_of(g_o_.cpu(), B, N, C, ld_out)
        v.rows(name, got, outa.t.reshape(B, N, C), ref)
        v.ssq(name, g_s.cpu(), got, C, False)
        v.guard(name, g_o_, mask)
        v.guard(name + ".ssq_out", g_s)
        outs.append(got)
    if len(outs) == 2:
        e = figures(outs[1], outs[0])[1]
        v.figs["stats_vs_own"] = e
        v.check("ln_stats", e < 1e-4, f"the caller's statistics and the launch's own differ by {e:.3e}")
    v.check("operands", torch.equal(kbuf.cpu(), k0) and torch.equal(vbuf.cpu(), v0), "the K^ / V^T operand buffers (their zero padding J .. Jp included) changed")
    v.done()


# ------------------------------------------------------------------------------------------------ mode 3: QKV

#             B, N,  C,   n_ctx, strided
QKV_CASES = [(2, 64, 128, 2, True),        # r0 = 3: the V^T columns start at an odd key
             (3, 32, 32, 41, False),       # one tile per image
             (2, 64, 256, 39, False)]


@pytest.mark.parametrize("stats", [False, True], ids=["own_stats", "ln_stats"])
@pytest.mark.parametrize("B,N,C,n_ctx,strided,t64", with_tiles(QKV_CASES))
def test_qkv(B, N, C, n_ctx, strided, t64, stats, monkeypatch):
    """y = fp16(fp16(LN(x) g0) [Wq | Wkv]^T); out[r, :512] = q; K^[b, r0 + n] = fp16(k / |k| k_scale); V^T[b, :, r0 + n] = v.  Columns 512 .. 639 of
    the output rows are not written (k and v leave the launch as K^ / V^T only)."""
    from imagen_pytorch_amd import ops
    dev = gpu_device()
    set_tiles(monkeypatch, ops, t64)
    torch.manual_seed(12)
    nout = INNER + 2 * DH
    x = rnd16(B, N, C)
    w, w64 = w16(nout, C)
    (g_n, g_n64) = gain(C)
    k_scale = (1 + 0.1 * torch.randn(DH)).float()
    y = r16(ln64(x, g_n64)) @ w64.t()
    kk = r16(y[..., INNER:INNER + DH])
    ref_q, ref_v = y[..., :INNER], y[..., INNER + DH:]
    ref_k = kk / kk.norm(dim=-1, keepdim=True).clamp(min=1e-12) * k_scale.double()
    pw = ops.pack_weight(w, None, dev)
    gn, ksc = g_n.to(dev), k_scale.to(dev)
    r0 = n_ctx + 1
    Jp = ops._round_up(r0 + N, 32)
    ks, vs = (Jp * DH, 0, DH), (DH * Jp, 0, Jp)
    # the launch-per-op plan
    xa = dense(ops, x, dev)
    plan = ops.Plan("unfused")
    mu, rs = torch.empty(B * N, device=dev), torch.empty(B * N, device=dev)
    ops.rowstat(plan, xa, mode=1, rs=rs, mu=mu)
    qkva = ops.new_act(B, 1, N, nout, dev, zero=True)
    ka = torch.zeros(B, Jp, DH, dtype=torch.float16, device=dev)
    va = torch.zeros(B, DH, Jp, dtype=torch.float16, device=dev)
    ops.igemm(plan, xa, pw, qkva, mu=mu, rs=rs, pa=gn)
    ops.kv_prep(plan, qkva.t, qkva.t, ksc, ka, va, B=B, heads=1, rows=N, r0=r0, src_strides=(N * nout, nout, 0), k_strides=ks, vt_strides=vs,
                k_off=INNER, v_off=INNER + DH, head_dim=DH)
    plan.run()
    torch.cuda.synchronize()
    # one ROWCHAIN launch
    pad = 8 if strided else 0
    xb = strided16(ops, x, C + pad, N * (C + pad), dev)
    ld_out = nout + pad
    g_q = guarded(B * N * ld_out, dev)
    outb = g_q.act(ops, B, N, nout, ld_out, N * ld_out)
    g_k, g_v = guarded(B * Jp * DH, dev), guarded(B * DH * Jp, dev)
    chain = ops.Plan("chain")
    ops.rowchain_qkv(chain, xb, outb, pw, gn, g_k.t, g_v.t, ksc, heads=HEADS, r0=r0, k_strides=ks, vt_strides=vs, rows_per_batch=N,
                     ln_stats=(mu, rs) if stats else None)
    chain.run()
    torch.cuda.synchronize()
    v = Verdict(f"rowchain_contract.qkv[{B}x{N}x{C} r0 {r0} tile{64 if t64 else 32} {'ln_stats' if stats else 'own stats'}{' strided' if strided else ''}]")
    kb, vb = g_k.cpu().reshape(B, Jp, DH), g_v.cpu().reshape(B, DH, Jp)
    v.rows("q", rows_of(g_q.cpu(), B, N, INNER, ld_out), qkva.t.reshape(B, N, nout)[..., :INNER], ref_q)
    v.rows("k", kb[:, r0:r0 + N], ka[:, r0:r0 + N], ref_k)
    v.rows("v", vb[:, :, r0:r0 + N].transpose(1, 2), va[:, :, r0:r0 + N].transpose(1, 2), ref_v)
    # rows in front of r0 belong to the conditioning: untouched, bit for bit (the neighbouring file's assertion, on sentinels instead of zeros)
    word = g_k.word
    v.check("khat", bool((kb[:, :r0].contiguous().view(torch.int16) == word).all()), "K^ rows in front of r0 were written")
    v.check("vt", bool((vb[:, :, :r0].contiguous().view(torch.int16) == word).all()), "V^T columns in front of r0 were written")
    mk = torch.zeros(B, Jp, DH, dtype=torch.bool)
    mk[:, r0:r0 + N] = True
    mv = torch.zeros(B, DH, Jp, dtype=torch.bool)
    mv[:, :, r0:r0 + N] = True
    v.guard("khat", g_k, mk)
    v.guard("vt", g_v, mv)
    v.guard("out (columns 512 .. 639 stay unwritten)", g_q, rows_mask(B * N * ld_out, B, N, INNER, ld_out, N * ld_out))
    v.done()


# ------------------------------------------------------------------------------------------------ mode 4: RESPREP

#            B, N,  C1,  C2, C,   prep_C2, strided
RP_CASES = [(2, 64, 64, 32, 64, 0, False),       # T = 2, wk = 4, 6 K steps: an uneven split
            (2, 64, 96, 64, 32, 8, True),        # T = 1, wk = 8, 10 K steps: uneven
            (1, 64, 256, 32, 32, 24, False),     # T = 1, wk = 8, 18 K steps: uneven
            (2, 64, 480, 32, 256, 256, False),   # the K = 512 ceiling, 8 cout tiles: no K split
            (5, 32, 96, 0, 128, 72, False),      # one tile per image, five gate rows
            (2, 64, 32, 0, 64, 0, False)]        # T = 2, 2 K steps: wk = 4 clamped to 2


@pytest.mark.parametrize("B,N,C1,C2,C,C2n,strided,t64", with_tiles(RP_CASES))
def test_resprep(B, N, C1, C2, C, C2n, strided, t64, monkeypatch):
    """out = fp16(concat(x, x2) Wres^T + bias + addend gate[b]); prep_out = fp16(silu(concat(out, prep_x2) rsqrt(max(ssq_out + wb ssq_b, 1e-24)) pa)).
    Every case with and without a gate, and with no prep request, a request over `out` alone and (prep_C2 > 0) one with the skip tensor; the
    strided case once more with a strided `out`, which request_prep refuses."""
    from imagen_pytorch_amd import ops
    dev = gpu_device()
    set_tiles(monkeypatch, ops, t64)
    torch.manual_seed(13)
    K = C1 + C2
    x, skip = rnd16(B, N, C1), (rnd16(B, N, C2, scale=1.4) if C2 else None)
    h2 = rnd16(B, N, C)
    nskip = rnd16(B, N, C2n, scale=0.8) if C2n else None
    w, w64 = w16(C, K)
    bias = (0.1 * torch.randn(C)).float()
    gate = torch.sigmoid(torch.randn(B, C)).float()
    pa_full = ((1 + 0.1 * torch.randn(C + C2n)) * math.sqrt(C + C2n)).float()
    wb = 0.5
    cat = torch.cat((x, skip), -1) if C2 else x
    pw = ops.pack_weight(w, bias, dev)
    nssq = (nskip.float() ** 2).sum(-1).reshape(-1) if C2n else None      # (fp32 values as given to the launch; the reference reads the same)
    pad = 8 if strided else 0
    xa, h2a = dense(ops, x, dev), dense(ops, h2, dev)
    ska = dense(ops, skip, dev) if C2 else None
    nska = dense(ops, nskip, dev) if C2n else None
    xb = strided16(ops, x, C1 + pad, N * (C1 + pad), dev)
    skb = strided16(ops, skip, C2 + 2 * pad, N * (C2 + 2 * pad), dev) if C2 else None
    h2b = strided16(ops, h2, C + pad, N * (C + pad), dev)
    nskb = strided16(ops, nskip, C2n + pad, N * (C2n + pad), dev) if C2n else None
    nssq_d = nssq.to(dev) if C2n else None
    ones = torch.ones(B, C, device=dev)
    v = Verdict(f"rowchain_contract.resprep[{B}x{N} {C1}+{C2}->{C}|{C2n} tile{64 if t64 else 32}{' strided' if strided else ''}]")
    variants = [(g, p, False) for g in (False, True) for p in (("none", "out", "skip") if C2n else ("none", "out"))]
    if strided:
        variants.append((True, "none", True))
    for gated, prep, strided_out in variants:
        tag = ("gate" if gated else "nogate") + "." + prep + (".ld_out" if strided_out else "")
        g64 = gate.double() if gated else torch.ones(B, C, dtype=torch.float64)
        exact = cat @ w64.t() + bias.double() + h2 * g64[:, None, :]
        mag = cat.abs() @ w64.abs().t() + bias.double().abs() + (h2 * g64[:, None, :]).abs()
        ref = r16(exact)
        c2n = C2n if prep == "skip" else 0
        pa = pa_full[:C + c2n].contiguous()
        pad_d = pa.to(dev)
        gd = gate.to(dev) if gated else None
        # the launch-per-op plan (IGEMM's gate * addend epilogue needs a gate: ones where the chain gets none)
        plan = ops.Plan("unfused")
        outa, ssq_a = ops.new_act(B, 1, N, C, dev), torch.empty(B * N, device=dev)
        opa = ops.igemm(plan, xa, pw, outa, x2=ska, addend=h2a, gate=gd if gated else ones, ssq_out=ssq_a)
        if prep != "none":
            ya = ops.new_act(B, 1, N, C + c2n, dev)
            kw = dict(x2=nska if c2n else None, ssq_b=nssq_d if c2n else None, ssq_wb=wb, pa=pad_d, act_in=ops.ACT_SILU)
            if opa.ssq_emitted:
                ops.act_prep(plan, outa, ya, ssq_a=ssq_a, **kw)
            else:
                ops.act_prep(plan, outa, ya, self_stat=True, **kw)
        plan.run()
        # one ROWCHAIN launch
        ld_out = C + 3 * pad if strided_out else C
        g_o, outb, mask = out_buffer(ops, B, N, C, ld_out, dev)
        g_s = guarded(B * N, dev, torch.float32)
        chain = ops.Plan("chain")
        p = ops.rowchain_resprep(chain, xb, skb, h2b, gd, outb, pw, rows_per_batch=N, ssq_out=g_s.t)
        g_p = None
        if strided_out:
            assert ops.request_prep(outb, None, None, wb, pad_d) is None, "request_prep takes a dense producer only"
        elif prep != "none":
            yb = ops.request_prep(outb, nskb if c2n else None, nssq_d if c2n else None, wb, pad_d)
            assert yb is not None and (yb.C, yb.ld) == (C + c2n, C + c2n) and ops.request_prep(outb, None, None, wb, pad_d) is None
            g_p = guarded(B * N * (C + c2n), dev)         # the wrapper's own allocation -> a guarded one of the same layout
            p.prep_out = g_p.act(ops, B, N, C + c2n).ptr
        assert bool(p.prep_out) == (g_p is not None)
        chain.run()
        torch.cuda.synchronize()
        got = rows_of(g_o.cpu(), B, N, C, ld_out)
        v.rows(tag + ".out", got, outa.t.reshape(B, N, C), exact)
        el = ((got.double() - exact).abs() / (ulp16(exact) + (K + 4) * ULP32 * mag)).reshape(-1)
        el = float(torch.nan_to_num(el, nan=float("inf")).max())
        v.figs[tag + ".out_elem"] = el
        v.check(tag + ".out", el <= 1.0, f"an element is {el:.2f} x its bound ulp16 + (K + 4) ulp32 sum|terms| from the exact value")
        v.ssq(tag + ".out", g_s.cpu(), got, C, t64)
        v.guard(tag + ".out", g_o, mask)
        v.guard(tag + ".ssq_out", g_s)
        if g_p is not None:
            tot = (ref ** 2).sum(-1) + (wb * nssq.double().reshape(B, N) if c2n else 0.0)
            z = (torch.cat((ref, nskip), -1) if c2n else ref) * torch.rsqrt(tot.clamp(min=1e-24))[..., None] * pa.double()
            ref_y = z * torch.sigmoid(z)
            v.rows(tag + ".prep", g_p.cpu().reshape(B, N, C + c2n), ya.t.reshape(B, N, C + c2n), ref_y)
            v.guard(tag + ".prep_out", g_p)
    v.done()
