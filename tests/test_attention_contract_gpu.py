"""The spatial attention of csrc/attention.hip — the 4-wave kernel with 32-key tiles at head dim 64 and 32 (`k64`, `k32`), the 8-wave online kernel
with 64-key tiles (`w8`, SUB = 1 up to 128 keys and 2 above) and the bounded-logit ring pipeline (`bnd`) — per ELEMENT against an fp64 restatement
of ATTENTION's contract (include/imagen_hip.h), every tiling selected through ops.attention exactly as the engine selects it.

Reference.  The contract takes q^, K^ and V^T as given fp16 operands, so the reference reads back the device's own fp16 q^ (the buffer after the
QNORM op), K^ and V^T (after KV_PREP; tests/test_elementwise_kernels_gpu.py holds those two ops to fp64) and evaluates
    o_d = sum_j 2^(q^ . k^_j) v_jd / sum_j 2^(q^ . k^_j),   j < J
in fp64, the row maximum subtracted in fp64 and the last fp16 rounding NOT applied (the stance of tests/test_rowchain_contract_gpu.py: against
the unrounded value every element carries its own half ulp, and a fault moves it from under to over that).

Per-element bound, derived and not measured.  p_j the exact weights scaled to max_j p_j = 1, l = sum_j p_j, a_d = sum_j p_j |v_jd| / l,
delta = (D + 4) ulp32 max_j sum_d |q^_d k^_jd| (the fp32 contraction of one logit: D products added in any order on the matrix pipe):
    |got - ref| <= 1/2 ulp16(binade of ref or of got, whichever is larger) (1 + 2^-10)         the fp16 store
                 + (rho + (J + 8) ulp32 + 2 ln2 delta) a_d                                      P's format, the fp32 sums, the logits (numerator and denominator)
                 + sigma
rho = 2^-11 for w8 and bnd (P enters the PV product as ONE fp16), 2^-21 for the 4-wave kernels (an fp16 hi + lo pair); sigma = J 2^-25 max_j |v_jd| / l
for the online kernels (weights below 2^-14 of the running maximum go subnormal in fp16: 2^-25 absolute each), 0 for bnd (logit_bound <= 14 keeps
every weight normal).  One dropped key is tens to hundreds of times over this bound; a failure is a finding.

What a case asserts (everything is measured and recorded first, then asserted: `Verdict`):
 * every element of every row within the bound, none left out; no NaN;
 * the whole-tensor figure under the project's bar ATTN_TOL_BOUNDED = 1e-3 (the worst row's relative error is recorded with it);
 * `o` lies in a `guarded` allocation: the sentinels around it and in the gaps of its strided rows survive;
 * q^ / the raw q of a fused launch, K^ and V^T are bit for bit what they were before the launch;
 * pa.softmax_mode is the expected one, and the launch took the tiling the case is named after (rows, head dim and bound decide).
K^ and V^T are `guarded` allocations of exactly Jp = round_up(J, 32) keys, keys [J, Jp) zero as the contract says, NaN (the sentinel) behind them;
the `shared` layout also leaves 8 NaN columns behind every V^T row (vt_ds = Jp + 8).  The gaps of strided q rows hold NaN.  A read of V^T past Jp
multiplies a NaN into the row and fails it.  A read of K^ past Jp is NOT visible this way: the kernels overwrite the logits of keys >= J with
-1e30 whatever they were, so only the allocation's bounds protect it (the 64-key tilings redirect those loads: `kk` of one_load / load_item).

Layouts (each on every tiling with B = 2 in test_layouts; the sweeps rotate through them with fewer heads):
 * self: the engine's self-attention site — 8 query heads over ONE k / v head (k_hs = vt_hs = 0), q rows inside the wider q | k | v buffer
   (q_rs = inner + 2 dh), o dense, the keys written by KV_PREP at r0 = 3 behind context rows written by another KV_PREP launch;
 * cross: the engine's cross-attention site — per-head K^ and V^T, dense q and o rows;
 * shared: heads = 1 and rows = 8 n over one key set (the form the kernel's header describes), q_rs = D + 8, o_rs = D + 4 (the smallest
   alignment the stores take), vt_ds = Jp + 8.
Fused QNORM: test_fused_qnorm.  The fused q load and the QNORM op evaluate (f16)((float)q * inv * g) with the same expression, but NOT the same
sum of squares: QNORM adds 8 dims per lane and then a butterfly over 8 (4) lanes, the attention kernels 32 (16) dims per lane and one exchange.
The squares of fp16 values are exact in fp32, their sums round, so `inv` may differ in the last bit and flip the fp16 rounding of a q^ element.
On q drawn from a 2^-5 grid every partial sum is exact in either order and the two outputs are asserted bit for bit equal; on random q the fused
rows are held to the same per-element bound against the reference built from the QNORM op's q^ and the number of differing elements is recorded:
of 65 792 elements (2 x 2 x 257 x 64) 101 differ on w8 and 193 on bnd on MI355X (100 and 193 on the emulation), every one within the bound (worst
0.48 of it); none of the 8 448 elements of the 33-row cases of the 4-wave kernels differ.  The raw q buffer of a fused launch is unchanged.

Runs on MI355X (-m gpu) and on the CPU emulation (IMAGEN_EMUL_TESTS=1; tests/test_igemm_emulated.py keeps the whole file in the CPU suite: no
case is hardware-only)."""
import math

import pytest
import torch

from conftest import gpu_device, record_parity
from test_elementwise_kernels_gpu import ULP32, guarded, rows_mask, strided16, ulp16

pytestmark = pytest.mark.gpu

ATTN_TOL_BOUNDED = 1e-3     # the project's bar on the whole-tensor figure (tests/test_kernels_gpu.py)
LN2 = math.log(2.0)
TILINGS = ("k64", "k32", "w8", "bnd")
RHO = {"k64": 2.0 ** -21, "k32": 2.0 ** -21, "w8": 2.0 ** -11, "bnd": 2.0 ** -11}

#           shared k / v head, columns beside the q heads of a row (in head dims / elements), beside an o row, beside a V^T row, key offset of KV_PREP
LAYOUTS = {"self": dict(kv_shared=True, qpad_heads=2, qpad=0, opad=0, vpad=0, r0=3),
           "cross": dict(kv_shared=False, qpad_heads=0, qpad=0, opad=0, vpad=0, r0=0),
           "shared": dict(kv_shared=True, qpad_heads=0, qpad=8, opad=4, vpad=8, r0=0)}


def tiling_of(D, rows, mode):
    """The kernel launch_attention takes (csrc/attention.hip)."""
    if D == 32:
        return "k32"
    if rows < 256:
        return "k64"
    return "bnd" if mode == 1 else "w8"


# ------------------------------------------------------------------------------------------------ inputs

def scales(tiling, kind, D, g):
    """(q_scale, k_scale).  bnd: spread 0.04 around the init value, clamped so that the bound stays under 14; online kernels: spread 0.2 with one
    dim at 1.25 x 1.25, which alone puts the bound over 14; kind `edge`: every dim at sqrt(1.18): attention_logit_bound = 13.8, in (13.5, 14]."""
    if kind[0] == "edge":
        c = math.sqrt(1.18)
        return torch.full((D,), c), torch.full((D,), c)
    if tiling == "bnd":
        return ((1 + 0.04 * torch.randn(D, generator=g)).clamp(0.9, 1.09), (1 + 0.04 * torch.randn(D, generator=g)).clamp(0.9, 1.09))
    qs, ks = 1 + 0.2 * torch.randn(D, generator=g), 1 + 0.2 * torch.randn(D, generator=g)
    qs[0] = ks[0] = 1.25
    return qs, ks


def inputs(kind, B, H, Hk, rows, J, D, g):
    """Raw q [B, H, rows, D], k and v [B, Hk, J, D] as fp16-representable fp32.  kind:
    ("rand",)            normal draws;
    ("grid",)            q on a 2^-5 grid (sums of its squares are exact in fp32 in any order);
    ("edge", par, anti)  even query rows parallel to key `par`, key `anti` = -key `par`: logits at + and - 13.6 with the `edge` scales;
    ("wave",)            rows 0 .. 31 alternate between a maximum at key 0 (even rows) and at key J - 1 (odd rows); of rows 32 .. 63 only
                         row 40 and of rows 64 .. 95 only row 95 find theirs at key J - 1, the rest at key 0; rows from 96 on are random.
                         Key J - 1 is opposite to key 0 and every key between them close to key 0, so that a late maximum lies more than
                         17 above everything its row met before: a softmax is invariant under a shift, and a rescale that is skipped shows
                         only when the weight 2^(s - stale maximum) leaves the fp16 range (2^16);
    ("flat",)            row 0 is zero (all logits equal: o = mean of v), row 1 parallel to key min(5, J - 1), the rest random."""
    h = lambda t: t.half().float()
    q = h(torch.randn(B, H, rows, D, generator=g) * 2)
    k = h(torch.randn(B, Hk, J, D, generator=g))
    v = h(torch.randn(B, Hk, J, D, generator=g))
    along = lambda j: k[:, :, j].expand(B, H, D)          # (a shared k / v head serves every query head)
    length = lambda *s: 1 + torch.rand(*s, generator=g)
    if kind[0] == "grid":
        q = (torch.randint(-64, 65, (B, H, rows, D), generator=g) / 32.0).float()
    elif kind[0] == "edge":
        _, par, anti = kind
        k[:, :, anti] = -k[:, :, par]
        q[:, :, 0::2] = h(along(par)[:, :, None, :] * length(B, H, (rows + 1) // 2, 1))
    elif kind[0] == "wave":
        late = torch.zeros(rows, dtype=torch.bool)
        late[1:32:2] = True
        late[[40, 95]] = True
        n = min(rows, 96)
        k[:, :, 1:J - 1] = h(k[:, :, :1] + 0.5 * k[:, :, 1:J - 1])      # every key between the two within ~27 degrees of key 0,
        k[:, :, J - 1] = -k[:, :, 0]                                  # the last one opposite to it
        q[:, :, :n] = h(torch.where(late[:n, None], along(J - 1)[:, :, None, :], along(0)[:, :, None, :]) * length(B, H, n, 1))
    elif kind[0] == "flat":
        q[:, :, 0] = 0.0
        q[:, :, 1] = h(along(min(5, J - 1)) * 1.5)
    return q, k, v


# ------------------------------------------------------------------------------------------------ reference and bound

def reference(qh, kh, vt, J, D, rho, online):
    """fp64 (o, bound without the store term) from q^ [B, H, R, D], K^ [B, Hk, Jp, D], V^T [B, Hk, D, Jp] as the device holds them."""
    B, H, R, _ = qh.shape
    k = kh[:, :, :J].double().expand(B, H, J, D)
    v = vt[:, :, :, :J].double().transpose(2, 3).expand(B, H, J, D)
    q = qh.double()
    s = torch.einsum("bhid,bhjd->bhij", q, k)
    mag = torch.einsum("bhid,bhjd->bhij", q.abs(), k.abs()).amax(-1)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhij,bhjd->bhid", p, v) / l
    a = torch.einsum("bhij,bhjd->bhid", p, v.abs()) / l
    delta = (D + 4) * ULP32 * mag[..., None]
    bound = (rho + (J + 8) * ULP32 + 2 * LN2 * delta) * a
    if online:
        bound = bound + J * 2.0 ** -25 * v.abs().amax(2)[:, :, None, :] / l
    return o, bound, s


class Verdict:
    """The figures and failures of one case: everything is measured and recorded before anything is asserted."""

    def __init__(self, test_id):
        self.id, self.figs, self.fail = test_id, {}, []

    def elements(self, name, got, ref, lin):
        got = got.double()
        bound = 0.5 * torch.maximum(ulp16(ref), ulp16(torch.nan_to_num(got))) * (1 + 2.0 ** -10) + lin
        share = torch.nan_to_num((got - ref).abs() / bound, nan=float("inf"))
        d = torch.nan_to_num(got - ref, nan=float("inf"))
        row = d.norm(dim=-1) / ref.norm(dim=-1).clamp(min=1e-300)
        nan = int(torch.isnan(got).sum())
        worst = float(share.max())
        self.figs.update({f"{name}.elem_share": worst, f"{name}.row": float(row.max()), f"{name}.all": float(d.norm() / ref.norm()), f"{name}.nan": float(nan)})
        if nan:
            self.fail.append(f"{name}: {nan} NaN elements")
        if not worst <= 1.0:
            i = [int(x) for x in (share == share.max()).nonzero()[0]]
            self.fail.append(f"{name}: element (b, h, row, d) = {i} is at {worst:.3g} of its bound; {int((share > 1).sum())} elements of {int((share > 1).any(-1).sum())} rows are over")
        if not self.figs[f"{name}.all"] < ATTN_TOL_BOUNDED:
            self.fail.append(f"{name}: whole-tensor figure {self.figs[name + '.all']:.3e} >= {ATTN_TOL_BOUNDED}")

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


# ------------------------------------------------------------------------------------------------ one case

def bits(t):
    return t.contiguous().view(torch.int16)


def run_case(tiling, layout, B, H, rows, J, kind=("rand",), fused=False, seed=0):
    from imagen_pytorch_amd import ops
    dev = gpu_device()
    L = LAYOUTS[layout]
    D = 32 if tiling == "k32" else 64
    H = 1 if layout == "shared" else H
    Hk = 1 if L["kv_shared"] else H
    g = torch.Generator().manual_seed(7000 + 131 * seed + J + 7 * rows)
    qs, ks = scales(tiling, kind, D, g)
    q, k, v = inputs(kind, B, H, Hk, rows, J, D, g)
    q_mult = 8.0 * ops.LOG2E
    logit_bound = ops.attention_logit_bound(qs, ks, q_mult)
    if kind[0] == "edge":
        assert 13.5 < logit_bound <= 14.0
    given = None if tiling == "w8" and logit_bound <= ops.ATTN_BOUND_MAX else logit_bound    # (w8 on logits that bnd would take: a plan without a bound)
    mode = int(given is not None and given <= ops.ATTN_BOUND_MAX)
    vd = Verdict(f"attention_contract.{tiling}[{layout} B{B} H{H} rows{rows} J{J} {'-'.join(str(x) for x in kind)}{' fused' if fused else ''}]")
    vd.check("tiling", tiling_of(D, rows, mode) == tiling, f"the launch takes {tiling_of(D, rows, mode)} (rows {rows}, head dim {D}, bound {logit_bound:.2f})")
    # q rows [B, rows, H * D] inside rows of ldq elements, NaN beside them; o rows of ldo elements in a guarded allocation
    ldq, ldo = (H + L["qpad_heads"]) * D + L["qpad"], H * D + L["opad"]
    q_rows = q.permute(0, 2, 1, 3).reshape(B, rows, H * D)
    qa = strided16(ops, q_rows, ldq, rows * ldq, dev)
    q_st, o_st = (rows * ldq, D, ldq), (rows * ldo, D, ldo)
    # K^ [B, Hk, Jp, D] and V^T [B, Hk, D, vds]: exactly Jp keys, zero where KV_PREP does not write, the sentinel (a NaN) everywhere else
    Jp = ops._round_up(J, 32)
    vds = Jp + L["vpad"]
    g_k, g_v = guarded(B * Hk * Jp * D, dev), guarded(B * Hk * D * vds, dev)
    g_k.t.zero_()
    v_mask = rows_mask(g_v.numel, 1, B * Hk * D, Jp, vds, 0)
    v_init = g_v.cpu()
    v_init[v_mask] = 0.0
    g_v.t.copy_(v_init.to(dev))
    kp_k, kp_v = (Hk * Jp * D, Jp * D, D), (Hk * D * vds, D * vds, vds)
    k_st = (kp_k[0], 0 if layout == "self" else kp_k[1], D)
    v_st = (kp_v[0], 0 if layout == "self" else kp_v[1], vds)
    qs_d, ks_d = qs.to(dev), ks.to(dev)
    prep = ops.Plan("prep")
    ops.qnorm(prep, qa.t, qs_d, rows=B * rows, heads=H, ld=ldq, mult=q_mult, head_dim=D)
    r0 = min(L["r0"], J - 1)
    W = 2 * Hk * D
    src = torch.cat((k.permute(0, 2, 1, 3).reshape(B, J, Hk * D), v.permute(0, 2, 1, 3).reshape(B, J, Hk * D)), -1).half()
    for lo, hi in ((0, r0), (r0, J)):       # the context rows, then the keys behind them
        if hi > lo:
            part = src[:, lo:hi].contiguous().to(dev)
            ops.kv_prep(prep, part, part, ks_d, g_k.t, g_v.t, B=B, heads=Hk, rows=hi - lo, r0=lo, src_strides=((hi - lo) * W, W, D), k_strides=kp_k,
                        vt_strides=kp_v, k_off=0, v_off=Hk * D, head_dim=D)
    prep.run()
    torch.cuda.synchronize()
    qh_flat, k_dev, v_dev = qa.t.cpu().clone(), g_k.cpu(), g_v.cpu()
    qh = qh_flat.as_strided((B, H, rows, D), (rows * ldq, D, ldq, 1))
    kh = k_dev.view(B, Hk, Jp, D)
    vt = v_dev.as_strided((B, Hk, D, Jp), (Hk * D * vds, D * vds, vds, 1))
    vd.check("padding", bool((kh[:, :, J:] == 0).all() and (vt[..., J:] == 0).all() and torch.isfinite(kh).all() and torch.isfinite(vt).all()),
             "keys [J, Jp) of K^ / V^T are not zero")
    ref, lin, s = reference(qh, kh, vt, J, D, RHO[tiling], tiling != "bnd")
    if kind[0] == "edge":
        _, par, anti = kind
        even = s[:, :, 0::2]
        vd.check("inputs", bool((even.argmax(-1) == par).all() and (even.argmin(-1) == anti).all() and (even.amax(-1) > 13.5).all() and (even.amin(-1) < -13.5).all()
                                and (s.abs().amax() <= logit_bound)), "the extreme logits are not where the case puts them")
    if kind[0] == "wave":
        late = torch.zeros(min(rows, 96), dtype=torch.bool)
        late[1:32:2] = True
        late[[40, 95]] = True
        sw = s[:, :, :late.numel()]
        vd.check("inputs", bool((sw.argmax(-1) == torch.where(late, J - 1, 0)).all() and (sw[:, :, late, J - 1] - sw[:, :, late, :J - 1].amax(-1) > 17).all()),
                 "the row maxima are not where the case puts them, or a late one is less than 17 above the keys before it")
    if kind[0] == "flat":
        vd.check("inputs", bool((s[:, :, 0] == 0).all() and (s[:, :, 1].argmax(-1) == min(5, J - 1)).all()), "row 0 / row 1 are not flat / dominated")

    def launch(q_t, **kw):
        g_o = guarded(B * rows * ldo, dev)
        plan = ops.Plan("attention")
        pa = ops.attention(plan, q_t, g_k.t, g_v.t, g_o.t, B=B, heads=H, rows=rows, J=J, q_strides=q_st, k_strides=k_st, vt_strides=v_st, o_strides=o_st,
                           head_dim=D, logit_bound=given, **kw)
        plan.run()
        torch.cuda.synchronize()
        return pa, g_o, g_o.cpu().as_strided((B, H, rows, D), (rows * ldo, D, ldo, 1))

    o_mask = rows_mask(B * rows * ldo, B, rows, H * D, ldo, rows * ldo)
    pa, g_o, got = launch(qa.t)
    vd.check("softmax_mode", pa.softmax_mode == mode, f"softmax_mode {pa.softmax_mode}, expected {mode} at bound {logit_bound:.2f}")
    vd.elements("o", got, ref, lin)
    vd.guard("o", g_o, o_mask)
    vd.check("operands", torch.equal(bits(qa.t.cpu()), bits(qh_flat)), "the q^ buffer changed")
    if fused:
        raw = strided16(ops, q_rows, ldq, rows * ldq, dev)
        raw0 = raw.t.cpu().clone()
        paf, g_f, got_f = launch(raw.t, q_scale=qs_d, q_mult=q_mult)
        vd.check("softmax_mode", paf.softmax_mode == mode, f"fused: softmax_mode {paf.softmax_mode}, expected {mode}")
        vd.elements("fused", got_f, ref, lin)
        vd.guard("fused", g_f, o_mask)
        differ = int((bits(got_f) != bits(got)).sum())
        vd.figs["fused.differs"] = float(differ)
        if kind[0] == "grid":
            vd.check("fused", differ == 0, f"{differ} elements differ from the unfused launch although the sums of squares are exact")
        vd.check("fused", torch.equal(bits(raw.t.cpu()), bits(raw0)), "the fused launch changed the raw q buffer")
    vd.check("operands", torch.equal(bits(g_k.cpu()), bits(k_dev)) and torch.equal(bits(g_v.cpu()), bits(v_dev)), "the K^ / V^T buffers changed")
    vd.guard("khat", g_k, torch.ones(g_k.numel, dtype=torch.bool))
    vd.guard("vt", g_v, v_mask)
    vd.done()


# ------------------------------------------------------------------------------------------------ cases

KEYS64 = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 193, 257, 321, 449]     # 1 .. 7 tiles of 64; Jpad ends mid-tile at 96 and 160
ROWS64 = [256, 257, 300, 385, 513]      # 257: one valid row in the last workgroup of w8 (256 rows) and bnd (128); 385: of bnd only
KEYS32 = [1, 31, 32, 33, 64, 65, 292]
ROWS4 = [1, 31, 33, 128, 129, 255]
NAMES = ("cross", "self", "shared")


def _ids(cases):
    return [pytest.param(*c, id="-".join("_".join(str(y) for y in x) if isinstance(x, tuple) else str(x) for x in c)) for c in cases]


#              tiling, layout, B, H, rows, J
KEY_CASES = [(t, NAMES[i % 3], 2 if NAMES[i % 3] == "shared" else 1, 2, ROWS64[(i + n) % 5], J) for i, J in enumerate(KEYS64) for n, t in enumerate(("w8", "bnd"))] + [
    (t, NAMES[(i + 1) % 3], 2 if NAMES[(i + 1) % 3] == "shared" else 1, 2, ROWS4[(i + 3 * n) % 6], J) for i, J in enumerate(KEYS32) for n, t in enumerate(("k64", "k32"))] + [
    ("k32", "cross", 1, 2, 256, 65), ("k32", "self", 1, 2, 513, 292)]       # head dim 32 keeps the 4-wave kernel at any row count


@pytest.mark.parametrize("tiling,layout,B,H,rows,J", _ids(KEY_CASES))
def test_key_counts(tiling, layout, B, H, rows, J):
    """Every key count at which a tiling changes its path: one key, one short of / exactly / one past a tile, a Jpad that ends in the middle of a
    64-key tile, odd and even tile counts for SUB = 2, two wraps of bnd's ring of four slots with both parities of its non-last iterations."""
    run_case(tiling, layout, B, H, rows, J, seed=1)


ROW_CASES = [(t, NAMES[i % 3], 2, 2, r, (33, 97)[(i + n) % 2]) for i, r in enumerate(ROWS4) for n, t in enumerate(("k64", "k32"))] + [
    (t, NAMES[i % 3], 2, 2, r, (97, 193, 321)[(i + n) % 3]) for i, r in enumerate(ROWS64) for n, t in enumerate(("w8", "bnd"))]


@pytest.mark.parametrize("tiling,layout,B,H,rows,J", _ids(ROW_CASES))
def test_row_counts(tiling, layout, B, H, rows, J):
    """One row, one short of / one past a wave and a workgroup, 255 | 256 | 257 rows where the launcher switches tilings, one valid row in the last
    workgroup (the other rows of its waves are clamped to it and must not be stored)."""
    run_case(tiling, layout, B, H, rows, J, seed=2)


@pytest.mark.parametrize("layout", NAMES)
@pytest.mark.parametrize("tiling", TILINGS)
def test_layouts(tiling, layout):
    """The three layouts of the module docstring with the engine's head counts and two images, so that every batch and head stride matters."""
    big = tiling in ("w8", "bnd")
    rows = (264 if big else 72) if layout == "shared" else (257 if big else 33)
    run_case(tiling, layout, 2, 8, rows, 97, seed=3)


@pytest.mark.parametrize("kind", ["grid", "rand"])
@pytest.mark.parametrize("tiling", TILINGS)
def test_fused_qnorm(tiling, kind):
    """QNORM fused into the q load on strided q rows (the self layout) against the QNORM op + the same launch: see the module docstring."""
    run_case(tiling, "self", 2, 2, 257 if tiling in ("w8", "bnd") else 33, 65, kind=(kind,), fused=True, seed=4)


@pytest.mark.parametrize("par,anti", [(0, 63), (63, 96), (96, 0)])
@pytest.mark.parametrize("tiling", TILINGS)
def test_logits_at_the_bound(tiling, par, anti):
    """Stress a: attention_logit_bound = 13.8, in (13.5, 14] (the 14.0 the fp16 range argument of bnd rests on), half the queries parallel to one key
    and antiparallel to another, placed at key 0, at the last key of a full tile (63) and at key J - 1 = 96 of the ragged last tile: the weight
    of the antiparallel key is about 2^-13.6 before the division in bnd and 2^-27 of the maximum (flushed to zero: sigma) in the online kernels.
    The 4-wave kernels get softmax_mode 1 too and ignore it."""
    run_case(tiling, "cross", 1, 2, 257 if tiling in ("w8", "bnd") else 129, 97, kind=("edge", par, anti), seed=5)


@pytest.mark.parametrize("tiling", ["k64", "k32", "w8"])
def test_late_maximum_in_some_rows_of_a_wave(tiling):
    """Stress b: w8 rescales its accumulators only when SOME row of the wave meets a new maximum (`__any(m_new > m_run)`), with the factor of each
    row: a wave whose rows alternate between a maximum in the first and in the last tile, one in which a single row (lane 8) and one in which
    the last row (lane 31) meets it late, more than 17 above what the row met before (a skipped rescale is otherwise invisible: see `inputs`).
    (Lanes l and l + 32 hold the same row, half of its keys each, and the same m_new after their exchange.)"""
    run_case(tiling, "cross", 1, 2, 256 if tiling == "w8" else 128, 193 if tiling == "w8" else 97, kind=("wave",), seed=6)


@pytest.mark.parametrize("tiling", ["k64", "k32", "w8"])
def test_flat_and_dominated_rows(tiling):
    """Stress c: a row whose logits are all equal (a zero query: o is the mean of v) and a row with one dominating key, at scale spread 0.2: the
    bound exceeds 14 and the launch takes softmax_mode 0."""
    run_case(tiling, "cross", 1, 2, 256 if tiling == "w8" else 64, 97, kind=("flat",), seed=7)


# ------------------------------------------------------------------------------------------------ launcher

def _valid(ops, dev, plan, **over):
    """A valid launch on allocations large enough for it (B 2, heads 2, 4 rows, J 5, head dim 64); `over`: params fields overwritten afterwards."""
    B, H, rows, J, D, Jp = 2, 2, 4, 5, 64, 32
    z = lambda n: torch.zeros(n, dtype=torch.float16, device=dev)
    t = dict(q=z(B * rows * H * D + 64), k=z(B * H * Jp * D + 64), vt=z(B * H * D * Jp + 64), o=z(B * rows * H * D + 64), qs=torch.ones(D + 16, device=dev))
    p = ops.attention(plan, t["q"], t["k"], t["vt"], t["o"], B=B, heads=H, rows=rows, J=J, q_strides=(rows * H * D, D, H * D), k_strides=(H * Jp * D, Jp * D, D),
                      vt_strides=(H * D * Jp, D * Jp, Jp), o_strides=(rows * H * D, D, H * D), q_scale=t["qs"], q_mult=1.0, head_dim=D)
    for name, val in over.items():
        setattr(p, name, val(p) if callable(val) else val)
    return p


_off = lambda field, nbytes: (lambda p: getattr(p, field) + nbytes)
#            name -> (params fields overwritten, the field the message must name)
REFUSALS = {"q_bs": dict(q_bs=_off("q_bs", 4)), "q_hs": dict(q_hs=68), "k_bs": dict(k_bs=_off("k_bs", 4)), "k_hs": dict(k_hs=4), "vt_bs": dict(vt_bs=_off("vt_bs", 4)),
            "vt_hs": dict(vt_hs=_off("vt_hs", 4)), "o_bs": dict(o_bs=_off("o_bs", 2)), "o_hs": dict(o_hs=66), "q": dict(q=_off("q", 8)), "k": dict(k=_off("k", 8)),
            "vt": dict(vt=_off("vt", 8)), "o": dict(o=_off("o", 4)), "q_scale": dict(q_scale=_off("q_scale", 8)), "null_q": dict(q=None), "null_k": dict(k=None),
            "null_vt": dict(vt=None), "null_o": dict(o=None), "vt_ds": dict(vt_ds=24, J=25)}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_launcher_refuses(name):
    """launch_attention refuses what no access of the kernels takes — batch and head strides that break the 16-byte loads (q, K^, V^T) or the 8-byte
    stores (o), misaligned or null operands, a q_scale the float4 loads cannot take, V^T rows shorter than round_up(J, 32) keys — on the host,
    with a message that names the field; nothing is launched."""
    from imagen_pytorch_amd import ops
    from imagen_pytorch_amd._abi import ImagenHipError
    dev = gpu_device()
    plan = ops.Plan()
    _valid(ops, dev, plan, **REFUSALS[name])
    with pytest.raises(ImagenHipError) as e:
        plan.run()
    torch.cuda.synchronize()
    fragment = "attention: null pointer" if name.startswith("null") else f"attention: {name} = "
    assert fragment in str(e.value), str(e.value)


def test_launcher_takes_the_engines_strides():
    """The stride triples of the engine's three call sites (engine.py: self attention with k_hs = vt_hs = 0 and q inside the q | k | v rows, cross
    attention, the Perceiver pooling) at head dims 64 and 32, and the valid form of the refusals above, pass the launcher's checks."""
    from imagen_pytorch_amd import ops
    dev = gpu_device()
    plan = ops.Plan()
    _valid(ops, dev, plan)
    R, heads, N, J = 2, 8, 4, 7
    Jp = ops._round_up(J, 32)
    for dh in (64, 32):
        inner, ld = heads * dh, heads * dh + 2 * dh
        z = lambda *s: torch.zeros(*s, dtype=torch.float16, device=dev)
        qsc = torch.ones(dh, device=dev)
        kw = dict(B=R, heads=heads, rows=N, J=J, o_strides=(N * inner, dh, inner), q_scale=qsc, q_mult=8 * ops.LOG2E, head_dim=dh, logit_bound=11.7)
        ops.attention(plan, z(R, N, ld), z(R, Jp, dh), z(R, dh, Jp), z(R, N, inner), q_strides=(N * ld, dh, ld), k_strides=(Jp * dh, 0, dh), vt_strides=(dh * Jp, 0, Jp), **kw)
        ops.attention(plan, z(R, N, inner), z(R, heads, Jp, dh), z(R, heads, dh, Jp), z(R, N, inner), q_strides=(N * inner, dh, inner),
                      k_strides=(heads * Jp * dh, Jp * dh, dh), vt_strides=(heads * dh * Jp, dh * Jp, Jp), **kw)
    assert len(plan) == 5
    plan.run()
    torch.cuda.synchronize()
