"""Test infrastructure: one IGEMM launch on a forced kernel family against an fp64 restatement of the IGEMM block of include/imagen_hip.h, on
strided operands in guarded allocations, with the launch-per-op plan of the same operation beside it.  Same role as tests/igemm_case.py (which
stays as it is, whole-tensor and fp32); used by tests/test_conv_contract_gpu.py.

    in(p, c)  = concat(x1, x2)
    a(p, c)   = fp16(act_in((in - mu[p]) * rs[p] * pa[b, c] + ps[b, c])), 0 outside the image;  a = in where there is no prologue at all
    acc       = conv(a, W, stride, pad)
    v         = act_out(acc + bias);  v += addend * gate[b, c]  |  v += res
    y         = v (NHWC fp16 | pixel-shuffle | NCHW fp32);  ssq_out = sum_c fp16(v)^2
    post:       y = silu(v / max(||v||, 1e-12) * post_pa[b, c] + post_ps[b, c])
    gca:        part[b][tile] = (m, sum_q exp(l_q - m), sum_q exp(l_q - m) fp16(v)[q, :]),  l_q = fp16(v)[q, :] . wk + bk,  m = max_q l_q

Inputs and weights are fp16-representable (what pack_weight stores), gains / shifts / statistics fp32 values; the reference computes in fp64 and
rounds to fp16 exactly where the kernels must: `a`, the operand of the matrix pipe (every family writes it to LDS or registers as fp16), and
fp16(v) inside ssq_out and the GlobalContext logits (both are statistics of the STORED tensor: they are checked against the fp16 rows the
launch stored, so the rounding is the kernel's own).

The final fp16 rounding of y is left out, as in tests/test_rowchain_contract_gpu.py: against the rounded value the error of a pixel is the
count of its channels that landed on the other fp16 neighbour — zero for most pixels of a correct launch, one ulp of one channel for a few — so
that the worst pixel of two correct plans differs by whichever channel happened to flip.  Against the unrounded value every element carries its
own rounding error of up to half an ulp, the same for both plans, and a flip moves it from just under to just over that.

Operands: every input (x1, x2, addend, res) comes through `strided16` with a pixel pitch, an image pitch and a lead of its own and NaN in the gaps;
every output (y in the three output modes, ssq_out, gca_part) lies in a `guarded` allocation.  gca_part is allocated inside ops.igemm: the
pointer of the params struct is rewritten to a guarded buffer of the same layout.

Figures of a launch (`Verdict`, everything recorded before anything is asserted): the worst per-pixel relative error over the Cout channels of a
pixel, the whole-tensor figure, the share of the per-element bound used (where the contract has no intermediate rounding), ssq_out per pixel
against the sum of squares of the stored fp16 row, the GlobalContext partials per tile row, sentinel survival."""
import math

import torch
import torch.nn.functional as F

from conftest import record_parity
from test_elementwise_kernels_gpu import U, ULP32, guarded, rows_mask, strided16, sum_bound, ulp16

TOL = 1e-3     # the project's per-op bar on the whole-tensor figure (tests/test_igemm_cfgs_gpu.py)
WB = 0.5       # weight of ssq_b

DEFAULTS = dict(B=2, H=8, W=8, C1=32, C2=0, Cout=32, K=3, stride=1, pad=None, G=None,
                prologue="none",    # none | rs | ssq | ln
                affine=True,        # per-(batch, channel) pa / ps at a pitch of `pstride` floats; False: one shared gain, no shift
                pstride_extra=0,    # pstride = Cin_pad + this
                act_in="none", act_out="none", epilogue="plain",   # plain | post | addend | res | shuffle | nchw
                ssq_out=False, gca=False, bias=True, seed=0,
                # layouts (elements): pixel pitch = C + ld, image pitch = pixels * pitch + bs, first element at `lead`
                x1_l=(8, 64, 8), x2_l=(24, 16, 16), add_l=(8, 8, 8), res_l=(16, 24, 8), y_l=(32, 64, 16))

SUMMARY = {}   # family -> worst figures over the cases run (written as one parity record per family by the test module)


def r16(t):
    return t.to(torch.float16).double()


def silu64(v):
    return v * torch.sigmoid(v)


def gelu64(v):
    return 0.5 * v * torch.erfc(-v / math.sqrt(2.0))


ACT64 = dict(none=lambda v: v, silu=silu64, gelu=gelu64)


def figures(got, ref):
    """(worst per-pixel relative error, whole-tensor relative error) of rows [..., C] in fp64; a NaN (an unwritten sentinel) counts as inf."""
    got, ref = got.detach().cpu().double(), ref.double()
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    d = got - ref
    e = torch.nan_to_num(d.norm(dim=-1) / ref.norm(dim=-1).clamp(min=1e-300), nan=float("inf"))
    return float(e.max()), float(torch.nan_to_num(d.norm() / ref.norm(), nan=float("inf")))


class Verdict:
    """The figures and failures of one test: everything is measured and recorded before anything is asserted."""

    def __init__(self, test_id, fam):
        self.id, self.fam, self.figs, self.fail = test_id, fam, {}, []

    def worst(self, key, val):
        s = SUMMARY.setdefault(self.fam, {"cases": 0})
        s[key] = max(s.get(key, 0.0), val)

    def check(self, name, ok, msg=""):
        if not ok:
            self.fail.append(f"{name}: {msg}")

    def guard(self, name, g, mask=None):
        try:
            g.check(mask)
        except AssertionError as ex:
            self.fail.append(f"{name}: {ex}")

    def done(self):
        record_parity(self.id, **self.figs)
        print(self.id, " ".join(f"{k}={v:.3e}" for k, v in self.figs.items()))
        assert not self.fail, "\n".join(self.fail)


# ------------------------------------------------------------------------------------------------ kernel families

def family_cfgs(ops, fam):
    """cfg ids of a kernel family in the loaded library: [(cfg, tile pixels, tile couts, third column of the table)]."""
    return [(i, c[0], c[1], c[2]) for i, c in enumerate(ops.cfg_table()) if c[3] == fam]


def tile_shape(ops, fam, cfg, OH, OW, K, stride):
    """(TH, TW) with which `cfg` is launched on an OH x OW output."""
    tp = ops.cfg_table()[cfg][0]
    if fam == 3:
        return 16, 16
    if fam == 6:
        return 8, 16
    if fam == 4:
        return 1, tp
    if fam == 7:
        tw = 128 if OW >= 128 else 1 << (OW.bit_length() - 1)
        return 128 // tw, tw
    if fam == 8:
        return (1, 32) if OH == 1 or OW > 16 else ((2, 16) if OW > 8 else (4, 8))
    sh = ops.launchable_shapes(cfg, max(OH, 2) if K > 1 else OH, OW, K, K, stride)     # (OH = 1 means token rows to the planner: a window needs a 2-D tile)
    assert sh, f"cfg {cfg} has no tile shape for {OH}x{OW} k{K} s{stride}"
    return sh[0][2], sh[0][3]


# ------------------------------------------------------------------------------------------------ one case

def _act(ops, vals, lay, dev, H, W):
    B, R, C = vals.shape
    ld = C + lay[0]
    a = strided16(ops, vals, ld, R * ld + lay[1], dev, lay[2])
    a.H, a.W = H, W
    return a


def _dense(ops, vals, dev, H, W):
    return _act(ops, vals, (0, 0, 0), dev, H, W)


def build(c):
    """The operands (fp64 holding the values the launch reads) and the fp64 reference of a case."""
    g = torch.Generator().manual_seed(c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, H, W, C1, C2, Cout, K, stride = c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"], c["K"], c["stride"]
    C = C1 + C2
    pad = c["pad"] if c["pad"] is not None else ((K - 1) // 2 if stride == 1 else 0)
    T = dict(pad=pad)
    T["x1"] = r16(rn(B, H, W, C1) * 1.2 + 0.1)
    T["x2"] = r16(rn(B, H, W, C2) * 0.8) if C2 else None
    T["w"] = (rn(Cout, C, K, K) / math.sqrt(K * K * C)).half().float()      # what pack_weight stores without rounding
    T["bias"] = (rn(Cout) * 0.1).float() if c["bias"] else None
    xin = T["x1"] if C2 == 0 else torch.cat((T["x1"], T["x2"]), -1)
    pro = c["prologue"]
    assert pro != "none" or c["act_in"] == "none", "an input activation is part of a prologue"
    a = xin
    if pro != "none":
        T["pa"] = (1 + 0.2 * rn(B if c["affine"] else 1, C)).float()
        T["ps"] = (0.2 * rn(B, C)).float() if c["affine"] else None
        z = xin
        if pro == "ln":
            T["mu"] = xin.mean(-1).float()
            T["rs"] = torch.rsqrt(xin.var(-1, unbiased=False) + 1e-5).float()
            z = (z - T["mu"].double()[..., None]) * T["rs"].double()[..., None]
        elif pro == "rs":
            T["rs"] = (1.0 / (xin.norm(dim=-1) + 0.3)).float()     # an arbitrary per-pixel scale
            z = z * T["rs"].double()[..., None]
        else:
            T["ssq_a"] = (T["x1"] ** 2).sum(-1).float()
            q = T["ssq_a"].double()
            if C2:
                T["ssq_b"] = (T["x2"] ** 2).sum(-1).float()
                q = q + float(torch.tensor(WB, dtype=torch.float32)) * T["ssq_b"].double()
            z = z / q.sqrt().clamp(min=1e-12)[..., None]
        z = z * T["pa"].double()[:, None, None, :]
        if T["ps"] is not None:
            z = z + T["ps"].double()[:, None, None, :]
        a = r16(ACT64[c["act_in"]](z))
    w64 = T["w"].double()
    an = a.permute(0, 3, 1, 2)
    acc = F.conv2d(an, w64, None, stride=stride, padding=pad)
    mag = F.conv2d(an.abs(), w64.abs(), None, stride=stride, padding=pad)
    if T["bias"] is not None:
        acc = acc + T["bias"].double().view(1, -1, 1, 1)
        mag = mag + T["bias"].double().abs().view(1, -1, 1, 1)
    OH, OW = acc.shape[2], acc.shape[3]
    T["OH"], T["OW"] = OH, OW
    v = ACT64[c["act_out"]](acc).permute(0, 2, 3, 1)        # [B, OH, OW, Cout]
    mag = mag.permute(0, 2, 3, 1)
    ep = c["epilogue"]
    if ep == "addend":
        T["add"], T["gate"] = r16(rn(B, OH, OW, Cout)), torch.rand(B, Cout, generator=g, dtype=torch.float64).float()
        t = T["add"] * T["gate"].double()[:, None, None, :]
        v, mag = v + t, mag + t.abs()
    elif ep == "res":
        T["res"] = r16(rn(B, OH, OW, Cout))
        v, mag = v + T["res"], mag + T["res"].abs()
    elif ep == "post":
        T["post_pa"], T["post_ps"] = (1 + 0.2 * rn(B, Cout)).float(), (0.2 * rn(B, Cout)).float()
        v = silu64(v / v.norm(dim=-1, keepdim=True).clamp(min=1e-12) * T["post_pa"].double()[:, None, None, :] + T["post_ps"].double()[:, None, None, :])
    if ep == "shuffle":     # the launch gets the output channels in (s1, s2, c) order; PixelShuffle reads channel c * 4 + s1 * 2 + s2
        sh = lambda t: F.pixel_shuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        v, mag = sh(v), sh(mag)
    T["ref"], T["mag"] = v, mag
    if c["gca"]:
        T["wk"], T["bk"] = (rn(Cout) * 0.3).float(), 0.1
    # no intermediate rounding anywhere in the contract: the per-element bound applies
    T["exact"] = pro == "none" and c["act_out"] == "none" and ep != "post"
    return T


def launch(ops, dev, c, T, cfg, guards=True, dense=False):
    """One IGEMM launch of case `c` with tile configuration `cfg` = (id, TH, TW) | None (family 0, the planner's tile): strided operands in
    guarded allocations, or (dense) what new_act gives.  Returns (plan, params, outputs dict)."""
    B, H, W, C1, C2, Cout, K = c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"], c["K"]
    C, OH, OW, ep = C1 + C2, T["OH"], T["OW"], c["epilogue"]
    lay = (lambda k: (0, 0, 0)) if dense else (lambda k: c[k])
    tok = lambda t: t.reshape(t.shape[0], -1, t.shape[-1])
    x1 = _act(ops, tok(T["x1"]), lay("x1_l"), dev, H, W)
    x2 = _act(ops, tok(T["x2"]), lay("x2_l"), dev, H, W) if C2 else None
    w, bias = T["w"], T["bias"]
    if ep == "shuffle":
        perm = torch.arange(Cout).view(Cout // 4, 4).t().reshape(-1)
        w, bias = w[perm], (bias[perm] if bias is not None else None)
    pw = ops.pack_weight(w, bias, dev, G=c["G"])
    kw, O = {}, {}
    if c["prologue"] != "none":
        ps_ = pw.Cin_pad + c["pstride_extra"]
        rows = lambda t: torch.cat((t, torch.zeros(t.shape[0], ps_ - C)), 1).contiguous().to(dev)
        kw["pa"] = rows(T["pa"])
        if T["ps"] is not None:
            kw["ps"] = rows(T["ps"])
        kw["pstride"] = ps_ if c["affine"] else 0
        for k in ("mu", "rs", "ssq_a", "ssq_b"):
            if T.get(k) is not None:
                kw[k] = T[k].reshape(-1).contiguous().to(dev)
        kw["ssq_wb"] = WB
    act = dict(none=ops.ACT_NONE, silu=ops.ACT_SILU, gelu=ops.ACT_GELU)
    kw["act_in"], kw["act_out"] = act[c["act_in"]], act[c["act_out"]]
    if ep == "addend":
        kw.update(addend=_act(ops, tok(T["add"]), lay("add_l"), dev, OH, OW), gate=T["gate"].to(dev))
    elif ep == "res":
        kw["res"] = _act(ops, tok(T["res"]), lay("res_l"), dev, OH, OW)
    elif ep == "post":
        kw["post"] = dict(pa=T["post_pa"].contiguous().to(dev), ps=T["post_ps"].contiguous().to(dev), pstride=Cout)
    if ep == "nchw":
        O["gy"] = guarded(B * Cout * OH * OW, dev, torch.float32)
        y = O["gy"].t.view(B, Cout, OH, OW)
        O["mask"] = None
        kw["out_mode"] = ops.OUT_NCHW_F32
    else:
        R, Cy = (4 * OH * OW, Cout // 4) if ep == "shuffle" else (OH * OW, Cout)
        l = lay("y_l")
        ld = Cy + l[0]
        bs = R * ld + l[1]
        O["geom"] = (B, R, Cy, ld, bs, l[2])
        n = l[2] + (B - 1) * bs + (R - 1) * ld + Cy + (0 if dense else 24)
        O["gy"] = guarded(n, dev)
        y = O["gy"].act(ops, B, R, Cy, ld, bs, l[2])
        y.H, y.W = (2 * OH, 2 * OW) if ep == "shuffle" else (OH, OW)
        O["mask"] = rows_mask(n, B, R, Cy, ld, bs, l[2])
        if ep == "shuffle":
            kw["out_mode"] = ops.OUT_PIXEL_SHUFFLE
    if c["ssq_out"]:
        O["gs"] = guarded(B * OH * OW, dev, torch.float32)
        kw["ssq_out"] = O["gs"].t
    if c["gca"]:
        kw["gca"] = dict(wk=T["wk"].to(dev), bk=T["bk"])
    plan = ops.Plan("case")
    p = ops.igemm(plan, x1, pw, y, x2=x2, stride=c["stride"], pad=T["pad"], cfg=cfg, **kw)
    if p.gca_part_t is not None:
        O["gg"] = guarded(p.gca_part_t.numel(), dev, torch.float32)
        p.gca_part = O["gg"].t.data_ptr()
    O["keep"] = (x1, x2, pw, kw, y)
    return plan, p, O


def read_y(c, T, O):
    """The stored output as rows [B, pixels, channels] (fp16 / fp32 values as stored)."""
    B, Cout, OH, OW = c["B"], c["Cout"], T["OH"], T["OW"]
    if c["epilogue"] == "nchw":
        return O["gy"].cpu().reshape(B, Cout, OH * OW).permute(0, 2, 1)
    _, R, Cy, ld, bs, lead = O["geom"]
    return O["gy"].cpu().as_strided((B, R, Cy), (bs, ld, 1), lead).clone()


def baseline(ops, dev, c, T):
    """The launch-per-op plan on dense operands: ACT_PREP for the prologue, the raw convolution on a family-0 configuration with the same
    epilogue (post: the plain convolution, then ACT_PREP with its own statistics; ACT_PREP and ROWSTAT need Cout % 8 == 0, so for other widths
    ACT_PREP's fp32 arithmetic runs in torch on the stored rows and ROWSTAT is left out), ROWSTAT for ssq_out.  Returns (rows, ssq | None)."""
    cb = dict(c, prologue="none", act_in="none", C1=c["C1"] + c["C2"], C2=0, ssq_out=False, gca=False)
    Tb = dict(T)
    B, H, W, C = c["B"], c["H"], c["W"], c["C1"] + c["C2"]
    plan = ops.Plan("launch-per-op")
    tok = lambda t: t.reshape(t.shape[0], -1, t.shape[-1])
    keep = []
    if c["prologue"] != "none":
        x1 = _dense(ops, tok(T["x1"]), dev, H, W)
        x2 = _dense(ops, tok(T["x2"]), dev, H, W) if c["C2"] else None
        ya = ops.new_act(B, H, W, C, dev)
        d = lambda k: T[k].reshape(-1).contiguous().to(dev) if T.get(k) is not None else None
        act = dict(none=ops.ACT_NONE, silu=ops.ACT_SILU)
        ops.act_prep(plan, x1, ya, x2=x2, mu=d("mu"), rs=d("rs"), pa=T["pa"].contiguous().to(dev), ps=T["ps"].contiguous().to(dev) if T["ps"] is not None else None,
                     pstride=C if c["affine"] else 0, act_in=act[c["act_in"]], ssq_a=d("ssq_a"), ssq_b=d("ssq_b"), ssq_wb=WB)
        plan.run()
        torch.cuda.synchronize()
        Tb["x1"], Tb["x2"] = ya.t.cpu().double().reshape(B, H, W, C), None
    else:
        Tb["x1"] = T["x1"] if c["C2"] == 0 else torch.cat((T["x1"], T["x2"]), -1)
        Tb["x2"] = None
    post = c["epilogue"] == "post"
    if post:
        cb["epilogue"] = "plain"
    G = ops.choose_G(C, c["K"] * c["K"]) if c["G"] is None else c["G"]
    cfg = ops.pick_cfg(G, c["Cout"], max(T["OH"], 2) if c["K"] > 1 else T["OH"], T["OW"], B, c["K"], c["K"], c["stride"], family=0)
    plan, p, O = launch(ops, dev, cb, Tb, cfg, dense=True)
    plan.run()
    torch.cuda.synchronize()
    rows = read_y(cb, Tb, O)
    ssq = None
    if post and c["Cout"] % 8:      # ACT_PREP takes whole 8-channel groups: for other widths its arithmetic in torch, fp32 from the stored fp16 rows
        h = rows.float()
        z = h * torch.rsqrt((h * h).sum(-1, keepdim=True).clamp(min=1e-24)) * T["post_pa"][:, None, :] + T["post_ps"][:, None, :]
        return (z * torch.sigmoid(z)).half(), None
    if post or (c["ssq_out"] and c["Cout"] % 8 == 0):     # (ROWSTAT takes whole 8-channel groups: no figure of its own for other widths)
        ya = _dense(ops, rows.double(), dev, T["OH"], T["OW"])
        plan = ops.Plan("launch-per-op tail")
        if post:
            out = ops.new_act(B, T["OH"], T["OW"], c["Cout"], dev)
            ops.act_prep(plan, ya, out, pa=T["post_pa"].contiguous().to(dev), ps=T["post_ps"].contiguous().to(dev), pstride=c["Cout"], act_in=ops.ACT_SILU, self_stat=True)
        else:
            ssq = torch.empty(B * T["OH"] * T["OW"], device=dev)
            ops.rowstat(plan, ya, mode=2, rs=ssq)
        plan.run()
        torch.cuda.synchronize()
        if post:
            rows = out.t.cpu().reshape(B, -1, c["Cout"])
        else:
            ssq = ssq.cpu()
    return rows, ssq


def gca_rows(got, c, T, th, tw):
    """fp64 GlobalContext partials of the stored rows `got` [B, OH * OW, Cout], tile by tile: (logits' maxima [B, tiles], per tile a function
    (m) -> (sum exp, weighted channel sums) evaluated at the maximum the kernel reports, bound on a logit's error)."""
    B, OH, OW, Cout = c["B"], T["OH"], T["OW"], c["Cout"]
    h = got.double().reshape(B, OH, OW, Cout)
    wk = T["wk"].double()
    logit = h @ wk + float(torch.tensor(T["bk"], dtype=torch.float32))
    dl = (Cout + 2) * U * ((h.abs() @ wk.abs()) + abs(T["bk"]))      # Cout products (one rounding each: fp16 x fp32) and Cout additions in any order
    tiles = []
    for ty in range(-(-OH // th)):
        for tx in range(-(-OW // tw)):
            ys, xs = slice(ty * th, min(OH, (ty + 1) * th)), slice(tx * tw, min(OW, (tx + 1) * tw))
            tiles.append((logit[:, ys, xs].reshape(B, -1), h[:, ys, xs].reshape(B, -1, Cout), dl[:, ys, xs].reshape(B, -1)))
    return tiles


def run_case(ops, dev, v, name, fam, cfg_id, **kw):
    """Run one case on family `fam` (tile configuration `cfg_id`) and its launch-per-op plan, record every figure in the Verdict `v` under
    `name` and append what fails to it.  Returns the figures."""
    c = dict(DEFAULTS)
    c.update(kw)
    T = build(c)
    B, Cout, OH, OW, ep = c["B"], c["Cout"], T["OH"], T["OW"], c["epilogue"]
    th, tw = tile_shape(ops, fam, cfg_id, OH, OW, c["K"], c["stride"])
    plan, p, O = launch(ops, dev, c, T, (cfg_id, th, tw))
    v.check(name, not c["ssq_out"] or p.ssq_emitted, "ssq_out was not emitted")
    v.check(name, ep != "post" or p.post_applied, "post was not applied")
    v.check(name, not c["gca"] or p.gca_part_t is not None, "the GlobalContext partials were not emitted")
    plan.run()
    torch.cuda.synchronize()
    got = read_y(c, T, O)
    ref = T["ref"].reshape(B, -1, got.shape[-1])
    base, base_ssq = baseline(ops, dev, c, T)
    wf, tf = figures(got, ref)
    wb, tb = figures(base, ref)
    f = {"px": wf, "px_unfused": wb, "all": tf, "all_unfused": tb}
    v.check(name, tf < TOL, f"whole-tensor figure {tf:.3e} >= {TOL}")
    v.check(name, tb < TOL, f"whole-tensor figure of the launch-per-op plan {tb:.3e} >= {TOL}")
    if T["exact"]:
        mag = T["mag"].reshape(B, -1, got.shape[-1])
        Kp = c["K"] * c["K"] * (c["C1"] + c["C2"])
        last = ULP32 * ref.abs() if ep == "nchw" else ulp16(ref)
        el = ((got.double() - ref).abs() / (last + (Kp + 4) * ULP32 * mag)).reshape(-1)
        f["elem"] = float(torch.nan_to_num(el, nan=float("inf")).max())
        v.check(name, f["elem"] <= 1.0, f"an element is {f['elem']:.2f} x its bound ulp + (K + 4) ulp32 sum|terms| from the exact value (worst pixel {wf:.3e})")
        v.worst("elem", f["elem"])
    else:
        v.check(name, wf <= 2 * wb, f"worst pixel {wf:.3e} > 2 x that of the launch-per-op plan {wb:.3e}")
        v.worst("px", wf)
        v.worst("px_unfused", wb)
        v.worst("ratio", wf / max(wb, 1e-300))
    v.guard(name + ".y", O["gy"], O["mask"])
    if c["ssq_out"] and p.ssq_emitted:
        # every family keeps a pixel's couts on the two half-wave lanes of WN waves: tile couts / WN / 16 groups of 8 per lane one after the
        # other, one __shfl_xor addition, then WN - 1 <= 3 additions across the waves (inside sum_bound's extra).  WN is a template argument
        # of each configuration that the cfg table does not export, so the bar takes tile couts / 16 groups, which is exact for WN = 1 and up
        # to 4 x the chain of a WN = 4 configuration (8 bn / 16 + 5 against 8 bn / 64 + 5 roundings).  The ROWSTAT figure of the launch-per-op
        # plan is recorded beside it for the record only: it is asserted in tests/test_elementwise_kernels_gpu.py
        bn = ops.cfg_table()[cfg_id][1]
        bar = sum_bound(-(-bn // 16), 2)
        want = (got.double() ** 2).sum(-1).reshape(-1)
        e = (O["gs"].cpu().double() - want).abs() / want.clamp(min=1e-300)
        f["ssq"] = float(torch.nan_to_num(e, nan=float("inf")).max())
        if base_ssq is not None:
            wb_ = (base.double() ** 2).sum(-1).reshape(-1)
            f["ssq_rowstat"] = float(((base_ssq.double() - wb_).abs() / wb_.clamp(min=1e-300)).max())
        v.check(name, f["ssq"] <= bar, f"ssq_out off by {f['ssq']:.3e} of its pixel's sum (bar {bar:.3e})")
        v.worst("ssq_of_bar", f["ssq"] / bar)
        v.guard(name + ".ssq_out", O["gs"])
    if "gg" in O:
        part = O["gg"].cpu().double().reshape(B, -1, Cout + 2)
        tiles = gca_rows(got, c, T, th, tw)
        v.check(name, part.shape[1] == len(tiles), f"{part.shape[1]} rows of partials for {len(tiles)} tiles")
        worst = 0.0
        for i, (lg, h, dl) in enumerate(tiles[:part.shape[1]]):
            m, se, sv = part[:, i, 0], part[:, i, 1], part[:, i, 2:]
            e_m = ((m - lg.max(-1).values).abs() / dl.max(-1).values).max()     # the maximum of logits that are each within dl of these
            ew = torch.exp(lg - m[:, None])
            # exp of a logit that is off by dl, through exp2 of a rounded product (|x| u) at one ulp32; then a sum of n terms in any order
            rel = 2 * dl.max() + (float((lg - m[:, None]).abs().max()) + 4 + ew.shape[1]) * ULP32
            e_s = ((se - ew.sum(-1)).abs() / ew.sum(-1)).max() / rel
            want = torch.einsum("bq,bqc->bc", ew, h)
            e_v = ((sv - want).norm(dim=-1) / torch.einsum("bq,bqc->bc", ew, h.abs()).norm(dim=-1).clamp(min=1e-300)).max() / rel
            worst = max(worst, float(torch.nan_to_num(torch.stack((e_m, e_s, e_v)), nan=float("inf")).max()))
        f["gca_of_bar"] = worst
        v.check(name, worst <= 1.0, f"a row of GlobalContext partials is {worst:.2f} x its bound from the stored tile")
        v.guard(name + ".gca_part", O["gg"])
    SUMMARY.setdefault(fam, {"cases": 0})["cases"] += 1
    v.figs.update({f"{name}.{k}": x for k, x in f.items()})
    return f
