"""The convolution / GEMM kernel families behind launch_igemm() — family 0 (csrc/igemm.hip), 2 conv_dma, 3 conv_stream, 4 conv_pw, 5 conv_big,
6 conv_pro, 7 conv_gemm, 8 conv_small — each forced by its tile configuration, per PIXEL against the fp64 restatement of the IGEMM contract
(tests/igemm_contract.py), on strided operands in guarded allocations.  tests/test_igemm_cfgs_gpu.py covers the configurations with one
whole-tensor fp32 norm on dense tensors; here the shapes are the smallest at which a path can go wrong and every figure is local:

 * per ELEMENT where the contract has no intermediate rounding (raw input; plain / addend / res / NCHW-fp32 / pixel-shuffle epilogue, no act_out):
   |got - exact| <= ulp16(exact) + (K + 4) ulp32 sum|terms|, K = KH KW Cin products (NCHW fp32: one ulp32 of the value instead of ulp16) — the
   bound of RESPREP's `out` in tests/test_rowchain_contract_gpu.py: the stored value is a neighbour of the exact one, a full ulp32 per addition.
 * per PIXEL everywhere else (a prologue, act_out, post): the worst pixel of the family is at most twice the worst pixel of the launch-per-op plan
   on the same inputs against the same reference (ACT_PREP, the raw convolution on a family-0 configuration, ACT_PREP with its own statistics
   for post).  Same rounding points, another fp32 summation order, the occasional one-ulp flip of an intermediate: the factor 2 of the
   ROWCHAIN file.  The whole-tensor figure of both plans stays under the project's 1e-3.
 * ssq_out per pixel against the sum of squares of the stored fp16 row at `sum_bound`: in every family a pixel's couts sit on the two half-wave
   lanes of WN waves (tile couts / WN / 16 groups of 8 per lane, one __shfl_xor addition, WN - 1 additions across the waves).
 * the GlobalContext partials per tile row against the stored tile, partly covered tiles included.
 * sentinels around every output, in the channel gap Cout .. ld of every pixel, between images, behind ssq_out and behind gca_part.
 * the GlobalContext maximum m equals the tile's largest logit within the logit's own rounding bound.
 * the alignment predicates of launch_igemm and of the families' launchers: met just inside by passing cases (test_eight_byte_operands: every pitch and base at 8 but not 16
   bytes where the accesses are 8 bytes wide), refused just outside (test_refusals: by return status, nothing written).

Cases: outputs as channel slices (ld = Cout + 32, off = 16, bs = pixels * ld + 64) with Cout ending inside a 4-wide and an 8-wide store; inputs,
addend and res with pitches of their own, pstride > Cin_pad; maps smaller than a tile and one past it (1x1, 2x2, 4x4, 3x5, (TH+1) x (TW+1), token
rows of TP + 1) at B = 1 and 3; the concat boundary inside a 32-channel chunk; the all-cout epilogues on ragged tiles; the shortest tile ranges of
the persistent kernels.  A case is skipped only where the loaded library does not hold the family.

Runs on MI355X (-m gpu) and on the CPU emulation (IMAGEN_EMUL_TESTS=1; tests/test_igemm_emulated.py keeps it in the CPU suite)."""
import pytest
import torch

from conftest import gpu_device, record_parity
from igemm_contract import DEFAULTS, SUMMARY, Verdict, build, family_cfgs, launch, run_case, tile_shape

pytestmark = pytest.mark.gpu

RAW = dict(prologue="none", act_in="none")
SSQ = dict(prologue="ssq", act_in="silu", affine=False)
SSQ_AFF = dict(prologue="ssq", act_in="silu", affine=True, pstride_extra=8)
LN = dict(prologue="ln", act_in="none", affine=True, pstride_extra=8)
RS = dict(prologue="rs", act_in="silu", affine=True)


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o

    return o


@pytest.fixture(scope="module")
def dev():
    return gpu_device()


@pytest.fixture(scope="module", autouse=True)
def _summary():
    """One parity record per family, written when the module's last test has run."""
    yield
    for fam, rec in sorted(SUMMARY.items()):
        record_parity(f"conv_contract.family{fam}", **{k: float(x) for k, x in rec.items()})


def cfg_of(ops, fam, bn=None, G=4, Cout=None, kch=None):
    """The tile configuration of `fam` a case is forced onto (the smallest tile that fits), or a skip where the library has none."""
    cfgs = family_cfgs(ops, fam)
    if not cfgs:
        pytest.skip(f"the loaded library holds no kernel family {fam}")
    if fam == 0:
        cfgs = [c for c in cfgs if c[3] == G]
    if fam == 4:
        cfgs = [c for c in cfgs if c[3] == kch and c[2] >= Cout]
    if fam == 6:
        cfgs = [c for c in cfgs if c[2] == (64 if Cout == 64 else 32)]
    if bn is not None:
        cfgs = [c for c in cfgs if c[2] == bn] or cfgs
    assert cfgs, (fam, bn, G, Cout, kch)
    return min(cfgs, key=lambda c: (c[1], c[2]))[0]


def forms(ops, fam):
    """[(tag, cfg, base case)] of a family: its 3x3 and its 1x1 form, with the narrowest inputs it takes."""
    if fam == 0:
        return [("3x3", cfg_of(ops, 0, bn=64), dict(K=3, G=4, C1=32)), ("1x1", cfg_of(ops, 0, bn=64), dict(K=1, G=4, C1=32))]
    if fam in (2, 5):
        return [("3x3", cfg_of(ops, fam), dict(K=3, G=4, C1=32))]
    if fam == 3:
        return [("3x3", cfg_of(ops, 3), dict(K=3, G=4, C1=32))]
    if fam == 4:
        return [("1x1", None, dict(K=1, G=4, C1=32, C2=32))]
    if fam == 6:
        return [("3x3", None, dict(K=3, G=4, C1=32))]
    if fam == 7:
        return [("1x1", cfg_of(ops, 7), dict(K=1, G=4, C1=64, C2=32))]
    return [("3x3", cfg_of(ops, 8, bn=32), dict(K=3, G=4, C1=32)), ("1x1", cfg_of(ops, 8, bn=32), dict(K=1, G=4, C1=32))]


def resolve(ops, fam, cfg, c):
    """Families 4 and 6 have one configuration per channel count: chosen by the case."""
    if fam == 4:
        return cfg_of(ops, 4, Cout=c.get("Cout", 32), kch=(c["C1"] + c.get("C2", 0)) // 32)
    if fam == 6:
        return cfg_of(ops, 6, Cout=c.get("Cout", 32))
    return cfg


def bn_of(ops, cfg):
    return ops.cfg_table()[cfg][1]


def pro_of(fam):
    """A prologue the family takes (None: raw inputs only)."""
    return {0: RS, 3: SSQ_AFF, 6: SSQ, 7: LN, 8: SSQ_AFF}.get(fam)


def go(ops, dev, v, name, fam, cfg, base, **kw):
    c = dict(base, **kw)
    return run_case(ops, dev, v, name, fam, resolve(ops, fam, cfg, c), **c)


FAMS = (0, 2, 3, 4, 5, 6, 7, 8)


# ------------------------------------------------------------------------------------------------ channel slices, strided inputs

@pytest.mark.parametrize("fam", FAMS)
def test_slices(ops, dev, fam):
    """y as a channel slice of a wider tensor with a gap between images, every input with a pitch and a lead of its own; Cout that fills the
    tile, ends inside an 8-wide store (tile - 4, 36, 20) and inside a pair of them (tile - 8); every epilogue and prologue the family takes."""
    v = Verdict(f"conv_contract.slices[family {fam}]", fam)
    for tag, cfg, base in forms(ops, fam):
        H, W = (5, 9) if fam not in (3, 5, 6) else (9, 18)
        b = dict(base, B=2, H=H, W=W)
        pro = pro_of(fam)
        if fam == 4:
            for ep, Cout in (("plain", 32), ("addend", 24), ("res", 32)):
                go(ops, dev, v, f"{tag}.{ep}.{Cout}", fam, cfg, b, Cout=Cout, epilogue=ep, ssq_out=True)
            go(ops, dev, v, f"{tag}.one_input", fam, cfg, b, C1=64, C2=0, Cout=32, epilogue="addend")
            continue
        if fam == 6:
            for C2 in (0, 32):
                go(ops, dev, v, f"{tag}.ssq.{C2}", fam, cfg, b, C2=C2, Cout=32, ssq_out=True, **SSQ)
                go(ops, dev, v, f"{tag}.ssq_aff.post.{C2}", fam, cfg, b, C2=C2, Cout=32, epilogue="post", **SSQ_AFF)
            go(ops, dev, v, f"{tag}.raw", fam, cfg, b, Cout=32, ssq_out=True)
            go(ops, dev, v, f"{tag}.64.post", fam, cfg, b, C1=64, C2=32, Cout=64, epilogue="post", **SSQ)
            go(ops, dev, v, f"{tag}.64.raw", fam, cfg, b, C1=32, C2=32, Cout=64)
            continue
        bn = bn_of(ops, cfg)
        top = 32 if fam == 3 else bn
        go(ops, dev, v, f"{tag}.plain.{top}", fam, cfg, b, Cout=top, ssq_out=True, gca=fam in (2, 5, 7, 8))
        go(ops, dev, v, f"{tag}.plain.{top - 4}", fam, cfg, b, Cout=top - 4, ssq_out=True)
        go(ops, dev, v, f"{tag}.plain.{top - 8}", fam, cfg, b, Cout=top - 8, gca=fam in (2, 5, 7, 8))
        for ep, Cout in (("addend", 36), ("res", 20), ("addend", top - 8), ("nchw", 3), ("post", top - 4)):
            if fam == 3 and Cout > 32:
                Cout = 28
            go(ops, dev, v, f"{tag}.{ep}.{Cout}", fam, cfg, b, Cout=Cout, epilogue=ep)
        Cs = 32 if fam == 3 else 64
        go(ops, dev, v, f"{tag}.shuffle.{Cs}", fam, cfg, b, Cout=Cs, epilogue="shuffle", act_out="silu")
        go(ops, dev, v, f"{tag}.shuffle.raw.{Cs}", fam, cfg, b, Cout=Cs, epilogue="shuffle")
        if pro is not None:
            two = dict(C2=32) if fam != 7 else {}
            go(ops, dev, v, f"{tag}.pro.plain", fam, cfg, b, Cout=top - 4, ssq_out=True, **two, **pro)
            go(ops, dev, v, f"{tag}.pro.res", fam, cfg, b, Cout=20, epilogue="res", **two, **pro)
            go(ops, dev, v, f"{tag}.pro.pstride0", fam, cfg, b, Cout=32, **two, **dict(pro, pstride_extra=0))     # pstride == Cin_pad: the shortest rows
            go(ops, dev, v, f"{tag}.pro.post", fam, cfg, b, Cout=top, epilogue="post", **two, **dict(pro, affine=False, pstride_extra=0))
        if fam in (0, 7, 8):
            go(ops, dev, v, f"{tag}.gelu", fam, cfg, b, Cout=36, act_out="gelu", **(LN if fam != 0 or tag == "1x1" else RS))
    v.done()


# ------------------------------------------------------------------------------------------------ maps smaller than a tile, one past a tile

@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("fam", FAMS)
def test_small_maps(ops, dev, fam, B):
    """1x1, 2x2, 4x4 and 3x5 maps (the 2^2 and 4^2 levels of the README unets), one row and one column past a tile, and token rows of one
    tile + 1: halos that lie wholly outside the image, tiles with a single valid pixel, batch strides between tiny images."""
    v = Verdict(f"conv_contract.small_maps[family {fam} B{B}]", fam)
    for tag, cfg, base in forms(ops, fam):
        c0 = resolve(ops, fam, cfg, dict(base, Cout=32))
        tp = ops.cfg_table()[c0][0]
        th, tw = tile_shape(ops, fam, c0, 64, 64, base["K"], 1)
        sizes = [(1, 1), (2, 2), (4, 4), (3, 5), (th + 1, tw + 1), (1, tp + 1)]
        pro = pro_of(fam)
        for i, (H, W) in enumerate(sizes):
            kw = dict(Cout=32, ssq_out=True)
            if pro is not None and (i + B) % 2 == 0:
                kw.update(pro)
                if fam == 6:
                    kw.update(C2=32, ssq_out=True)
            go(ops, dev, v, f"{tag}.{H}x{W}", fam, cfg, dict(base, B=B, H=H, W=W), **kw)
    v.done()


@pytest.mark.parametrize("form", ("2x2s2", "15x15"))
def test_family0_windows(ops, dev, form):
    """The 2x2 stride-2 downsample and the 15x15 cross-embed window of family 0 on the same small maps."""
    v = Verdict(f"conv_contract.family0_windows[{form}]", 0)
    if form == "2x2s2":
        cfg, base, sizes = cfg_of(ops, 0, bn=64), dict(K=2, stride=2, pad=0, G=4, C1=32, Cout=36), [(2, 2), (4, 4), (6, 10), (18, 18), (2, 130)]
    else:
        cfg, base, sizes = cfg_of(ops, 0, G=1, bn=32), dict(K=15, G=1, C1=8, Cout=20), [(1, 1), (2, 2), (4, 4), (3, 5), (9, 9)]
    for B in (1, 3):
        for H, W in sizes:
            go(ops, dev, v, f"B{B}.{H}x{W}", 0, cfg, dict(base, B=B, H=H, W=W))
    go(ops, dev, v, "pro", 0, cfg, dict(base, B=2, H=6, W=10), **RS)
    v.done()


# ------------------------------------------------------------------------------------------------ concat boundary, all-cout epilogues, tile ranges

@pytest.mark.parametrize("fam", (0, 8))
def test_concat_boundary_inside_a_chunk(ops, dev, fam):
    """C1 = 40, C2 = 24: the second tensor starts at the second 8-channel group of the second 32-channel chunk."""
    v = Verdict(f"conv_contract.concat_boundary[family {fam}]", fam)
    for tag, cfg, base in forms(ops, fam):
        b = dict(base, B=2, H=5, W=9, C1=40, C2=24)
        go(ops, dev, v, f"{tag}.raw", fam, cfg, b, Cout=36, epilogue="addend")
        go(ops, dev, v, f"{tag}.ssq", fam, cfg, b, Cout=32, ssq_out=True, **SSQ_AFF)
        go(ops, dev, v, f"{tag}.ln", fam, cfg, b, Cout=28, **LN)
    v.done()


@pytest.mark.parametrize("fam", FAMS)
def test_all_cout_epilogues_on_ragged_tiles(ops, dev, fam):
    """ssq_out, post and the GlobalContext partials with a last tile that is ragged in both directions; the rows of gca_part that belong to
    partly covered tiles are checked like the others."""
    v = Verdict(f"conv_contract.all_cout[family {fam}]", fam)
    for tag, cfg, base in forms(ops, fam):
        c0 = resolve(ops, fam, cfg, dict(base, Cout=32))
        th, tw = tile_shape(ops, fam, c0, 64, 64, base["K"], 1)
        H, W = (th + 3, tw + 5) if fam != 4 else (3, ops.cfg_table()[c0][0] // 3 + 5)
        b = dict(base, B=2, H=H, W=W)
        wide = cfg_of(ops, fam, bn=128) if fam == 8 else cfg
        Cout = 32 if fam in (3, 4, 6) else bn_of(ops, wide) - 4
        go(ops, dev, v, f"{tag}.ssq_out", fam, wide, b, Cout=Cout, ssq_out=True)
        if fam != 4:
            go(ops, dev, v, f"{tag}.post", fam, wide, b, Cout=Cout, epilogue="post")
        if fam in (2, 5, 7, 8):
            go(ops, dev, v, f"{tag}.gca", fam, wide, b, Cout=Cout, gca=True, ssq_out=True)
            go(ops, dev, v, f"{tag}.gca.B3", fam, wide, dict(b, B=3, H=th + 1, W=tw + 1), Cout=Cout - 4, gca=True)
    v.done()


@pytest.mark.parametrize("fam", (3, 4, 6))
def test_persistent_tile_ranges(ops, dev, fam):
    """The persistent kernels on the shortest ranges: one tile in total, two tiles, an odd count (three images of one tile, five tiles in a row)."""
    v = Verdict(f"conv_contract.tile_ranges[family {fam}]", fam)
    for tag, cfg, base in forms(ops, fam):
        c0 = resolve(ops, fam, cfg, dict(base, Cout=32))
        th, tw = tile_shape(ops, fam, c0, 64, 64, base["K"], 1)
        pro = pro_of(fam) or {}
        for B, H, W in ((1, th, tw), (1, th, 2 * tw), (3, th - 1, tw), (1, th, 5 * tw - 3)):
            if fam == 4:
                H, W = 1, W * th
            go(ops, dev, v, f"{tag}.B{B}.{H}x{W}", fam, cfg, dict(base, B=B, H=H, W=W), Cout=32, ssq_out=True, **(dict(pro, C2=32) if fam == 6 else pro))
    v.done()


# ------------------------------------------------------------------------------------------------ launch_igemm's alignment predicates

ODD8 = dict(x1_l=(8, 64, 8), y_l=(8, 4, 4), add_l=(4, 4, 4), res_l=(12, 12, 4))   # Cout = 20: ld = 28 | 24 | 32, bs % 8 == 4, bases at 8 bytes


@pytest.mark.parametrize("fam", (0, 2, 3, 5))
def test_eight_byte_operands(ops, dev, fam):
    """Just inside the launcher's predicates: a Cout % 8 == 4 output is stored four channels at a time (igemm.hip / conv_epilogue.h: the 16-byte
    pieces need Cout % 8 == 0; the generic epilogue of family 0 widens only after testing ld, bs and the bases), and addend / res are loaded the
    same way, so ldy % 8 == 4, bsy % 8 == 4 and bases at 8 but not 16 bytes are all these accesses need."""
    v = Verdict(f"conv_contract.eight_byte_operands[family {fam}]", fam)
    for tag, cfg, base in forms(ops, fam):
        b = dict(base, B=2, H=5, W=9, Cout=20, **ODD8)
        go(ops, dev, v, f"{tag}.plain", fam, cfg, b, ssq_out=True)
        go(ops, dev, v, f"{tag}.addend", fam, cfg, b, epilogue="addend")
        go(ops, dev, v, f"{tag}.res", fam, cfg, b, epilogue="res", act_out="silu")
        go(ops, dev, v, f"{tag}.post", fam, cfg, b, epilogue="post")
        # a Cout % 8 == 0 output beside an addend at 8 bytes: 16-byte stores of y are not taken by the generic epilogue of family 0 (it
        # tests the addend too), and conv_epilogue.h's generic path never widens
        go(ops, dev, v, f"{tag}.addend.32", fam, cfg, dict(b, Cout=32, y_l=(32, 64, 16)), epilogue="addend")
    v.done()


#        name            epilogue  Cout  field     delta (elements | bytes for a pointer)   needs
POKES = [("bs1",         "plain",  32, "bs1",     4, ""),
         ("x1_base",     "plain",  32, "x1",      8, ""),
         ("ld1",         "plain",  32, "ld1",     4, ""),
         ("bs2",         "plain",  32, "bs2",     4, "two"),
         ("x2_base",     "plain",  32, "x2",      8, "two"),
         ("ld2",         "plain",  32, "ld2",     4, "two"),   # each family's own check beside ld1
         ("ldy_16",      "plain",  32, "ldy",     4, ""),      # a Cout % 8 == 0 plain output: 16-byte pieces
         ("bsy_16",      "plain",  32, "bsy",     4, ""),
         ("y_base_16",   "plain",  32, "y",       8, ""),
         ("post_ldy_16", "post",   32, "ldy",     4, ""),
         ("ldy_8",       "plain",  20, "ldy",     2, ""),      # a Cout % 8 == 4 output: 8-byte stores
         ("bsy_8",       "res",    20, "bsy",     2, ""),
         ("y_base_8",    "addend", 20, "y",       4, ""),
         ("ld_add",      "addend", 20, "ld_add",  2, ""),
         ("bs_add",      "addend", 20, "bs_add",  2, ""),
         ("add_base",    "addend", 20, "addend",  4, ""),
         ("ld_res",      "res",    20, "ld_res",  2, ""),
         ("bs_res",      "res",    20, "bs_res",  2, ""),
         ("res_base",    "res",    20, "res",     4, ""),
         # conv_pw loads addend / res in 16-byte pieces: 8-byte operands pass launch_igemm's check and are refused by the family's own
         ("pw_ld_add",   "addend", 32, "ld_add",  4, "pw"),
         ("pw_bs_add",   "addend", 32, "bs_add",  4, "pw"),
         ("pw_add_base", "addend", 32, "addend",  8, "pw"),
         ("pw_ld_res",   "res",    32, "ld_res",  4, "pw"),
         ("pw_bs_res",   "res",    32, "bs_res",  4, "pw"),
         ("pw_res_base", "res",    32, "res",     8, "pw"),
         # the fp32 per-channel rows are read four floats at a time
         ("pstride_4",   "plain",  32, "pstride", 2, "pro"),
         ("pa_base",     "plain",  32, "pa",      4, "pro"),
         ("ps_base",     "plain",  32, "ps",      4, "pro_ps"),
         ("gate_stride", "addend", 32, "gate_stride", 2, ""),
         ("gate_base",   "addend", 32, "gate",    4, ""),
         ("post_pstride", "post",  32, "post_pstride", 2, ""),
         ("post_pa_base", "post",  32, "post_pa", 4, ""),
         # conv_small: per-batch affine rows no shorter than Cin_pad (just inside: pstride == Cin_pad, test_slices' pro.pstride0)
         ("small_pstride", "plain", 32, "pstride", -4, "small")]


def _takes(fam, poke):
    """Whether the family's own launcher takes the unmoved launch (else the predicate is unreachable behind that refusal): families 2 and 5
    take one raw input tensor, 4 raw inputs and Cout % 8 == 0 with the plain / addend / res epilogues, 6 exactly 32 couts with plain / post."""
    _, ep, Cout, field, _, needs = poke
    if needs == "pw":
        return fam == 4
    if needs == "small":
        return fam == 8
    if needs == "two" and fam in (2, 5):
        return False
    if needs.startswith("pro") and (pro_of(fam) is None or (needs == "pro_ps" and fam == 6)):
        return False
    if fam == 4:
        return Cout == 32 and ep != "post"
    if fam == 6:
        return Cout == 32 and ep in ("plain", "post")
    return True


@pytest.mark.parametrize("fam,poke", [pytest.param(f, p, id=f"{f}-{p[0]}") for f in FAMS for p in POKES if _takes(f, p)])
def test_refusals(ops, dev, fam, poke):
    """Just outside: one stride or base of an otherwise valid launch moved off its alignment.  The launch returns an error (checked by status
    only) and nothing is written; the unmoved launch is a passing case of the tests above."""
    name, ep, Cout, field, delta, needs = poke
    plan, p, O = _valid_launch(ops, dev, fam, ep, Cout, needs)
    assert needs != "small" or p.pstride == p.Cin_pad
    setattr(p, field, (getattr(p, field) or 0) + delta)
    _refused(plan, O)


def _valid_launch(ops, dev, fam, ep, Cout, needs, **kw):
    """A launch the family takes (a passing case of the tests above), built and not yet run: (plan, params, outputs)."""
    tag, cfg, base = forms(ops, fam)[0]
    c = dict(DEFAULTS, **base)
    c.update(B=2, H=5, W=9, Cout=Cout, epilogue=ep, C2=32 if needs == "two" or fam in (4, 7) else 0)
    if fam == 7:
        c.update(C1=64)
    if needs.startswith("pro") or needs == "small" or (fam == 6 and ep == "post"):
        c.update(pro_of(fam), pstride_extra=0)
        if fam == 6:
            c.update(SSQ)
    c.update(kw)
    cid = resolve(ops, fam, cfg, c)
    T = build(c)
    return launch(ops, dev, c, T, (cid,) + tile_shape(ops, fam, cid, T["OH"], T["OW"], c["K"], 1))


def _refused(plan, O):
    from imagen_pytorch_amd._abi import ImagenHipError

    with pytest.raises(ImagenHipError):
        plan.run()
    torch.cuda.synchronize()
    for g in ("gy", "gs", "gg"):
        if g in O:
            O[g].check(torch.zeros(O[g].numel, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ the launchers' contract predicates

def _set(**fields):
    """Poke: fields set to a constant, or (a string) to the value of another field — a pointer to a buffer the launch already holds."""
    def f(ops, p):
        for k, v in fields.items():
            setattr(p, k, getattr(p, v) if isinstance(v, str) else v)
    return f


def _cout_over_tile(ops, p):
    p.Cout = bn_of(ops, p.cfg) + 4


def _gemm_cin_over_2048(ops, p):
    p.C1, p.Cin_pad = 2080 - p.C2, 2080


BASE = (0, 2, 3, 5, 7, 8)          # the families whose epilogue is conv_epilogue.h's contract (family 0: its own restatement of it)
GCA = (2, 5, 7, 8)                 # ... that emit GlobalContext partials
SAFE, EMUL = False, True           # EMUL: a launch that would leave its allocations if a launcher took it (geometry, channel counts, padding) — emulation only
#              name                    families             epilogue  Cout needs   case           poke                                                      emulation only
CONTRACT = [("act_in_gelu",         (2, 3, 4, 5, 6, 7, 8), "plain",  32, "",     {},            lambda o, p: setattr(p, "act_in", o.ACT_GELU),             SAFE),
            ("pro_act_in_gelu",     (3, 6, 8),             "plain",  32, "pro",  {},            lambda o, p: setattr(p, "act_in", o.ACT_GELU),             SAFE),
            ("pro_act_in_none",     (6,),                  "plain",  32, "pro",  {},            lambda o, p: setattr(p, "act_in", o.ACT_NONE),             SAFE),
            ("act_out_silu",        (4, 6),                "plain",  32, "",     {},            lambda o, p: setattr(p, "act_out", o.ACT_SILU),            SAFE),
            ("nhwc_cout_3",         BASE,                  "nchw",   3,  "",     {},            lambda o, p: setattr(p, "out_mode", o.OUT_NHWC),           SAFE),
            ("shuffle_cout_20",     BASE,                  "plain",  20, "",     {},            lambda o, p: setattr(p, "out_mode", o.OUT_PIXEL_SHUFFLE),  SAFE),
            ("shuffle",             (4, 6),                "plain",  32, "",     {},            lambda o, p: setattr(p, "out_mode", o.OUT_PIXEL_SHUFFLE),  SAFE),
            ("addend_and_res",      BASE,                  "addend", 20, "",     {},            _set(res="addend", ld_res="ld_add", bs_res="bs_add"),      SAFE),
            ("pw_addend_and_res",   (4,),                  "addend", 32, "",     {},            _set(res="addend", ld_res="ld_add", bs_res="bs_add"),      SAFE),
            ("res",                 (6,),                  "plain",  32, "",     {},            _set(res="y", ld_res="ldy", bs_res="bsy"),                 SAFE),
            ("addend_no_gate",      BASE,                  "addend", 20, "",     {},            _set(gate=0),                                              SAFE),
            ("pw_addend_no_gate",   (4,),                  "addend", 32, "",     {},            _set(gate=0),                                              SAFE),
            ("post_no_ps",          BASE + (6,),           "post",   32, "",     {},            _set(post_ps=0),                                           SAFE),
            ("post_ssq_out",        BASE + (6,),           "post",   32, "",     {},            _set(ssq_out="y"),                                         SAFE),
            ("post_addend",         BASE + (6,),           "post",   32, "",     {},            _set(addend="y", ld_add="ldy", bs_add="bsy", gate="post_pa", gate_stride="post_pstride"), SAFE),
            ("post_res",            BASE + (6,),           "post",   32, "",     {},            _set(res="y", ld_res="ldy", bs_res="bsy"),                 SAFE),
            ("post_act_out",        BASE + (6,),           "post",   32, "",     {},            lambda o, p: setattr(p, "act_out", o.ACT_SILU),            SAFE),
            ("post",                (4,),                  "plain",  32, "",     {},            _set(post_pa="bias", post_ps="bias"),                      SAFE),
            ("post_cout_over_tile", (0, 2, 5, 7, 8),       "post",   32, "",     {},            _cout_over_tile,                                           EMUL),
            ("ssq_cout_over_tile",  (0, 2, 5, 7, 8),       "plain",  32, "",     dict(ssq_out=True), _cout_over_tile,                                      EMUL),
            ("ssq_nchw",            (0, 2, 3, 4, 5, 6),    "plain",  32, "",     dict(ssq_out=True), lambda o, p: setattr(p, "out_mode", o.OUT_NCHW_F32),  SAFE),
            ("ssq_64_couts",        (6,),                  "plain",  64, "",     dict(C1=32, C2=32), _set(ssq_out="y"),                                    SAFE),
            ("gca_no_wk",           GCA,                   "plain",  32, "",     dict(gca=True), _set(gca_wk=0),                                           SAFE),
            ("gca_shuffle",         GCA,                   "plain",  32, "",     dict(gca=True), lambda o, p: setattr(p, "out_mode", o.OUT_PIXEL_SHUFFLE), SAFE),
            ("gca_act_out",         GCA,                   "plain",  32, "",     dict(gca=True), lambda o, p: setattr(p, "act_out", o.ACT_SILU),           SAFE),
            ("gca_cout_over_tile",  GCA,                   "plain",  32, "",     dict(gca=True), _cout_over_tile,                                          EMUL),
            ("gca_none_emitted",    (0, 3, 4, 6),          "plain",  32, "",     {},            _set(gca_part="y", gca_wk="bias"),                         SAFE),
            ("mu_without_rs",       (7,),                  "plain",  32, "pro",  {},            _set(rs=0),                                                SAFE),
            ("small_mu_without_rs", (8,),                  "plain",  32, "pro",  {},            _set(mu="pa"),                                             SAFE),
            ("mu_rs_beside_ssq_a",  (3, 6),                "plain",  32, "pro",  {},            _set(mu="pa", rs="pa"),                                    SAFE),
            ("mu_rs_no_prologue",   (2, 4, 5),             "plain",  32, "",     {},            _set(mu="bias", rs="bias"),                                SAFE),
            ("ssq_b_one_input",     (6,),                  "plain",  32, "pro",  {},            _set(ssq_b="ssq_a"),                                       SAFE),
            ("no_ssq_b_two_inputs", (6,),                  "plain",  32, "pro",  dict(C2=32),   _set(ssq_b=0),                                             SAFE),
            ("gemm_ssq_b",          (7,),                  "plain",  32, "pro",  {},            _set(ssq_b="pa"),                                          SAFE),
            ("tile_shape",          (0, 2, 3, 5, 6, 7, 8), "plain",  32, "",     {},            lambda o, p: setattr(p, "TH", p.TH + 1),                   EMUL),   # (conv_pw walks 256 | 128 consecutive pixels and has never looked at TH x TW)
            ("stride_2",            (2, 3, 4, 5, 6, 7, 8), "plain",  32, "",     {},            _set(stride=2),                                            EMUL),
            ("kh_off",              (2, 3, 4, 5, 6, 7, 8), "plain",  32, "",     {},            lambda o, p: setattr(p, "KH", 4 - p.KH),                   EMUL),
            ("c2_null_x2",          (3, 4, 6, 7, 8),       "plain",  32, "two",  {},            _set(x2=0),                                                EMUL),
            ("c2_one_input_family", (2, 5),                "plain",  32, "",     {},            _set(C2=32, x2="x1", ld2="ld1", bs2="bs1"),                EMUL),
            ("c1_off_chunk",        (2, 3, 4, 5, 6, 7, 8), "plain",  32, "",     {},            lambda o, p: setattr(p, "C1", p.C1 - 8),                   EMUL),
            ("cout_pad_off_tile",   (0, 2, 3, 5, 6, 7, 8), "plain",  32, "",     {},            lambda o, p: setattr(p, "Cout_pad", p.Cout_pad + 16),      EMUL),
            ("gemm_cin_over_2048",  (7,),                  "plain",  32, "",     {},            _gemm_cin_over_2048,                                       EMUL)]


@pytest.mark.parametrize("fam,poke", [pytest.param(f, p, id=f"{f}-{p[0]}") for p in CONTRACT for f in p[1]])
def test_contract_refusals(ops, dev, fam, poke):
    """Just outside, clause by clause: every predicate of the eight launchers that the alignment pokes above do not reach — the epilogue contract
    (csrc/conv_launch.h: Cout against the output mode, addend beside res, what post_pa / ssq_out / gca_part exclude and the one tile over all couts
    they need), the prologues and activations a family does not build, its tile shape, kernel size, channel chunking and padding.  One field of a
    launch the family takes is moved; the launch is refused (by status) and nothing is written.  Every poke was seen refused by the launchers as
    they stood before conv_launch.h; conv_gemm and conv_small take ssq_out beside any output mode (CONV_EP_SSQ_ANY_LAYOUT), so `ssq_nchw` leaves
    them out."""
    import os

    name, _, ep, Cout, needs, case, fn, emul_only = poke
    if emul_only and os.environ.get("IMAGEN_EMUL_TESTS") != "1":
        pytest.skip("would not stay inside its allocations if a launcher took it: on the emulation only")
    plan, p, O = _valid_launch(ops, dev, fam, ep, Cout, needs, **case)
    fn(ops, p)
    _refused(plan, O)
