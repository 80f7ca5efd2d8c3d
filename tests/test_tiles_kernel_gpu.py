"""MI355X (-m gpu; also on the CPU emulation, IMAGEN_EMUL_TESTS=1: tests/test_tiles_cpu.py keeps the file in the CPU suite): TILES of
csrc/tiles.hip against its contract (tests/plan_interp_tile.py), on sentinel-guarded output buffers.

Geometries (canvas, tile, overlap -> T), the smallest at which the kernel can go wrong:
    16 x 16,   16 x 16, any     -> 1   the identity
    16 x 24,   16 x 16, 8       -> 2   two tiles side by side
    24 x 40,   16 x 16, (8, 4)  -> 6   a 2 x 3 grid whose last column is clamped
    20 x 22,   16 x 16, 10      -> 4   origins at x = 0 and 6, so x0 % 4 != 0 (and W % 4 != 0): the 4-byte path
    256 x 640, 256 x 256, 64    -> 3   many workgroups
(B, C) in {(1, 3), (3, 1), (3, 3)}, both blends; one case has `src` and `nw` 4 bytes off a 16-byte boundary.

Gather: torch slicing, bit for bit.  Blend: per element against the contract in fp64 under TOL = 1e-6 normwise, the project's bar of the
elementwise sampler kernels (COMPOSE_X0 / GUIDE_X0): a covered element is a sum of at most 4 products of fp32 numbers whose weights sum to 1,
so its fp32 evaluation is within a few 2^-24 of the fp64 one.  Bit-exact: absdst == |dst|; blend(gather(x)) == x at T = 1; singly-covered
pixels carry the tile's bits; two runs are identical.  An out-of-range origin is clamped: sentinels intact, the result the clamped origin's."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import gpu_device, record_parity  # noqa: E402
from plan_interp_tile import tiles_blend_contract, tiles_gather_contract  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6
SENTINEL = -77.25
GEOMETRIES = (((16, 16), (16, 16), (4, 4), 1), ((16, 24), (16, 16), (8, 8), 2), ((24, 40), (16, 16), (8, 4), 6), ((20, 22), (16, 16), (10, 10), 4),
              ((256, 640), (256, 256), (64, 64), 3))
BLENDS = ("ramp", "uniform")


def nerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o
    return o


def geometry(canvas, tile, overlap, blend):
    from imagen_pytorch_amd.sample_call import tile_geometry
    return tile_geometry(*canvas, *tile, *overlap, blend)


def guarded(n, dev):
    whole = torch.full((n + 32,), SENTINEL, device=dev)
    return whole, whole[16:16 + n]


def intact(whole, name):
    assert bool((whole[:16] == SENTINEL).all()) and bool((whole[-16:] == SENTINEL).all()), f"{name}: written outside the buffer"


def off16(t, off, dev):
    """`t` on the device at `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=dev, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def run_gather(ops, canvas, origins, h, w, off=0):
    dev = gpu_device()
    B, C, H, W = canvas.shape
    T = origins.shape[0]
    whole, dst = guarded(T * B * C * h * w, dev)
    src = off16(canvas, off, dev)
    plan = ops.Plan("tiles")
    ops.tiles(plan, src, dst, origins.to(dev), mode="gather", B=B, C=C, H=H, W=W, h=h, w=w)
    assert [l for _, _, l in plan.ops] == ["tiles.gather"]
    plan.run()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    intact(whole, "gather dst")
    return dst.cpu().reshape(T, B, C, h, w)


def run_blend(ops, tiles, origins, nw, H, W, off=0, absdst=True):
    dev = gpu_device()
    T, B, C, h, w = tiles.shape
    whole, dst = guarded(B * C * H * W, dev)
    whole_a, ab = guarded(B * C * H * W, dev)
    src, nwd = off16(tiles, off, dev), off16(nw, off, dev)
    plan = ops.Plan("tiles")
    ops.tiles(plan, src, dst, origins.to(dev), mode="blend", nw=nwd, absdst=ab if absdst else None, B=B, C=C, H=H, W=W, h=h, w=w)
    assert [l for _, _, l in plan.ops] == ["tiles.blend"]
    plan.run()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    intact(whole, "blend dst")
    intact(whole_a, "blend absdst")
    out = dst.cpu().reshape(B, C, H, W)
    if absdst:
        assert torch.equal(ab.cpu().reshape(B, C, H, W), out.abs()), "absdst != |dst|"
    else:
        assert bool((ab == SENTINEL).all()), "absdst == NULL, yet written"
    return out


def coverage(geo, H, W):
    cnt = torch.zeros(H, W, dtype=torch.int32)
    for y0, x0 in geo["origins"].tolist():
        cnt[y0:y0 + geo["h"], x0:x0 + geo["w"]] += 1
    return cnt


@pytest.mark.parametrize("canvas,tile,overlap,T", GEOMETRIES)
@pytest.mark.parametrize("B,C", [(1, 3), (3, 1), (3, 3)])
def test_gather_and_blend(ops, canvas, tile, overlap, T, B, C):
    (H, W), (h, w) = canvas, tile
    g = torch.Generator().manual_seed(900 + H + 3 * W + B)
    x = torch.randn(B, C, H, W, generator=g)
    worst = 0.0
    for blend in BLENDS:
        geo = geometry(canvas, tile, overlap, blend)
        assert geo["T"] == T
        tiles = run_gather(ops, x, geo["origins"], h, w)
        assert torch.equal(tiles, tiles_gather_contract(x, geo["origins"], h, w)), "gather is a pure copy"
        v = torch.randn(T, B, C, h, w, generator=g)
        got = run_blend(ops, v, geo["origins"], geo["nw"], H, W)
        err = nerr(got, tiles_blend_contract(v, geo["origins"], geo["nw"], H, W, dtype=torch.float64))
        worst = max(worst, err)
        print(f"tiles {H}x{W} B={B} C={C} {blend}: blend normwise error vs fp64 {err:.2e}")
        assert err < TOL, (canvas, blend, err)
        assert torch.equal(got, run_blend(ops, v, geo["origins"], geo["nw"], H, W, absdst=False)), "two runs differ"
        # singly-covered pixels (nw exactly 1.0) carry the tile's bits
        single = coverage(geo, H, W) == 1
        for t, (y0, x0) in enumerate(geo["origins"].tolist()):
            m = single[y0:y0 + h, x0:x0 + w]
            assert torch.equal(got[:, :, y0:y0 + h, x0:x0 + w][:, :, m], v[t][:, :, m])
        if T == 1:
            assert torch.equal(run_blend(ops, tiles, geo["origins"], geo["nw"], H, W), x), "T = 1: blend(gather(x)) == x"
    record_parity(f"tiles_kernel[{H}x{W}-B{B}-C{C}]", worst=worst)


def test_unaligned_src_and_nw_take_the_scalar_path(ops):
    """24 x 40 with 16 x 16 tiles (every size a multiple of 4), but src and nw start 4 bytes past a 16-byte boundary: 16-byte loads would be
    misaligned, so the launcher must pick the 4-byte kernel; the result has the aligned run's bits."""
    g = torch.Generator().manual_seed(77)
    geo = geometry((24, 40), (16, 16), (8, 4), "ramp")
    x, v = torch.randn(3, 3, 24, 40, generator=g), torch.randn(6, 3, 3, 16, 16, generator=g)
    assert torch.equal(run_gather(ops, x, geo["origins"], 16, 16, off=1), run_gather(ops, x, geo["origins"], 16, 16))
    got = run_blend(ops, v, geo["origins"], geo["nw"], 24, 40, off=1)
    assert nerr(got, tiles_blend_contract(v, geo["origins"], geo["nw"], 24, 40, dtype=torch.float64)) < TOL
    assert torch.equal(got, run_blend(ops, v, geo["origins"], geo["nw"], 24, 40)), "the 4-byte and the 16-byte paths differ"


def test_out_of_range_origins_are_clamped(ops):
    """An origin table with entries outside the canvas reads and writes nothing outside the buffers (the sentinels of run_gather / run_blend), and
    gives what the clamped table gives."""
    g = torch.Generator().manual_seed(78)
    geo = geometry((24, 40), (16, 16), (8, 4), "ramp")
    x, v = torch.randn(1, 3, 24, 40, generator=g), torch.randn(6, 1, 3, 16, 16, generator=g)
    bad = geo["origins"].clone()
    bad[0], bad[2], bad[5] = torch.tensor([-5, -1000000]), torch.tensor([0, 1 << 30]), torch.tensor([9, 25])
    good = bad.clone()
    good[:, 0].clamp_(0, 24 - 16)
    good[:, 1].clamp_(0, 40 - 16)
    assert torch.equal(run_gather(ops, x, bad, 16, 16), run_gather(ops, x, good, 16, 16))
    assert torch.equal(run_gather(ops, x, bad, 16, 16), tiles_gather_contract(x, good, 16, 16))
    assert torch.equal(run_blend(ops, v, bad, geo["nw"], 24, 40), run_blend(ops, v, good, geo["nw"], 24, 40))


def test_launcher_refuses_bad_fields(ops):
    """The C side validates on the host (a caller binding the ABI directly): nothing is launched."""
    from imagen_pytorch_amd import _abi

    dev = gpu_device()
    lib = _abi.load_library()
    kind = _abi.ENUMS["IMAGEN_OP_TILES"]
    geo = geometry((16, 24), (16, 16), (8, 8), "ramp")
    for mode, field, value, msg in (("gather", "T", 0, b"T outside"), ("gather", "T", 65, b"T outside"), ("gather", "h", 17, b"larger than the canvas"),
                                    ("gather", "w", 25, b"larger than the canvas"), ("gather", "B", 0, b"non-positive"), ("gather", "C", -1, b"non-positive"),
                                    ("gather", "H", 0, b"non-positive"), ("gather", "w", 0, b"non-positive"), ("gather", "mode", 2, b"mode"),
                                    ("gather", "mode", -1, b"mode"), ("blend", "nw", None, b"nw == NULL")):
        canvas, rows = torch.zeros(1, 3, 16, 24, device=dev), torch.zeros(2, 1, 3, 16, 16, device=dev)
        src, dst = (canvas, rows) if mode == "gather" else (rows, canvas)
        p = ops.tiles(ops.Plan(), src, dst, geo["origins"].to(dev), mode=mode, nw=geo["nw"].to(dev), B=1, C=3, H=16, W=24, h=16, w=16)
        setattr(p, field, value)
        assert lib.imagen_launch(kind, ctypes.addressof(p), ctypes.sizeof(p), ops.current_stream_handle() if dev.type == "cuda" else None) != 0
        assert msg in lib.imagen_last_error(), (field, lib.imagen_last_error())
