"""The plan interpreter (tests/plan_interp_compose.py) with TILES' contract as include/imagen_hip.h states it: gather the overlapping windows of a
canvas into tile rows, blend tile rows into the canvas.  TEST INFRASTRUCTURE, never imported by the product.

A subclass: the parents stay as they are; TILES is kind 35 of the extension range (_abi.EXT_OP_STRUCT), so DISPATCH has the parent's entries and
one more.  `tiles` lists (mode, T) of every TILES launch, in order."""
from __future__ import annotations

import torch

from plan_interp import K, f32
from plan_interp_compose import ComposeInterpreter

i32 = torch.int32


def clamp_origins(origins, H, W, h, w):
    """The (y0, x0) the kernel uses: every entry clamped into [0, H - h] x [0, W - w]."""
    return [(min(max(int(y0), 0), H - h), min(max(int(x0), 0), W - w)) for y0, x0 in origins.tolist()]


def tiles_gather_contract(canvas, origins, h, w):
    """canvas [B, C, H, W] -> tiles [T, B, C, h, w]: a pure copy of every window."""
    H, W = canvas.shape[-2:]
    return torch.stack([canvas[:, :, y0:y0 + h, x0:x0 + w] for y0, x0 in clamp_origins(origins, H, W, h, w)])


def tiles_blend_contract(tiles, origins, nw, H, W, dtype=torch.float32):
    """tiles [T, B, C, h, w], nw [T, h * w] -> canvas [B, C, H, W] in `dtype`: per element acc = nw_t v_t for the first covering tile, acc + nw_t v_t
    for the rest, t ascending; 0 where no tile covers."""
    T, B, C, h, w = tiles.shape
    acc = torch.zeros(B, C, H, W, dtype=dtype)
    seen = torch.zeros(H, W, dtype=torch.bool)
    for t, (y0, x0) in enumerate(clamp_origins(origins, H, W, h, w)):
        term = nw[t].reshape(h, w).to(dtype) * tiles[t].to(dtype)
        win = acc[:, :, y0:y0 + h, x0:x0 + w]
        win.copy_(torch.where(seen[y0:y0 + h, x0:x0 + w], win + term, term))     # (the first term is stored, not added to 0: -0 stays -0)
        seen[y0:y0 + h, x0:x0 + w] = True
    return acc


class TileInterpreter(ComposeInterpreter):
    def __init__(self):
        super().__init__()
        self.tiles = []             # (mode, T) of every TILES launch, in order

    def tiles_op(self, p):
        m = self.mem
        B, C, H, W, h, w, T = p.B, p.C, p.H, p.W, p.h, p.w, p.T
        assert 1 <= T <= K["IMAGEN_TILE_MAX"] and min(B, C, H, W, h, w) > 0 and h <= H and w <= W and p.mode in (0, 1)
        self.tiles.append((int(p.mode), int(T)))
        origins = m.view(p.origins, i32)[:2 * T].reshape(T, 2)
        if p.mode == 0:
            out = tiles_gather_contract(m.view(p.src, f32)[:B * C * H * W].reshape(B, C, H, W), origins, h, w)
            m.view(p.dst, f32)[:T * B * C * h * w].copy_(out.reshape(-1))
            return
        assert p.nw, "the blend reads nw"
        out = tiles_blend_contract(m.view(p.src, f32)[:T * B * C * h * w].reshape(T, B, C, h, w), origins,
                                   m.view(p.nw, f32)[:T * h * w].reshape(T, h * w), H, W)
        m.view(p.dst, f32)[:B * C * H * W].copy_(out.reshape(-1))
        if p.absdst:
            m.view(p.absdst, f32)[:B * C * H * W].copy_(out.abs().reshape(-1))

    DISPATCH = {**ComposeInterpreter.DISPATCH}


TileInterpreter.DISPATCH[K["IMAGEN_OP_TILES"]] = TileInterpreter.tiles_op
