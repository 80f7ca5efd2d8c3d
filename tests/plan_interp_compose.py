"""The plan interpreter (tests/plan_interp_guide.py) with COMPOSE_X0's contract as include/imagen_hip.h states it: K weighted, optionally masked
prompts against one null branch, then CFG_X0's x0.  TEST INFRASTRUCTURE, never imported by the product.

A subclass: the parents stay as they are; COMPOSE_X0 is the second kind of the extension range (_abi.EXT_OP_STRUCT), so DISPATCH has the parent's
entries and one more.  `composes` counts the COMPOSE_X0 launches by (K, masks present)."""
from __future__ import annotations

import torch

from plan_interp import K, f32
from plan_interp_guide import GuideInterpreter, x0_of


def compose_x0_contract(x, pred, row, weights, masks, *, objective: int, dtype=torch.float32):
    """COMPOSE_X0 over plain tensors in `dtype`: x [B, n], pred [(K + 1) B, n] branch-major with the null rows last, row = the step's 8 table
    entries, weights [K, B], masks [K, B, hw] or None (element e reads pixel e % hw).  The branches are accumulated in ascending k."""
    B, n = x.shape
    Kp = weights.shape[0]
    assert pred.shape[0] == (Kp + 1) * B
    x, pred, row, weights = x.to(dtype), pred.to(dtype), row.to(dtype), weights.to(dtype)
    nul = pred[Kp * B:]
    out = nul
    for k in range(Kp):
        t = weights[k][:, None]
        if masks is not None:
            hw = masks.shape[-1]
            t = t * masks[k].to(dtype).repeat(1, n // hw)
        out = out + (pred[k * B:(k + 1) * B] - nul) * t
    return x0_of(x, out, row[0], row[1], objective)


class ComposeInterpreter(GuideInterpreter):
    def __init__(self):
        super().__init__()
        self.composes = []          # (K, masks present) of every COMPOSE_X0 launch, in order

    def compose_x0(self, p):
        m = self.mem
        B, n, Kp, hw = p.B, p.n_per_sample, p.K, p.hw
        assert 1 <= Kp <= K["IMAGEN_COMPOSE_MAX"] and hw > 0 and n % hw == 0
        self.composes.append((int(Kp), bool(p.masks)))
        _, row = self._coef_row(p.coef, p.step_ptr)
        masks = m.view(p.masks, f32)[:Kp * B * hw].reshape(Kp, B, hw) if p.masks else None
        x0 = compose_x0_contract(m.view(p.x, f32)[:B * n].reshape(B, n), m.view(p.pred, f32)[:(Kp + 1) * B * n].reshape((Kp + 1) * B, n), row,
                                 m.view(p.weights, f32)[:Kp * B].reshape(Kp, B), masks, objective=p.objective)
        m.view(p.x0, f32)[:B * n].copy_(x0.reshape(-1))
        m.view(p.absx0, f32)[:B * n].copy_(x0.abs().reshape(-1))

    DISPATCH = {**GuideInterpreter.DISPATCH}


ComposeInterpreter.DISPATCH[K["IMAGEN_OP_COMPOSE_X0"]] = ComposeInterpreter.compose_x0
