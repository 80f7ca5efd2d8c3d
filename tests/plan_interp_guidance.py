"""The plan interpreter (tests/plan_interp.py) with CFG_X0's contract as include/imagen_hip.h states it since guidance schedules: cfg == 2 reads
the scale from column 7 of the step's table row, the immediate `cond_scale` is not used.  TEST INFRASTRUCTURE, never imported by the product.

A subclass: the parent class states the contract the default calls use (cfg 0 / 1) and stays as it is; no op kind is new, so DISPATCH has the
parent's entries with CFG_X0's replaced.  `launches` counts the CFG_X0 launches by (cfg, rows of pred): which plan a step replayed."""
from __future__ import annotations

import torch

from plan_interp import Interpreter, K, f32


def cfg_x0_contract(x, pred, row, *, cfg: int, cond_scale: float, objective: int, dtype=torch.float32):
    """CFG_X0 over plain tensors in `dtype`: x [n], pred [2 n] (cond first) where cfg != 0 else [n], row = the step's 8 table entries."""
    assert cfg in (0, 1, 2), cfg
    n = x.numel()
    x, pred, row = x.to(dtype), pred.to(dtype), row.to(dtype)
    alpha, sigma = row[0], row[1]
    if cfg:
        s = row[7] if cfg == 2 else torch.tensor(cond_scale, dtype=torch.float32).to(dtype)
        out = pred[n:] + (pred[:n] - pred[n:]) * s
    else:
        out = pred
    if objective == 0:
        return (x - sigma * out) / alpha.clamp(min=1e-8)
    return out if objective == 1 else alpha * x - sigma * out


class GuidanceInterpreter(Interpreter):
    def __init__(self):
        super().__init__()
        self.launches = []          # (cfg, rows) of every CFG_X0 launch, in order

    def cfg_x0(self, p):
        m = self.mem
        n = p.B * p.n_per_sample
        _, row = self._coef_row(p.coef, p.step_ptr)
        x0 = cfg_x0_contract(m.view(p.x, f32)[:n], m.view(p.pred, f32)[: (2 * n if p.cfg else n)], row, cfg=p.cfg, cond_scale=p.cond_scale,
                             objective=p.objective)
        m.view(p.x0, f32)[:n].copy_(x0)
        m.view(p.absx0, f32)[:n].copy_(x0.abs())
        self.launches.append((int(p.cfg), 2 * p.B if p.cfg else p.B))

    DISPATCH = {**Interpreter.DISPATCH}


GuidanceInterpreter.DISPATCH[K["IMAGEN_OP_CFG_X0"]] = GuidanceInterpreter.cfg_x0
