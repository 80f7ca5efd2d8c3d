"""The plan interpreter (tests/plan_interp_guidance.py) with GUIDE_X0's contract as include/imagen_hip.h states it: the guided evaluation of
CFG_X0 with guidance rescale (mode 1) or adaptive projected guidance (mode 2), as two launches of one struct (phase 0 reduces, phase 1 applies).
TEST INFRASTRUCTURE, never imported by the product.

A subclass: the parents state the base range of the ABI and stay as they are; GUIDE_X0 is a kind of the extension range (_abi.EXT_OP_STRUCT), so
DISPATCH has the parent's entries and one more.  The restatement does its work in phase 1 (from the inputs, as the kernel's apply pass may: the
partials buffer is scratch) and checks in phase 0 only that the partials buffer is there.  `guides` counts the GUIDE_X0 launches by
(mode, phase, cfg)."""
from __future__ import annotations

import torch

from plan_interp import K, f32
from plan_interp_guidance import GuidanceInterpreter

RESCALE, APG = K["IMAGEN_GUIDE_RESCALE"], K["IMAGEN_GUIDE_APG"]


def x0_of(x, e, alpha, sigma, objective: int):
    """CFG_X0's objective formulas on an already combined model output `e`."""
    if objective == 0:
        return (x - sigma * e) / alpha.clamp(min=1e-8)
    return e if objective == 1 else alpha * x - sigma * e


def guide_x0_contract(x, pred, row, *, cfg: int, cond_scale: float, objective: int, mode: int, phi: float = 0.0, eta: float = 0.0,
                      norm_threshold: float = 0.0, momentum: float = 0.0, avg=None, dtype=torch.float32):
    """GUIDE_X0 over plain tensors: x [B, n], pred [2 B, n] (cond rows first), row = the step's 8 table entries, avg [B, n] or None.  The
    elementwise arithmetic runs in `dtype`, the per-sample sums in fp64 (as the kernel's).  Returns (x0 [B, n], the new avg or None)."""
    assert cfg in (1, 2) and mode in (RESCALE, APG), (cfg, mode)
    B = x.shape[0]
    x, pred, row = x.to(dtype), pred.to(dtype), row.to(dtype)
    alpha, sigma = row[0], row[1]
    s = row[7] if cfg == 2 else torch.tensor(cond_scale, dtype=torch.float32).to(dtype)
    cond, nul = pred[:B], pred[B:]
    f64 = torch.float64
    low = lambda v: (v.to(torch.float32) if dtype == torch.float32 else v).to(dtype)[:, None]    # the kernel rounds the per-sample scalars to fp32
    if mode == RESCALE:
        g = nul + (cond - nul) * s
        n = x.shape[1]
        var = lambda v: ((v.to(f64) ** 2).sum(1) / n - (v.to(f64).sum(1) / n) ** 2).clamp(min=0.0)
        vc, vg = var(cond), var(g)
        f = low(torch.where(vg > 0, (vc / vg.clamp(min=1e-300)).sqrt(), torch.ones_like(vg)))
        ph = torch.tensor(phi, dtype=torch.float32).to(dtype)
        out = g if phi == 0.0 else ph * (g * f) + (1 - ph) * g
        return x0_of(x, out, alpha, sigma, objective), None
    dc, du = x0_of(x, cond, alpha, sigma, objective), x0_of(x, nul, alpha, sigma, objective)
    d = dc - du
    if avg is not None:
        d = d + torch.tensor(momentum, dtype=torch.float32).to(dtype) * avg.to(dtype)
    dd, ddc, dcdc = (d.to(f64) ** 2).sum(1), (d.to(f64) * dc.to(f64)).sum(1), (dc.to(f64) ** 2).sum(1)
    r = torch.ones_like(dd)
    if norm_threshold > 0.0:
        thr = torch.tensor(norm_threshold, dtype=torch.float32).to(f64)
        r = torch.where(dd > 0, (thr / dd.clamp(min=1e-300).sqrt()).clamp(max=1.0), r)
    k = torch.where(dcdc > 0, r * ddc / dcdc.clamp(min=1e-300), torch.zeros_like(dd))
    r, k = low(r), low(k)
    dp, par = r * d, k * dc
    etat = torch.tensor(eta, dtype=torch.float32).to(dtype)
    x0 = dc + (s - 1) * ((dp - par) + etat * par)
    return x0, (d if avg is not None else None)


class GuideInterpreter(GuidanceInterpreter):
    def __init__(self):
        super().__init__()
        self.guides = []            # (mode, phase, cfg) of every GUIDE_X0 launch, in order

    def guide_x0(self, p):
        m = self.mem
        B, n = p.B, p.n_per_sample
        self.guides.append((int(p.mode), int(p.phase), int(p.cfg)))
        assert m.view(p.partials, torch.float64).numel() >= B * K["IMAGEN_GUIDE_PARTIAL_DOUBLES"]
        if p.phase == 0:
            return
        _, row = self._coef_row(p.coef, p.step_ptr)
        avg = m.view(p.avg, f32)[:B * n].reshape(B, n) if p.avg else None
        x0, new_avg = guide_x0_contract(m.view(p.x, f32)[:B * n].reshape(B, n), m.view(p.pred, f32)[:2 * B * n].reshape(2 * B, n), row, cfg=p.cfg,
                                        cond_scale=p.cond_scale, objective=p.objective, mode=p.mode, phi=p.phi, eta=p.eta,
                                        norm_threshold=p.norm_threshold, momentum=p.momentum, avg=avg)
        m.view(p.x0, f32)[:B * n].copy_(x0.reshape(-1))
        m.view(p.absx0, f32)[:B * n].copy_(x0.abs().reshape(-1))
        if avg is not None:
            avg.copy_(new_avg)

    DISPATCH = {**GuidanceInterpreter.DISPATCH}


GuideInterpreter.DISPATCH[K["IMAGEN_OP_GUIDE_X0"]] = GuideInterpreter.guide_x0
