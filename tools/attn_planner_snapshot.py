"""Launch lists of the attention planner's plans that no other fixture holds in wired form: a unet with linear cross-attention sites, and the
batched time-table pass with the step plan it returns.

    python tools/attn_planner_snapshot.py            # compare the plans this tree builds with tests/golden/attn_planner_snapshot.json
    python tools/attn_planner_snapshot.py --write    # regenerate the fixture (a deliberate change of what these plans launch)

  * `lin64` / `lin32` (tests/fixtures_linxattn.py, Unet(use_linear_cross_attn=...)): the step plan and the static plan of the guided engine;
  * engine.enable_time_table on `lin64` and on the tiny base unet (tests/golden/unet_tiny_base.pt): `tt`, the batched all-steps pass
    (engine._tt_plan: the sites' ctx.self / ctx.cross projections re-emitted over every step's rows), and `step_tt`, the step plan with the
    timestep chain replaced by one STEP_SLICE.

tests/golden/sampler_snapshot.json already holds the `step_tt` of the tiny cascade's engines inside each image stage's `.plan`; it holds no
`_tt_plan` and no linear site.  Records, digest and fixture format are tools/sampler_snapshot.py's (routing_snapshot.wired_records: labels in
launch order + one SHA-256 per plan); tests/test_attn_planner_snapshot.py asserts equality.  The engines are built dry: no GPU.
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import routing_snapshot as rs  # noqa: E402
import sampler_snapshot as ss  # noqa: E402

FIXTURE = os.path.join(rs.GOLDEN, "attn_planner_snapshot.json")
T = 3                                    # rows of the coefficient table enable_time_table is given
TIME_TABLE = ("lin64", "tiny_base")      # the engines that also build their time table
PLANS = ("step", "static", "tt", "step_tt")


def _engine(name: str):
    """The dry guided engine (rows = 2 * batch) of a fixture unet, its static plan built by set_conditioning."""
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.engine import UnetEngine

    if name == "tiny_base":
        g = torch.load(os.path.join(rs.GOLDEN, "unet_tiny_base.pt"), weights_only=False)
        u = Unet(**g["kwargs"]).eval()
        u.load_state_dict(g["state_dict"])
        x, text, mask = g["x"], g["text_embeds"], g["text_mask"]
    else:
        import fixtures_linxattn as lx

        f = lx.unet_record(name)[0]["forward"]
        u, x, text, mask = lx.unet(name), f["x"], f["text_embeds"], f["text_mask"]
    B = x.shape[0]
    eng = UnetEngine(u, 2 * B, B, x.shape[-1], "cpu", dry=True)
    keep = torch.ones(2 * B, dtype=torch.bool)
    keep[B:] = False
    eng.set_conditioning(text_embeds=text, text_mask=mask, keep=keep, lowres_noise_times=None)
    return eng


def snapshot() -> dict:
    """{"<model>.<plan>": [wired record, ...]} over PLANS (`tt` / `step_tt` for the models of TIME_TABLE)."""
    out = {}
    for name in ("lin64", "lin32", "tiny_base"):
        eng = _engine(name)
        if name != "tiny_base":     # (the tiny base unet's step and static plans: tests/golden/routing_wiring.json)
            out[name + ".step"] = rs.wired_records(eng.step_plan)
            (static,) = eng._last_static
            out[name + ".static"] = rs.wired_records(static)
        if name in TIME_TABLE:
            coef = torch.zeros(T, 8)
            coef[:, 6] = torch.tensor([0.3, -0.2, -0.8])
            fast = eng.enable_time_table(coef, torch.ones(1, dtype=torch.int32))
            assert fast is not None
            out[name + ".tt"] = rs.wired_records(eng._tt_plan)
            out[name + ".step_tt"] = rs.wired_records(fast)
    return out


if __name__ == "__main__":
    sys.exit(ss.main(snapshot, FIXTURE, "attention planner launch lists"))
