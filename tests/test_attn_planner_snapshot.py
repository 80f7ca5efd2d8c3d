"""(CPU) The plans of the attention planner that the routing and sampler snapshots leave out are pinned in wired form: the step and static
plans of the linear cross-attention fixture unets (`lin64`, `lin32`), and engine.enable_time_table's batched all-steps pass (`_tt_plan`)
with the step plan it returns, on `lin64` and on the tiny base unet — equal tests/golden/attn_planner_snapshot.json, recorded from the
planner of the commit before the attention sites became records and the five attention chains one skeleton (twice, identically): per plan
the labels in launch order and one SHA-256 over every op's kind, label, non-pointer fields and the pattern of its pointers
(tools/attn_planner_snapshot.py, in the format of tools/sampler_snapshot.py).

tests/golden/sampler_snapshot.json already holds the returned step plan of the tiny cascade's engines inside its stage plans; it holds neither
a `_tt_plan` nor a linear site, so nothing here repeats it.

A refactor of the planner keeps this green without touching the fixture; a deliberate change regenerates it
(python tools/attn_planner_snapshot.py --write)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import attn_planner_snapshot as aps  # noqa: E402
import sampler_snapshot  # noqa: E402


def test_linear_site_and_time_table_plans_match_the_snapshot():
    new = sampler_snapshot.digest(aps.snapshot())
    with open(aps.FIXTURE) as f:
        old = json.load(f)
    want = [f"{m}.{p}" for m in ("lin64", "lin32") for p in ("step", "static")] + [f"{m}.{p}" for m in aps.TIME_TABLE for p in ("tt", "step_tt")]
    assert sorted(new["plans"]) == sorted(want)
    labels = lambda name: [new["labels"][i] for i in new["plans"][name]["ops"]]
    assert "linctx" in labels("lin64.step_tt") and "tt.ctx.cross" in labels("lin64.tt") and "tt.ctx.self" in labels("tiny_base.tt")
    diff = sampler_snapshot.first_difference(old, new)
    assert diff is None, diff
