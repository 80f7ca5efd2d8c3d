"""(CPU) The launch lists of the denoiser plans are pinned: the step / static plans of README unet1 and unet2, BASELINE C2, a merged-request
batch, the C5 video unet and the two tiny golden unets equal tests/golden/routing_snapshot.json, op by op and in order.  Of every IGEMM, ROWCHAIN,
ACT_PREP and GCA_* op the fixture holds kind, label, every non-pointer field of its params struct, the null-ness of every pointer field and what
ops.igemm() told its caller; the ops of the other kinds (and the position of every op) are held by one SHA-256 per plan over the same records.

tests/golden/routing_wiring.json pins what that fixture leaves out, which buffer every pointer field names: one SHA-256 per plan over the
same records with the pointers as ordinals of first use, recorded from the commit before the ResnetBlock planner was restated.

A refactor of the routing (ops.route, pick_cfg, the engines' planners) keeps this green without touching the fixture.  A deliberate routing
change regenerates it (python tools/routing_snapshot.py --write): the fixture's diff is then the list of launches that moved.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import routing_snapshot  # noqa: E402


def test_launch_lists_match_the_snapshot():
    wiring = {}
    new = routing_snapshot.snapshot(wiring)
    old = routing_snapshot.load()
    fams, modes = routing_snapshot.coverage(new)
    # the snapshot must keep exercising every gate: each kernel family and each ROWCHAIN mode at least once over all plans
    assert fams >= {0, 2, 3, 4, 5, 6, 7, 8}, sorted(fams)
    assert modes >= {1, 2, 3, 4}, sorted(modes)
    diff = routing_snapshot.first_difference(old, new)
    if diff:
        print(diff)
    assert diff is None, diff
    # ... and the buffer wiring of the same plans (pointer fields as ordinals of first use, one SHA-256 per plan), from the same engines
    with open(routing_snapshot.WIRING_FIXTURE) as f:
        pinned = json.load(f)
    assert list(pinned) == list(wiring)
    moved = [name for name in pinned if pinned[name] != wiring[name]]
    assert not moved, f"same launch lists, but the buffer wiring changed in {moved}"
