"""CPU: the alignment term of the conv routing (ops.ConvReq.io_ok, the mirror of launch_igemm's predicate).  ops.igemm plans a launch without
running it: an operand that no family's accesses can take has no route, and the 8-byte operands the kernels do take keep theirs."""
import pytest
import torch

from imagen_pytorch_amd import ops


def _plan(Cout, x_off=0, y_ld=None, y_off=0, y_bs_extra=0, x_bs_extra=0, **kw):
    B, H, W, C = 2, 4, 8, 32
    dev = torch.device("cpu")
    pw = ops.pack_weight(torch.zeros(Cout, C, 3, 3), None, dev)
    x = ops.Act(torch.zeros(B * (H * W * C + x_bs_extra) + 64, dtype=torch.float16), B, H, W, C, C, H * W * C + x_bs_extra, x_off)
    ld = y_ld or Cout
    bs = H * W * ld + y_bs_extra
    y = ops.Act(torch.zeros(B * bs + 64, dtype=torch.float16), B, H, W, Cout, ld, bs, y_off)
    return ops.igemm(ops.Plan("route"), x, pw, y, **kw)


def test_aligned_and_eight_byte_operands_are_routed():
    assert _plan(32).cfg >= 0
    p = _plan(20, y_ld=28, y_off=4, y_bs_extra=4)       # Cout % 8 == 4: stored four channels at a time, 8-byte pitches and base
    assert (p.ldy, p.bsy % 8) == (28, 4)
    res = ops.Act(torch.zeros(2 * 32 * 36 + 64, dtype=torch.float16), 2, 4, 8, 32, 36, 32 * 36, 4)
    assert _plan(32, res=res).cfg >= 0                  # a 16-byte output beside an 8-byte residual: the generic epilogues


@pytest.mark.parametrize("kw", [dict(x_off=4), dict(x_bs_extra=4), dict(y_off=4), dict(y_ld=36), dict(y_bs_extra=4)], ids=str)
def test_misaligned_operands_have_no_route(kw):
    with pytest.raises(ValueError, match="no conv family takes"):
        _plan(32, **kw)


def test_two_byte_output_pitch_has_no_route():
    with pytest.raises(ValueError, match="no conv family takes"):
        _plan(20, y_ld=22)


def test_cfg_table_answers_are_those_of_abi15():
    """What the library tells the planner about every tile cfg id — config_info, _config_family, _config_ring, _stage_slots and _lds_bytes (3x3 and
    1x1, stride 1 and 2, every tile shape launchable_shapes tries) — is what the launchers answered when each family still stated its tile table
    and its LDS formula twice (tests/golden/conv_cfg_table_abi15.json, recorded by tools/routing_snapshot.py --write-cfg-table from that library)."""
    import json
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import routing_snapshot

    with open(routing_snapshot.CFG_TABLE_FIXTURE) as f:
        want = json.load(f)
    got = json.loads(json.dumps(routing_snapshot.cfg_table_answers()))
    assert got["num_configs"] == want["num_configs"]
    for g, w in zip(got["rows"], want["rows"]):
        assert g == w, (g["cfg"], [k for k in w if g[k] != w[k]])
    assert len(got["rows"]) == len(want["rows"])
