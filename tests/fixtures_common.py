"""What the fixture modules (tests/fixtures_*.py) share: the golden directory, a cached loader, the reader of a flat-fp16 unet record and the
normwise relative error.  TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_cache = {}


def load(name):
    """tests/golden/<name>, loaded once."""
    if name not in _cache:
        _cache[name] = torch.load(os.path.join(GOLDEN, name), weights_only=False)
    return _cache[name]


def unpack_state_dict(spec):
    """{key: fp32 tensor} in state_dict order from a unet record (one flat fp16 tensor + the ordered (key, shape) index)."""
    sd, at = {}, 0
    for key, shape in spec["index"]:
        n = 1
        for d in shape:
            n *= d
        sd[key] = spec["flat"][at:at + n].float().reshape(shape)
        at += n
    assert at == spec["flat"].numel()
    return sd


def nerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm())
