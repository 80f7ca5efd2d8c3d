"""(CPU) The launch lists of the SAMPLER stages are pinned: the per-step plan(s) a stage replays, its engine's step plan and static plan(s), for
the tiny fixture models under Imagen (DDPM) and ElucidatedImagen (Karras) — guided / unguided, injected / in-kernel noise, inpainting with
resampling, self-conditioning, Unet3D with and without prompt frames, a low-res stage, a cond_images_channels unet — equal
tests/golden/sampler_snapshot.json, recorded from the commit before the sampling driver was restated: per plan the labels in launch order and one
SHA-256 over every op's kind, label, non-pointer fields and the pattern of its pointers (tools/sampler_snapshot.py).

A refactor of the driver or of the planners' shared head keeps this green without touching the fixture; a deliberate change regenerates it
(python tools/sampler_snapshot.py --write)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sampler_snapshot  # noqa: E402


def test_stage_launch_lists_match_the_snapshot():
    new = sampler_snapshot.digest(sampler_snapshot.snapshot())
    with open(sampler_snapshot.FIXTURE) as f:
        old = json.load(f)
    names = set(new["plans"])
    for case in sampler_snapshot.CASES:      # every case of the table, under both samplers but for the DDPM-only ones
        assert f"ddpm.{case}.plan" in names and (case in sampler_snapshot.DDPM_ONLY or {f"karras.{case}.plan", f"karras.{case}.last"} <= names)
    diff = sampler_snapshot.first_difference(old, new)
    assert diff is None, diff
