#!/usr/bin/env python
"""tests/golden/tile_runs.pt: what the tests of tiled sampling (Imagen.sample(tile_shapes=, tile_overlap=, tile_blend=)) compare against.

    python tools/make_tile_golden.py            # CPU only, needs nothing outside the repository

Runs of the restatement (tests/fixtures_tile.py: per step and tile the oracle's guided forward on the canvas crop, CFG_X0's x0 expression, the
blend in fp64, the dynamic threshold and the restated solver row on the canvas) on the tiny cascade at 16 x 48 -> 32 x 96 with 16 x 16 tiles at
overlap 4 on both stages (T = 4, then 24), every Gaussian draw recorded once (tests/golden/tile_noise.pt) and shared by the runs and their
untiled twins (the same canvas through image_shapes alone; tests/golden/tile_twins.pt):

    ddpm.ramp, ddpm.uniform                  4 steps
    dpmpp_2m.ramp, dpmpp_2m.uniform          6 steps
    dpmpp_2m.ramp.negative                   6 steps, a negative prompt on the null branch

Every stage of every run must lie at least DISCRIMINATION bars from its twin's, so that no test passes by ignoring the keywords: asserted here,
re-asserted by tests/test_tiles_cpu.py from the stored tensors."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fixtures_solver as fs  # noqa: E402
import fixtures_tile as ft  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR, DISCRIMINATION = 2e-2, 10


def main():
    torch.set_num_threads(min(4, torch.get_num_threads()))     # (the tiny oracle models only lose time on many threads)
    out, twins, ok = {}, {}, True
    noise = fs.memo_noise(701)                                 # one set of draws for every run and twin: the tags and shapes are the same
    for name, grp in ft.groups().items():
        steps = ft.STEPS[grp["sampler"]]
        twin = [o.clone() for o in ft.restate(grp, steps, noise, tiled=False)]
        run = [o.clone() for o in ft.restate(grp, steps, noise)]
        gaps = [ft.nerr(r, t) for r, t in zip(run, twin)]
        print(f"{name}: |tiled - untiled| / |untiled| per stage = {[f'{g:.3f}' for g in gaps]} ({', '.join(f'{g / BAR:.1f}' for g in gaps)} bars)")
        ok = ok and min(gaps) > DISCRIMINATION * BAR
        out[name] = dict(run=run, steps=steps, gaps=gaps)
        twins[name] = twin
    assert ok, "a run lies less than DISCRIMINATION bars from its untiled twin: change the overlap or the canvas (tests/fixtures_tile.py)"
    path = os.path.join(GOLDEN, "tile_runs.pt")
    torch.save(dict(groups=out, cond_scale=ft.COND_SCALE, shapes=ft.SHAPES, tiles=ft.TILES, overlaps=ft.OVERLAPS, bar=BAR,
                    discrimination=DISCRIMINATION, generator="tools/make_tile_golden.py"), path)
    npath = os.path.join(GOLDEN, "tile_noise.pt")
    torch.save(dict(noise=dict(noise.draws), generator="tools/make_tile_golden.py"), npath)
    tpath = os.path.join(GOLDEN, "tile_twins.pt")
    torch.save(dict(twins=twins, generator="tools/make_tile_golden.py"), tpath)
    for p in (path, npath, tpath):
        print(f"wrote {p} ({os.path.getsize(p)} bytes)")
        assert os.path.getsize(p) < (1 << 20)


if __name__ == "__main__":
    main()
