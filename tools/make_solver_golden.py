#!/usr/bin/env python
"""tests/golden/solver_*: what the tests of the few-step solvers (Imagen.sample(sampler='ddim' | 'dpmpp_2m')) compare against.

    python tools/make_solver_golden.py --launch-list   # only solver_parent_launch_list_abi<N>.json, from THIS tree: run it on the commit
                                                       # BEFORE a change whose no-regression it is to witness
    python tools/make_solver_golden.py                 # solver_runs.pt; CPU only, needs nothing outside the repository

  solver_parent_launch_list_abi15.json   per-step launch lists of both stages of the tiny cascade (tests/golden/sample_tiny_cascade.pt) as a
                                         default sample() builds them, recorded from the commit before the solvers
  solver_runs.pt                         runs of the restatement (tests/fixtures_solver.py: the issue's formulas in decimal arithmetic, applied
                                         in a plain fp32 loop over the oracle's guided forward), every Gaussian draw recorded:
                                         the tiny cascade 16^2 -> 32^2 under dpmpp_2m and ddim (eta 0) at 6 steps, CFG 3; one Unet(self_cond=True)
                                         stage, one Unet3D stage and the cascade's first unet at 16 x 24 under dpmpp_2m at 4 steps

The reference has no such sampler; its ancestral sampler anchors these through ddim at eta = 1 (tests/test_solver_cpu.py)."""
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fixtures_solver as fs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def make_launch_list():
    from imagen_pytorch_amd import _abi, engine

    engine.UnetEngine = functools.partial(engine.UnetEngine, dry=True)
    path = os.path.join(GOLDEN, f"solver_parent_launch_list_abi{_abi.ENUMS['IMAGEN_ABI_VERSION']}.json")
    with open(path, "w") as fh:
        json.dump(fs.launch_lists(), fh, separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def record(seed, **kw):
    noise = fs.memo_noise(seed)
    outs = fs.solver_sample(noise_fn=noise, return_all=True, **kw)
    return dict(noise=dict(noise.draws), outputs=[o.clone() for o in outs])


def main():
    g = fs.cascade_fixture()
    te = g["text_embeds"]
    specs = fs.cascade_specs()
    runs = {}
    for i, (sampler, eta) in enumerate((("dpmpp_2m", 0.0), ("ddim", 0.0))):
        runs[f"cascade.{sampler}"] = record(301 + i, unets=specs, sizes=g["image_sizes"], text_embeds=te, sampler=sampler, steps=fs.STEPS, eta=eta)
    runs["selfcond.dpmpp_2m"] = record(311, unets=[fs.selfcond_spec()], sizes=(16,), text_embeds=te, sampler="dpmpp_2m", steps=4)
    v = fs.load("sample_tiny_video.pt")
    runs["video.dpmpp_2m"] = record(313, unets=[fs.video_spec()], sizes=(v["image_sizes"][0],), text_embeds=v["text_embeds"], sampler="dpmpp_2m",
                                    steps=4, video_frames=v["frames"])
    runs["rect.dpmpp_2m"] = record(317, unets=specs[:1], sizes=((16, 24),), text_embeds=te, sampler="dpmpp_2m", steps=4)
    for k, r in runs.items():
        print(k, [tuple(o.shape) for o in r["outputs"]], f"{len(r['noise'])} draws")
    path = os.path.join(GOLDEN, "solver_runs.pt")
    torch.save(dict(runs=runs, steps=fs.STEPS, cond_scale=fs.COND_SCALE, generator="tools/make_solver_golden.py",
                    weights_from=dict(cascade="sample_tiny_cascade.pt", selfcond="selfcond_image_unet0.pt", video="sample_tiny_video.pt")), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    if "--launch-list" in sys.argv[1:]:
        make_launch_list()
    else:
        main()
