#!/usr/bin/env python
"""tests/golden/guide_runs.pt: what the tests of guidance rescale and projected guidance (Imagen.sample(guidance_rescale=, guidance_apg=))
compare against.

    python tools/make_guide_golden.py            # CPU only, needs nothing outside the repository

Runs of the restatement (tests/fixtures_guide.py: a plain fp32 loop over the oracle's conditional and null forwards that applies GUIDE_X0's
formulas per guided step, fp64 sums), every Gaussian draw recorded once per model and sampler and shared by its settings: the tiny cascade
16^2 -> 32^2 under ddpm (4 steps), dpmpp_2m and ddim (6 steps) with rescale (phi 0.7) and with projected guidance (eta 0, a norm threshold,
momentum -0.5), and its plain-CFG twin (7.5); one v-objective stage with rescale, one Unet(self_cond=True) stage, one Unet3D stage, the
cascade's first unet at 16 x 24, and one run with a negative prompt and a guidance interval.

Every run must lie at least DISCRIMINATION bars from its plain-CFG twin, so that no test passes by ignoring the keyword: asserted here,
re-asserted by tests/test_guide_cpu.py from the stored tensors."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fixtures_guidance as fg  # noqa: E402
import fixtures_guide as fgd  # noqa: E402
import fixtures_solver as fs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR, DISCRIMINATION = 2e-2, 10


def group(seed, settings, steps, n_stages, interval=False, **kw):
    """One model under one sampler: the plain-CFG twin and every setting of `settings`, from the same draws."""
    noise = fs.memo_noise(seed)
    scales = [fg.scales_of("interval", steps) if interval else [fgd.COND_SCALE] * steps] * n_stages
    twin = [o.clone() for o in fgd.guide_sample(noise_fn=noise, steps=steps, scales=scales, guides=[None] * n_stages, return_all=True, **kw)]
    runs = {}
    for w in settings:
        caps = []
        runs[w] = [o.clone() for o in fgd.guide_sample(noise_fn=noise, steps=steps, scales=scales, guides=[fgd.SETTINGS[w]] * n_stages, return_all=True,
                                                       caps=caps, **kw)]
        gap = fgd.nerr(runs[w][-1], twin[-1])
        bind = f", |D| per guided step {[round(c, 2) for c in caps]} against the threshold {fgd.APG[2]}" if caps else ""
        print(f"  {w}: |run - plain CFG| / |plain CFG| = {gap:.3f} ({gap / BAR:.1f} bars){bind}")
        assert gap > DISCRIMINATION * BAR, (w, gap)
    return dict(noise=dict(noise.draws), twin=twin, runs=runs, steps=steps)


def main():
    torch.set_num_threads(min(4, torch.get_num_threads()))     # (the tiny oracle models only lose time on many threads)
    g = fs.cascade_fixture()
    te, specs = g["text_embeds"], fs.cascade_specs()
    groups = {}
    for i, sampler in enumerate(("ddpm", "dpmpp_2m", "ddim")):
        print(f"cascade.{sampler}")
        groups[f"cascade.{sampler}"] = group(501 + i, ("rescale", "apg"), fgd.STEPS[sampler], 2, unets=specs, sizes=g["image_sizes"], text_embeds=te,
                                             sampler=sampler)
    for i, (name, v) in enumerate(fgd.variants().items()):
        print(name)
        groups[name] = group(511 + i, (v["which"],), v["steps"], 1, interval=v.get("interval", False), unets=v["unets"], sizes=v["sizes"],
                             text_embeds=v["te"], sampler=v["sampler"], **v.get("restate", {}))
    path = os.path.join(GOLDEN, "guide_runs.pt")
    torch.save(dict(groups=groups, cond_scale=fgd.COND_SCALE, rescale=fgd.RESCALE, apg=fgd.APG, bar=BAR, discrimination=DISCRIMINATION,
                    generator="tools/make_guide_golden.py"), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
