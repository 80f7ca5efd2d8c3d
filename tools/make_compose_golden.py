#!/usr/bin/env python
"""tests/golden/compose_runs.pt: what the tests of composed prompts (Imagen.sample(compose=[...], compose_mask=)) compare against.

    python tools/make_compose_golden.py            # CPU only, needs nothing outside the repository

Runs of the restatement (tests/fixtures_compose.py: a plain fp32 loop over the oracle's K + 1 forwards per step, combined as
out = nul + sum_k w_k m_k (cond_k - nul), k ascending), every Gaussian draw recorded once per group and shared by its settings and its
plain-CFG twin (the main prompt alone at cond_scale 7.5):

    cascade.ddpm            16^2 -> 32^2, 4 steps:  K = 2 with weights;  one negative weight
    cascade.dpmpp_2m        16^2 -> 32^2, 6 steps:  K = 3 with half-image masks (per-unet and per-sample weights);  the main prompt masked too
    negative_prompt.ddpm    the first unet, K = 2, a negative prompt on the null branch (twin: the negative prompt with plain guidance)
    rect.dpmpp_2m           the first unet at 16 x 24 (image_shapes), K = 3 with the masks resized by the nearest rule

Every run must lie at least DISCRIMINATION bars from its twin, so that no test passes by ignoring the keyword: asserted here, re-asserted by
tests/test_compose_cpu.py from the stored tensors.  The further prompts' weights are 15 .. 60 on embeddings scaled by 4, and -6 for the negated one, for that reason (see tests/fixtures_compose.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fixtures_compose as fc  # noqa: E402
import fixtures_solver as fs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR, DISCRIMINATION = 2e-2, 10


def main():
    torch.set_num_threads(min(4, torch.get_num_threads()))     # (the tiny oracle models only lose time on many threads)
    g = fs.cascade_fixture()
    te, specs, settings = g["text_embeds"], fs.cascade_specs(), fc.settings()
    out, ok = {}, True
    for i, (name, grp) in enumerate(fc.groups().items()):
        print(name)
        noise = fs.memo_noise(601 + i)
        n = grp["stages"]
        steps = fc.STEPS[grp["sampler"]]
        kw = dict(unets=specs[:n], sizes=grp.get("sizes", g["image_sizes"][:n]), text_embeds=te, sampler=grp["sampler"], steps=steps,
                  cond_scale=fc.COND_SCALE, noise_fn=noise, return_all=True, **grp.get("restate", {}))
        twin = [o.clone() for o in fc.compose_sample(compose=None, **kw)]
        runs = {}
        for w in grp["which"]:
            runs[w] = [o.clone() for o in fc.compose_sample(**settings[w], **kw)]
            gap = fc.nerr(runs[w][-1], twin[-1])
            print(f"  {w}: |run - plain CFG| / |plain CFG| = {gap:.3f} ({gap / BAR:.1f} bars)")
            ok = ok and gap > DISCRIMINATION * BAR
        out[name] = dict(noise=dict(noise.draws), twin=twin, runs=runs, steps=steps)
    assert ok, "a run lies less than DISCRIMINATION bars from its plain-CFG twin: raise its weights (tests/fixtures_compose.py)"
    path = os.path.join(GOLDEN, "compose_runs.pt")
    torch.save(dict(groups=out, cond_scale=fc.COND_SCALE, bar=BAR, discrimination=DISCRIMINATION, generator="tools/make_compose_golden.py"), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
