#!/usr/bin/env python
"""tests/golden/guidance_*: what the tests of the guidance schedules (Imagen.sample(guidance_schedule=, guidance_interval=)) compare against.

    python tools/make_guidance_golden.py                     # guidance_runs.pt; CPU only, needs nothing outside the repository
    IMAGEN_LIB_PATH=<the PARENT commit's libimagen_hip.so> python tools/make_guidance_golden.py --kernel [--out FILE]
                                                             # guidance_cfg_x0_parent.pt, on an MI355X: what the kernel library of the commit
                                                             # BEFORE cfg == 2 gives for CFG_X0 at cfg 0 / 1 on fixed inputs

  guidance_runs.pt            runs of the restatement (tests/fixtures_guidance.py: one scale per step, a plain fp32 loop over the oracle's
                              guided forward; scale 1 is the conditional forward alone), every Gaussian draw recorded once per model and
                              sampler and shared by its schedules: the tiny cascade 16^2 -> 32^2 under ddpm (4 steps), dpmpp_2m and ddim
                              (6 steps) with a ramp and with an interval, and its constant-scale twin (CFG 7.5); one Unet(self_cond=True)
                              stage under ddpm (a steeper ramp, interval) and dpmpp_2m (a sequence that switches guided / unguided every step), one
                              Unet3D stage and the cascade's first unet at 16 x 24 with the interval
  guidance_cfg_x0_parent.pt   inputs (seeded) and the parent library's x0 / |x0| for the three objectives at cfg 0 and 1

Every scheduled run must lie at least DISCRIMINATION bars from its constant-scale twin, so that no test passes by ignoring the schedule:
asserted here, re-asserted by tests/test_guidance_cpu.py from the stored tensors."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import fixtures_guidance as fg  # noqa: E402
import fixtures_solver as fs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR, DISCRIMINATION = 2e-2, 10


def record(noise, which, steps, n_stages, **kw):
    scales = [fg.scales_of(which, steps)] * n_stages if which != "constant" else [[fg.COND_SCALE] * steps] * n_stages
    outs = fg.guided_sample(noise_fn=noise, steps=steps, scales=scales, return_all=True, **kw)
    return [o.clone() for o in outs]


def group(seed, schedules, steps, **kw):
    """One model under one sampler: the constant-scale twin and every schedule of `schedules`, from the same draws."""
    noise = fs.memo_noise(seed)
    n = len(kw["unets"])
    twin = record(noise, "constant", steps, n, **kw)
    runs = {w: record(noise, w, steps, n, **kw) for w in schedules}
    for w, outs in runs.items():
        gap = fg.nerr(outs[-1], twin[-1])
        print(f"  {w}: |scheduled - constant| / |constant| = {gap:.3f} ({gap / BAR:.1f} bars)")
        assert gap > DISCRIMINATION * BAR, (w, gap)
    return dict(noise=dict(noise.draws), twin=twin, runs=runs, steps=steps)


def main():
    torch.set_num_threads(min(4, torch.get_num_threads()))     # (the tiny oracle models only lose time on many threads)
    g = fs.cascade_fixture()
    te, specs = g["text_embeds"], fs.cascade_specs()
    groups = {}
    for i, sampler in enumerate(("ddpm", "dpmpp_2m", "ddim")):
        print(f"cascade.{sampler}")
        groups[f"cascade.{sampler}"] = group(401 + i, ("ramp", "interval"), fg.STEPS[sampler], unets=specs, sizes=g["image_sizes"], text_embeds=te,
                                             sampler=sampler)
    print("selfcond.ddpm")
    groups["selfcond.ddpm"] = group(411, ("steep", "interval"), 4, unets=[fs.selfcond_spec()], sizes=(16,), text_embeds=te, sampler="ddpm")
    print("selfcond.dpmpp_2m")
    groups["selfcond.dpmpp_2m"] = group(412, ("switch",), 4, unets=[fs.selfcond_spec()], sizes=(16,), text_embeds=te, sampler="dpmpp_2m")
    v = fs.load("sample_tiny_video.pt")
    print("video.ddpm")
    groups["video.ddpm"] = group(413, ("interval",), 4, unets=[fs.video_spec()], sizes=(v["image_sizes"][0],), text_embeds=v["text_embeds"],
                                 sampler="ddpm", video_frames=v["frames"])
    print("rect.dpmpp_2m")
    groups["rect.dpmpp_2m"] = group(417, ("interval",), 4, unets=specs[:1], sizes=((16, 24),), text_embeds=te, sampler="dpmpp_2m")
    path = os.path.join(GOLDEN, "guidance_runs.pt")
    torch.save(dict(groups=groups, cond_scale=fg.COND_SCALE, bar=BAR, discrimination=DISCRIMINATION, generator="tools/make_guidance_golden.py",
                    weights_from=dict(cascade="sample_tiny_cascade.pt", selfcond="selfcond_image_unet0.pt", video="sample_tiny_video.pt")), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


def kernel_inputs(B=2, n=1540, steps=5):
    """Seeded inputs of the CFG_X0 cases: n is no multiple of the 256-thread block and spans several; a table of `steps` rows."""
    g = torch.Generator().manual_seed(431)
    coef = torch.rand(steps, 8, generator=g) * 0.9 + 0.05
    return dict(x=torch.randn(B, n, generator=g), pred=torch.randn(2 * B, n, generator=g), coef=coef, B=B, n=n, steps=steps, cond_scale=3.0, step=2)


def run_cfg_x0(inp, *, cfg, objective, cond_scale, step, coef=None, device="cuda"):
    """One CFG_X0 launch through ops; returns (x0, |x0|) on the CPU."""
    from imagen_pytorch_amd import ops

    dev = torch.device(device)
    B, n = inp["B"], inp["n"]
    x, pred = inp["x"].to(dev), inp["pred"].to(dev)
    coef = (inp["coef"] if coef is None else coef).to(dev).contiguous()
    step_ptr = torch.tensor([step], dtype=torch.int32, device=dev)
    x0, absx0 = torch.full((B, n), float("nan"), device=dev), torch.full((B, n), float("nan"), device=dev)
    plan = ops.Plan("cfg_x0")
    ops.cfg_x0(plan, x, pred, coef, step_ptr, x0, absx0, B=B, n_per_sample=n, cfg=cfg, cond_scale=cond_scale, objective=objective)
    plan.run()
    torch.cuda.synchronize()
    return x0.cpu(), absx0.cpu()


def kernel(out):
    assert os.environ.get("IMAGEN_LIB_PATH"), "point IMAGEN_LIB_PATH at the parent commit's kernel library"
    inp = kernel_inputs()
    rec = {}
    for objective in ("noise", "x_start", "v"):
        for cfg in (0, 1):
            rec[(objective, cfg)] = run_cfg_x0(inp, cfg=bool(cfg), objective=objective, cond_scale=inp["cond_scale"], step=inp["step"])
    torch.save(dict(outputs=rec, library=os.path.basename(os.environ["IMAGEN_LIB_PATH"]), generator="tools/make_guidance_golden.py --kernel"), out)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    if "--kernel" in sys.argv[1:]:
        kernel(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(GOLDEN, "guidance_cfg_x0_parent.pt"))
    else:
        main()
