"""Bit-equality of the sampling driver between two trees: a fixed list of tiny `sample*()` calls on the fixture models of tests/golden, and per
call the SHA-256 of every returned tensor plus the run log — the ordered (plan name, number of ops) of every `Plan.run` and graph launch, the
warm-up included.  A refactor of the driver must leave both equal; there is no tolerance.

    python tools/sampler_digests.py --mode cpu --out profiles/sampler_stage_bits_head_cpu.json
    python tools/sampler_digests.py --mode gpu --tree ../parent --out profiles/sampler_stage_bits_parent_gpu.json
    python tools/sampler_digests.py --compare profiles/sampler_stage_bits_parent_cpu.json profiles/sampler_stage_bits_head_cpu.json
    python tools/sampler_digests.py --mode refusals --out profiles/sample_call_refusals_head.json

--tree: the checkout whose `imagen_pytorch_amd` is sampled (default: this one); the tool, the fixtures and the interpreter are this tree's, and
the sampled tree is used through `sample()`, `sample_requests()` and `sample_pipelined()` alone.
--mode cpu: injected noise (`noise_fn`, drawn from the tag) through the plan interpreter, with the patches of tests/cpu_replay.py; the
interpreter has no in-kernel noise, so `sample_requests` is left to the other mode.  --mode gpu: the in-kernel Philox path with a fixed seed.
--mode refusals: no digests — the fixed list of malformed and out-of-scope calls of tools/sampler_refusals.py, per call the exception type and its
full message; nothing is built or launched.  --compare takes these files too; --expect names the cases an intended change makes differ.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import json
import os
import sys
import threading
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, SEED = 4, 20240229


def _noise(scale=1.0):
    """noise_fn: a standard normal draw that depends on the tag and the shape alone."""
    def fn(tag, shape):
        g = torch.Generator().manual_seed(zlib.crc32(repr((tag, tuple(shape))).encode()))
        return torch.randn(tuple(shape), generator=g) * scale
    return fn


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def cases(mode: str):
    """[(case name, model key, method name, args, keywords)]; a model key = (fixture model of tools/sampler_snapshot.py, Karras?) names ONE
    model for the whole list, so later calls meet the stages earlier ones cached."""
    import sampler_snapshot as ss

    img, vid = ss._load("sample_tiny_cascade.pt"), ss._load("sample_tiny_video.pt")
    te, vte = img["text_embeds"], vid["text_embeds"]
    s0, s1 = img["image_sizes"]
    B = te.shape[0]
    neg = dict(negative_text_embeds=te.flip(0) * 0.5)
    paint = dict(inpaint_images=_rand(1, B, 3, s1, s1), inpaint_masks=_rand(2, B, s1, s1) > 0.5, inpaint_resample_times=2)
    video = dict(text_embeds=vte, video_frames=vid["frames"])
    D, K, kw = ("image", False), ("image", True), dict(text_embeds=te, cond_scale=3.0)
    left = (torch.arange(s0) < s0 // 2).float().expand(s0, s0)                       # the left half of the image, [H, W]
    compose = [dict(text_embeds=te.flip(0) * 0.75, weight=(1.5, -0.5), mask=left[None]), dict(text_embeds=te[:1] * 1.25, weight=0.5)]
    batches = lambda: [dict(text_embeds=te * (1.0 + 0.1 * i)) for i in range(2)]
    out = [
        ("ddpm.guided", D, "sample", dict(kw, return_all_unet_outputs=True)),
        ("ddpm.unguided", D, "sample", dict(kw, cond_scale=1.0)),
        ("ddpm.guided.cached", D, "sample", dict(kw, return_all_unet_outputs=True)),
        ("ddpm.start_at_2", D, "sample", dict(kw, start_at_unet_number=2, start_image_or_video=_rand(3, B, 3, s0, s0))),
        ("ddpm.sample_offset", D, "sample", dict(kw, sample_offset=3)),
        ("ddpm.negative", D, "sample", dict(kw, **neg)),
        ("ddpm.init_skip", D, "sample", dict(kw, init_images=_rand(4, B, 3, s0, s0), skip_steps=1)),
        ("ddpm.inpaint", D, "sample", dict(kw, **paint)),
        ("ddpm.self_cond", ("self_cond", False), "sample", kw),
        ("ddpm.ddim", D, "sample", dict(kw, sampler="ddim", sample_steps=3)),
        ("ddpm.ddim_eta", D, "sample", dict(kw, sampler="ddim", sample_steps=3, eta=0.5)),
        ("ddpm.dpmpp_2m", D, "sample", dict(kw, sampler="dpmpp_2m", sample_steps=3)),
        ("ddpm.dpmpp_2m.skip1", D, "sample", dict(kw, sampler="dpmpp_2m", sample_steps=3, skip_steps=1)),
        ("ddpm.dpmpp_2m.skip2", D, "sample", dict(kw, sampler="dpmpp_2m", sample_steps=3, skip_steps=2)),
        ("ddpm.guidance_ramp", D, "sample", dict(kw, guidance_schedule=[3.0, 2.5, 2.0, 1.5])),
        ("ddpm.guidance_interval", D, "sample", dict(kw, guidance_interval=(0.3, 0.8))),
        ("ddpm.guidance_interval.dpmpp_2m", D, "sample", dict(kw, guidance_interval=(0.3, 0.8), sampler="dpmpp_2m", sample_steps=T)),
        ("karras.plain", K, "sample", dict(kw, return_all_unet_outputs=True)),
        ("karras.sigmas", K, "sample", dict(kw, sigma_min=0.01, sigma_max=40.0)),
        ("karras.inpaint", K, "sample", dict(kw, **paint)),
        ("karras.self_cond", ("self_cond", True), "sample", kw),
        ("karras.skip_last", K, "sample", dict(kw, skip_steps=T - 1)),
        ("ddpm.video", ("video", False), "sample", dict(video, cond_scale=3.0)),
        ("karras.video", ("video", True), "sample", dict(video, cond_scale=3.0)),
        ("ddpm.pipelined", D, "sample_pipelined", ([dict(text_embeds=te * (1.0 + 0.1 * i)) for i in range(3)],), dict(cond_scale=3.0)),
        ("ddpm.eager", D, "sample", dict(kw, use_graph=False)),
        ("karras.eager", K, "sample", dict(kw, use_graph=False)),
        # guidance rescale, projected guidance and composed prompts, through sample() and through the sample_pipelined pre-flight
        ("ddpm.rescale", D, "sample", dict(kw, guidance_rescale=0.7)),
        ("ddpm.apg_momentum", D, "sample", dict(kw, guidance_apg=dict(eta=0.5, norm_threshold=2.0, momentum=-0.5))),
        ("ddpm.apg_interval", D, "sample", dict(kw, guidance_apg=dict(momentum=-0.25), guidance_interval=(0.3, 0.8))),
        ("ddpm.compose", D, "sample", dict(kw, compose=compose, compose_mask=1.0 - left)),
        ("ddpm.negative_schedule", D, "sample", dict(kw, cond_scale=1.0, guidance_schedule=[3.0, 2.5, 2.0, 1.5], **neg)),
        ("ddpm.pipelined.negative", D, "sample_pipelined", (batches(),), dict(cond_scale=3.0, **neg)),
        ("ddpm.pipelined.rescale", D, "sample_pipelined", (batches(),), dict(cond_scale=3.0, guidance_rescale=(0.7, 0.3))),
        ("ddpm.pipelined.compose", D, "sample_pipelined", (batches(),), dict(cond_scale=3.0, compose=compose, compose_mask=1.0 - left)),
    ]
    if mode == "gpu":
        requests = lambda: [dict(text_embeds=te[:1], seed=SEED + 1), dict(text_embeds=te[1:], seed=SEED + 2, **{k: v[1:] for k, v in neg.items()})]
        out.insert(-10, ("ddpm.requests", D, "sample_requests", (requests(),), dict(cond_scale=3.0)))
        out.append(("ddpm.requests.rescale_negative", D, "sample_requests", (requests(),), dict(cond_scale=3.0, guidance_rescale=0.7)))
    return [c if len(c) == 5 else (*c[:3], (), c[3]) for c in out]


def _to(v, device):
    if torch.is_tensor(v):
        return v.to(device)
    if isinstance(v, (list, tuple)) and not all(isinstance(e, (int, float)) for e in v):
        return type(v)(_to(e, device) for e in v)
    return {k: _to(e, device) for k, e in v.items()} if isinstance(v, dict) else v


def _digests(out) -> list:
    if torch.is_tensor(out):
        t = out.detach().cpu().contiguous()
        return [f"{str(t.dtype)[6:]}{list(t.shape)}:{hashlib.sha256(t.numpy().tobytes()).hexdigest()}"]
    return [d for o in out for d in _digests(o)]


@contextlib.contextmanager
def _run_log(log: dict, one_at_a_time: bool = False):
    """Every Plan.run and Graph.launch appends (plan name, number of ops) to the list of the calling thread.  one_at_a_time: the plan
    interpreter keeps one table of the storages it has seen, so the stage workers of sample_pipelined take turns at it."""
    from imagen_pytorch_amd import ops

    run, launch = ops.Plan.run, ops.Graph.launch
    note = lambda plan: log.setdefault(threading.get_ident(), []).append([plan.name, len(plan.ops)])

    turn = threading.Lock() if one_at_a_time else contextlib.nullcontext()

    def logged_run(self, stream=None):
        note(self)
        with turn:
            return run(self, stream)

    def logged_launch(self):
        note(self.plan)
        return launch(self)

    ops.Plan.run, ops.Graph.launch = logged_run, logged_launch
    try:
        yield
    finally:
        ops.Plan.run, ops.Graph.launch = run, launch


def collect(mode: str) -> dict:
    import sampler_snapshot as ss

    device = "cpu" if mode == "cpu" else "cuda"
    models, result = {}, {}
    for name, mkey, method, args, kw in cases(mode):
        if mkey not in models:
            models[mkey] = ss._model(*mkey).to(device)
        args, kw = _to(args, device), dict(_to(kw, device), use_tqdm=False)
        if mode == "cpu":
            kw.update(device="cpu")
            if method == "sample_pipelined":
                for i, b in enumerate(args[0]):
                    b["noise_fn"] = _noise(1.0 - 0.25 * i)
            else:
                kw["noise_fn"] = _noise()
        elif method == "sample_pipelined":
            for i, b in enumerate(args[0]):
                b["seed"] = SEED + 10 + i
        elif method == "sample":
            kw["seed"] = SEED
        log = {}
        with _run_log(log, one_at_a_time=mode == "cpu"):
            out = getattr(models[mkey], method)(*args, **kw)
        if mode == "gpu":
            torch.cuda.synchronize()
        # (the stage workers of sample_pipelined run side by side: one ordered log per thread, the logs in sorted order)
        runs = sorted(log.values()) if method == "sample_pipelined" else [r for v in log.values() for r in v]
        result[name] = {"digests": _digests(out), "runs": runs}
        print(f"{name}: {len(result[name]['digests'])} tensors, {sum(len(v) for v in log.values())} launches", flush=True)
    return result


def compare(a_path: str, b_path: str, expect=()) -> int:
    """Equal but for the cases of `expect`, which must differ: those are printed with both outcomes."""
    a, b = (json.load(open(p))["cases"] for p in (a_path, b_path))
    differ = [n for n in sorted(set(a) | set(b)) if a.get(n) != b.get(n)]
    bad = sorted(set(differ) ^ set(expect))
    for n in differ:
        if n in expect:
            print(f"{n}: differs as expected\n    {json.dumps(a.get(n))}\n    {json.dumps(b.get(n))}")
        else:
            what = "missing" if n not in a or n not in b else "outcome" if "digests" not in a[n] else \
                "digests" if a[n]["digests"] != b[n]["digests"] else "run log"
            print(f"{n}: {what} differ")
    for n in set(expect) - set(differ):
        print(f"{n}: expected to differ, is equal")
    everything = "every outcome equal" if a and "digests" not in next(iter(a.values())) else "every digest and every run log equal"
    print(f"{len(a)} / {len(b)} cases, " + (f"{len(bad)} differ unexpectedly" if bad else everything + (f" but the {len(expect)} expected" if expect else "")))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("cpu", "gpu", "refusals"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is sampled")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--expect", nargs="*", default=(), metavar="CASE", help="with --compare: the cases that are to differ (an intended change)")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare, expect=args.expect)
    assert args.mode and args.out, "--mode and --out"
    tree = os.path.abspath(args.tree)
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), tree):      # (the sampled tree first on the path)
        sys.path.insert(0, p)
    import imagen_pytorch_amd       # (before any other module of this tree puts its own root on the path)

    assert os.path.abspath(imagen_pytorch_amd.__file__).startswith(tree + os.sep), imagen_pytorch_amd.__file__
    if args.mode == "cpu":
        import cpu_replay
        from plan_interp_compose import ComposeInterpreter        # (the superset interpreter: CFG_X0 at cfg == 2, GUIDE_X0, COMPOSE_X0)

        with cpu_replay.cpu_backend(ComposeInterpreter()):
            result = collect("cpu")
    elif args.mode == "refusals":
        import cpu_replay
        import sampler_refusals

        with cpu_replay.cpu_backend(sampler_refusals.NoLaunch()):
            result = sampler_refusals.collect()
    else:
        result = collect("gpu")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"mode": ' + json.dumps(args.mode) + ',\n"cases": {\n' + ",\n".join(
            f"{json.dumps(n)}: {json.dumps(v, separators=(',', ':'))}" for n, v in result.items()) + "\n}}\n")
    print(f"wrote {args.out}: {len(result)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
