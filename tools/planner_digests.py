"""Bit-equality of the model surface and the denoiser planner between two trees: a fixed list of tiny `Unet` / `Unet3D` models, each built
under torch.manual_seed(0), and per model what a refactor of unet.py / unet3d.py / engine.py / engine3d.py must leave equal, with no tolerance:

  models   the SHA-256 over the `state_dict` keys in order plus the tensor bytes, the sorted `_locals` keys, and per dry CPU engine the
           routing_snapshot.wiring_sha256 of the step plan and of the static plans `set_conditioning` builds, plus the sorted `taps` keys;
  outputs  the SHA-256 of the tensors `forward`, `forward_with_cond_scale(cond_scale=3)` and its negative-prompt form return — and of a
           `forward(cond_drop_prob=0.5)`, with the next draw of the caller's generator behind each call — on the fixture models of
           tests/golden, one self-conditioned `Unet` and one `Unet3D` with a conditioning image and prompt frames.  This is the host-side order
           inside `_run` (set_conditioning, set_cond_images, set_self_cond ...), which a launch-list digest does not see.

    python tools/planner_digests.py --mode cpu --out profiles/unet_base_digests_head_cpu.json
    python tools/planner_digests.py --mode gpu --tree ../parent --out profiles/unet_base_digests_parent_gpu.json
    python tools/planner_digests.py --compare profiles/unet_base_digests_parent_cpu.json profiles/unet_base_digests_head_cpu.json

--tree: the checkout whose `imagen_pytorch_amd` is digested (default: this one); the tool, the fixtures and the interpreter are this tree's.
--mode cpu: `models` and `outputs`, the latter through the plan interpreter with the patches of tests/cpu_replay.py.  --mode gpu: `outputs`
alone, on the device.  Both need the built kernel library (--mode cpu: for the host-side weight packing only).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B, S, FRAMES, N_TOK, WIDTH = 2, 16, 4, 8, 32       # batch, image side, frames of a clip, text tokens, text_embed_dim of every model below
RECT = ("memory_efficient_lowres", "combine_upsample_fmaps")     # the SWEEP entries planned at 16 x 24 as well

_T3 = dict(dim=8, cond_dim=32, text_embed_dim=WIDTH, dim_mults=(1, 2), attn_heads=2, max_text_len=16, attn_pool_num_latents=8)
VIDEO = {
    "default": dict(_T3),
    "temporal_strides": dict(_T3, temporal_strides=(1, 2), layer_attns=(False, True)),
    "lowres_cond": dict(_T3, lowres_cond=True),
    "memory_efficient": dict(_T3, memory_efficient=True),
    "self_cond": dict(_T3, self_cond=True),
    "cond_images_5": dict(_T3, cond_images_channels=5),
    "head_dim_32": dict(_T3, attn_dim_head=32, layer_attns=(False, True)),
    "no_final_resnet": dict(_T3, final_resnet_block=False),
}
VIDEO_ENGINES = {"": {}, ".ignore_time": dict(ignore_time=True), ".prompt_frames": dict(pre_frames=2, post_frames=2)}


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(f"{str(t.dtype)[6:]}{list(t.shape)}".encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _state_sha(unet) -> str:
    h = hashlib.sha256()
    for k, v in unet.state_dict().items():
        h.update(k.encode())
        h.update(_sha(v).encode())
    return h.hexdigest()


def _seeded(klass, kw):
    torch.manual_seed(0)
    return klass(**kw).eval()


def _engine_record(eng, unet) -> dict:
    """The wiring of the step plan and of what a guided set_conditioning() builds on the dry engine `eng`, and its taps."""
    import routing_snapshot as rs

    src = eng.src_batch
    te = _rand(1, src, N_TOK, WIDTH) if eng.has_text else None
    eng.set_conditioning(text_embeds=te, text_mask=None, keep=torch.arange(eng.R) < src,
                         lowres_noise_times=torch.full((src,), 0.25) if unet.lowres_cond else None)
    return {"step": rs.wiring_sha256(eng.step_plan), "static": [rs.wiring_sha256(p) for p in eng._last_static], "taps": sorted(eng.taps)}


def collect_models() -> dict:
    from unet_config_sweep import SWEEP

    from imagen_pytorch_amd import Unet, Unet3D
    from imagen_pytorch_amd.engine import UnetEngine
    from imagen_pytorch_amd.engine3d import UnetEngine3D

    out = {}
    for name, kw in SWEEP.items():
        u = _seeded(Unet, kw)
        rec = {"state_dict": _state_sha(u), "locals": sorted(u._locals), "engines": {}}
        for tag, size in [("16x16", (S, S))] + ([("16x24", (S, 24))] if name in RECT else []):
            rec["engines"][tag] = _engine_record(UnetEngine(u, 2 * B, B, size, "cpu", dry=True), u)
        out["unet." + name] = rec
        print(f"unet.{name}: {len(rec['engines'])} engines", flush=True)
    for name, kw in VIDEO.items():
        u = _seeded(Unet3D, kw)
        rec = {"state_dict": _state_sha(u), "locals": sorted(u._locals), "engines": {}}
        for tag, ekw in VIDEO_ENGINES.items():
            if kw.get("self_cond") and ekw.get("pre_frames"):
                continue            # (refused by both trees: a self-conditioning clip cannot be extended by prompt frames)
            rec["engines"][f"f{FRAMES}x{S}{tag}"] = _engine_record(UnetEngine3D(u, 2 * B, B, FRAMES, S, "cpu", dry=True, **ekw), u)
        out["unet3d." + name] = rec
        print(f"unet3d.{name}: {len(rec['engines'])} engines", flush=True)
    return out


def _dezero(unet, seed=3):
    """final_conv is zero-initialised: give it values, or every output is its bias."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        unet.final_conv.weight.copy_(torch.randn(unet.final_conv.weight.shape, generator=g) * 0.1)
        unet.final_conv.bias.copy_(torch.randn(unet.final_conv.bias.shape, generator=g) * 0.1)
    return unet


def _output_models():
    """(name, unet, positional inputs, keyword inputs) of every model of the `outputs` part."""
    from unet_config_sweep import SWEEP

    from imagen_pytorch_amd import Unet, Unet3D

    for name in ("unet_tiny_base", "unet_tiny_sr"):
        g = torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=False)
        u = Unet(**g["kwargs"]).eval()
        u.load_state_dict(g["state_dict"])
        kw = dict(text_embeds=g["text_embeds"], text_mask=g["text_mask"])
        if u.lowres_cond:
            kw.update(lowres_cond_img=_rand(4, *g["x"].shape), lowres_noise_times=torch.full((g["x"].shape[0],), 0.3))
        yield name, u, (g["x"], g["time"]), kw
    g = torch.load(os.path.join(GOLDEN, "sample_tiny_video.pt"), weights_only=False)
    u = Unet3D(**g["unets"][0]["kwargs"]).eval()
    u.load_state_dict(g["unets"][0]["state_dict"])
    yield "tiny_video", u, (_rand(5, B, 3, g["frames"], S, S), torch.tensor([0.4, -0.7])), dict(text_embeds=g["text_embeds"])
    te = _rand(6, B, N_TOK, WIDTH)
    yield ("self_cond_2d", _dezero(_seeded(Unet, SWEEP["self_cond"])), (_rand(7, B, 3, S, S), torch.tensor([0.2, -1.1])),
           dict(text_embeds=te, self_cond=_rand(8, B, 3, S, S)))
    yield ("cond_images_3d", _dezero(_seeded(Unet3D, VIDEO["cond_images_5"])), (_rand(9, B, 3, FRAMES, S, S), torch.tensor([0.9, -0.1])),
           dict(text_embeds=te, cond_images=_rand(10, B, 5, 8, 8), cond_video_frames=_rand(11, B, 3, 2, S, S)))


def collect_outputs(device: str) -> dict:
    out = {}
    for name, u, args, kw in _output_models():
        u = u.to(device)
        args = tuple(a.to(device) for a in args)
        kw = {k: v.to(device) for k, v in kw.items()}
        neg = dict(negative_text_embeds=(kw["text_embeds"].flip(0) * 0.5)[:, :5])
        calls = {"forward": lambda: u(*args, **kw),
                 "forward.drop_0.5": lambda: u(*args, cond_drop_prob=0.5, **kw),
                 "cond_scale_3": lambda: u.forward_with_cond_scale(*args, cond_scale=3., **kw),
                 "cond_scale_3.negative": lambda: u.forward_with_cond_scale(*args, cond_scale=3., **neg, **kw),
                 "cond_scale_1": lambda: u.forward_with_cond_scale(*args, cond_scale=1., **kw)}
        rec = {}
        for call, fn in calls.items():
            torch.manual_seed(14)       # (cond_drop_prob = 0.5 then keeps the second of the two samples and drops the first)
            y = fn()
            if device != "cpu":
                torch.cuda.synchronize()
            rec[call] = {"sha256": _sha(y), "next_draw": repr(torch.rand(1).item())}     # (the caller's CPU generator, behind the call)
        u.release_engines()
        out[name] = rec
        print(f"{name}: {len(rec)} calls", flush=True)
    return out


def compare(a_path: str, b_path: str) -> int:
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    bad = 0
    for part in sorted((set(a) | set(b)) - {"mode"}):
        pa, pb = a.get(part, {}), b.get(part, {})
        diff = [n for n in sorted(set(pa) | set(pb)) if pa.get(n) != pb.get(n)]
        for n in diff:
            what = "missing" if n not in pa or n not in pb else [k for k in pa[n] if pa[n][k] != pb[n].get(k)]
            print(f"{part} {n}: {what} differ")
        print(f"{part}: {len(pa)} / {len(pb)} entries, " + (f"{len(diff)} differ" if diff else "all equal"))
        bad += len(diff)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mode", choices=("cpu", "gpu"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is digested")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    assert args.mode and args.out, "--mode and --out"
    tree = os.path.abspath(args.tree)
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), tree):      # (the digested tree first on the path)
        sys.path.insert(0, p)
    import imagen_pytorch_amd       # (before any other module of this tree puts its own root on the path)

    assert os.path.abspath(imagen_pytorch_amd.__file__).startswith(tree + os.sep), imagen_pytorch_amd.__file__
    result = {"mode": args.mode}
    if args.mode == "cpu":
        import cpu_replay

        result["models"] = collect_models()
        with cpu_replay.cpu_backend():
            result["outputs"] = collect_outputs("cpu")
    else:
        result["outputs"] = collect_outputs("cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}: " + ", ".join(f"{len(v)} {k}" for k, v in result.items() if k != "mode"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
