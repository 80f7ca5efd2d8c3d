"""Launch lists of the SAMPLER stages as data: the per-step plan(s) a stage replays, its engine's step plan and static plan(s), for the tiny
fixture models of tests/golden under both samplers (Imagen = DDPM, ElucidatedImagen = Karras).

    python tools/sampler_snapshot.py            # compare the stages this tree builds with tests/golden/sampler_snapshot.json
    python tools/sampler_snapshot.py --write    # regenerate the fixture (a deliberate change of what a stage launches)

The stages are built dry (CPU memory, nothing launched).  A record is tools/routing_snapshot.py's — kind, label, every integer field by value,
floats as repr() — in its wired form (routing_snapshot.wired_records): a pointer field holds the ordinal of its address among the distinct
addresses of the plan, in order of first use (0 = null).  The fixture
keeps, per plan, the labels in launch order and one SHA-256 over the ordered records.  tests/test_sampler_snapshot.py asserts equality.
"""
from __future__ import annotations

import argparse
import functools
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import routing_snapshot as rs  # noqa: E402

FIXTURE = os.path.join(rs.GOLDEN, "sampler_snapshot.json")
B, T, TOKENS = 2, 4, 9
# case -> (model, stage index, _stage keywords beyond the defaults below); every case under both samplers unless listed in DDPM_ONLY
DEFAULTS = dict(cond_scale=3.0, with_text=True, inject_noise=True, sample_offset=0)
CASES = {
    "guided": ("image", 0, {}),
    "unguided": ("image", 0, dict(cond_scale=1.0)),
    "philox": ("image", 0, dict(inject_noise=False)),                      # inject_noise off: the in-kernel Philox stream
    "inpaint": ("image", 0, dict(resample_times=2)),
    "inpaint_philox": ("image", 0, dict(resample_times=2, inject_noise=False)),
    "self_cond": ("self_cond", 0, {}),
    "video": ("video", 0, dict(frames=4)),
    "video_prompts": ("video", 0, dict(frames=4, prompt_frames=(2, 2))),
    "lowres": ("image", 1, {}),
    "cond_images": ("cond_images", 0, {}),
}
DDPM_ONLY = ("cond_images",)
# what the few-step solvers and the guidance schedules build (Imagen only): recorded after the table above, so that its entries keep their place.
# A guidance vector with steps at exactly 1 also records its unguided sibling: `sibling.plan` and the sibling engine's `sibling.step`.
LATER_CASES = {
    "ddim": ("image", dict(solver=("ddim", T, 0.0))),
    "ddim_eta": ("image", dict(solver=("ddim", T, 0.5))),
    "dpmpp_2m": ("image", dict(solver=("dpmpp_2m", T, 0.0))),
    "dpmpp_2m_self_cond": ("self_cond", dict(solver=("dpmpp_2m", T, 0.0))),
    "dpmpp_2m_philox": ("image", dict(solver=("dpmpp_2m", T, 0.0), inject_noise=False)),
    "guidance_ramp": ("image", dict(guidance=[3.0, 2.5, 2.0, 1.5])),
    "guidance_interval": ("image", dict(guidance=[1.0, 3.0, 3.0, 1.0])),
    "guidance_interval_dpmpp_2m": ("image", dict(guidance=[1.0, 3.0, 3.0, 1.0], solver=("dpmpp_2m", T, 0.0))),
}


def _load(name):
    return torch.load(os.path.join(rs.GOLDEN, name), weights_only=False)


def _model(which: str, karras: bool):
    from imagen_pytorch_amd import ElucidatedImagen, Imagen, Unet, Unet3D

    g = _load("sample_tiny_video.pt" if which == "video" else "sample_tiny_cascade.pt")
    extra = {"self_cond": dict(self_cond=True), "cond_images": dict(cond_images_channels=4)}.get(which, {})
    torch.manual_seed(0)   # (the unets with an extra input keep their seeded init conv: its shape differs from the recorded one)
    unets = [(Unet3D if which == "video" else Unet)(**{**spec["kwargs"], **extra}).eval() for spec in g["unets"]]
    kw = dict(image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1)
    if karras:
        model = ElucidatedImagen(unets, num_sample_steps=T, **kw)
    else:
        model = Imagen(unets, timesteps=T, **kw)
    if not extra:
        for u, spec in zip(model.unets, g["unets"]):
            u.load_state_dict(spec["state_dict"])
    return model.eval()


def _stage_records(out: dict, name: str, model, idx: int, kw: dict) -> None:
    """Build stage `idx` of `model` dry, condition its engine(s) and file the records of its plans under `name`."""
    if kw.get("guidance") is not None:
        kw = {**kw, "guidance": torch.tensor(kw["guidance"], dtype=torch.float32)}
    st = model._stage(idx, B, torch.device("cpu"), **{**DEFAULTS, **kw})
    for prefix, s in ((name, st), (name + ".sibling", st.get("sibling"))):
        if s is None:
            continue
        eng = s["eng"]
        rows = eng.R
        keep = torch.ones(rows, dtype=torch.bool)
        keep[B:] = False
        eng.set_conditioning(text_embeds=torch.zeros(B, TOKENS, 32), text_mask=None, keep=keep,
                             lowres_noise_times=torch.full((B,), 0.2) if idx else None)
        out[prefix + ".plan"] = rs.wired_records(s["plan"])
        if "last" in s:
            out[prefix + ".last"] = rs.wired_records(s["last"])
        out[prefix + ".step"] = rs.wired_records(eng.step_plan)
        if s is st:
            for i, pl in enumerate(eng._last_static):
                out[f"{name}.static{i}"] = rs.wired_records(pl)


def snapshot() -> dict:
    """{"<sampler>.<case>.<plan>": [record, ...]}: `plan` (and `last` for Karras) of the stage, `step` and `static<i>` of its engine."""
    from imagen_pytorch_amd import engine, engine3d

    saved = engine.UnetEngine, engine3d.UnetEngine3D
    engine.UnetEngine = functools.partial(engine.UnetEngine, dry=True)
    engine3d.UnetEngine3D = functools.partial(engine3d.UnetEngine3D, dry=True)
    out = {}
    try:
        for sampler in ("ddpm", "karras"):
            for case, (which, idx, kw) in CASES.items():
                if sampler == "karras" and case in DDPM_ONLY:
                    continue
                _stage_records(out, f"{sampler}.{case}", _model(which, sampler == "karras"), idx, kw)
        for case, (which, kw) in LATER_CASES.items():
            _stage_records(out, f"ddpm.{case}", _model(which, False), 0, kw)
    finally:
        engine.UnetEngine, engine3d.UnetEngine3D = saved
    return out


def digest(snap: dict) -> dict:
    """What the fixture holds: a shared label table, and per plan the label indices in launch order + the SHA-256 of the ordered records."""
    labels, plans = {}, {}
    for name, recs in snap.items():
        plans[name] = {"ops": [labels.setdefault(r["label"], len(labels)) for r in recs],
                       "sha256": hashlib.sha256(json.dumps(recs, sort_keys=True).encode()).hexdigest()}
    return {"labels": list(labels), "plans": plans}


def first_difference(old: dict, new: dict):
    """None if the digests agree, else a line naming the first plan and op that differ."""
    if list(old["plans"]) != list(new["plans"]):
        return f"plans differ: {sorted(set(old['plans']) ^ set(new['plans'])) or 'order'}"
    for name, a in old["plans"].items():
        b = new["plans"][name]
        la, lb = [old["labels"][i] for i in a["ops"]], [new["labels"][i] for i in b["ops"]]
        if la != lb:
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            return f"{name}: op {i} was {la[i] if i < len(la) else None!r}, is {lb[i] if i < len(lb) else None!r} ({len(la)} ops before, {len(lb)} now)"
        if a["sha256"] != b["sha256"]:
            return f"{name}: same labels, but a params field or the buffer wiring changed (sha256 {a['sha256'][:12]} -> {b['sha256'][:12]})"
    return None


def write_fixture(path: str, dig: dict) -> None:
    with open(path, "w") as f:
        f.write('{"labels": ' + json.dumps(dig["labels"]) + ',\n"plans": {\n'
                + ",\n".join(f"{json.dumps(n)}: {json.dumps(v, separators=(',', ':'))}" for n, v in dig["plans"].items()) + "\n}}\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def main(snap=snapshot, fixture=FIXTURE, what="sampler launch lists"):
    """The command line of this tool, and of tools/attn_planner_snapshot.py over its own snapshot() and fixture."""
    ap = argparse.ArgumentParser(description=sys.modules[snap.__module__].__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help=f"regenerate {os.path.relpath(fixture, ROOT)} from this tree")
    args = ap.parse_args()
    new = digest(snap())
    print(f"{len(new['plans'])} plans, {sum(len(p['ops']) for p in new['plans'].values())} ops")
    if args.write:
        write_fixture(fixture, new)
        return 0
    with open(fixture) as f:
        diff = first_difference(json.load(f), new)
    print(diff or what + " unchanged")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
