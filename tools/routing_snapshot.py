"""Launch lists of the denoiser plans as data: every op of every plan with every field of its params struct.

    python tools/routing_snapshot.py            # compare the plans this tree builds with tests/golden/routing_snapshot.json
    python tools/routing_snapshot.py --write    # regenerate the fixture (a deliberate routing change: its diff is the list of launches that moved)

The plans are built dry (CPU memory, nothing launched), so this needs the kernel library but no GPU.  tests/test_routing_snapshot.py imports
snapshot() / first_difference() from here: one definition of what a launch list is.

A record is {"kind", "label", <field>: value ...} of one op: integer fields by value, float fields as repr(), pointer fields as
null / non-null (addresses differ from run to run); fields that are 0 / null are left out.  IGEMM records also carry what ops.igemm() told
its caller (ssq_emitted, post_applied, gca_chunks).  The fixture keeps the records of the IGEMM, ROWCHAIN, ACT_PREP and GCA_* ops exactly and in
order — each distinct one once, as a line of values — and one SHA-256 per plan over the ordered records of every other kind (see digest()).
tests/golden/routing_wiring.json holds a second view of the same plans: one SHA-256 per plan over wired_records(), which carry the pointer fields
as ordinals of first use — the buffer wiring.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "routing_snapshot.json")
WIRING_FIXTURE = os.path.join(GOLDEN, "routing_wiring.json")   # {plan name: wiring_sha256}: the buffer wiring the other fixture leaves out

README_U1 = dict(dim=32, cond_dim=512, dim_mults=(1, 2, 4, 8), num_resnet_blocks=3, layer_attns=(False, True, True, True),
                 layer_cross_attns=(False, True, True, True))
README_U2 = dict(dim=32, cond_dim=512, dim_mults=(1, 2, 4, 8), num_resnet_blocks=(2, 4, 8, 8), layer_attns=(False, False, False, True),
                 layer_cross_attns=(False, False, False, True), lowres_cond=True)
CFG_TABLE_FIXTURE = os.path.join(GOLDEN, "conv_cfg_table_abi15.json")   # cfg_table_answers() of the library the merged tile tables came from
C2_BASE = dict(README_U1, dim=128)
STATIC_TOKENS = 256   # text tokens of the static (once per request) plan, as in tests/test_bench_shapes_gpu.py
IGEMM_RESULTS = ("ssq_emitted", "post_applied", "gca_chunks")


def record(kind_name: str, p, label: str) -> dict:
    rec = {"kind": kind_name, "label": label}
    for name, ctype in p._fields_:
        v = getattr(p, name)
        if ctype is ctypes.c_void_p:
            v = bool(v)
        elif ctype is ctypes.c_float:
            v = repr(v)
        if v not in (0, "0.0"):     # (False == 0)
            rec[name] = v
    if kind_name == "IGEMM":
        for name in IGEMM_RESULTS:
            v = getattr(p, name)
            if v:
                rec[name] = int(v)
    return rec


def plan_records(plan) -> list:
    from imagen_pytorch_amd import _abi

    names = {v: k[len("IMAGEN_OP_"):] for k, v in _abi.ENUMS.items() if k.startswith("IMAGEN_OP_")}
    return [record(names[kind], p, label) for kind, p, label in plan.ops]


def wired_records(plan) -> list:
    """plan_records with every pointer field as the ordinal of its address among the distinct addresses of the plan, in order of first use
    (0 = null, left out): which launch reads what which other launch wrote, and at which of its offsets, without the addresses themselves.
    (A plan keeps every tensor it references alive, so distinct buffers have distinct addresses.)"""
    seen, out = {}, plan_records(plan)
    for rec, (_, p, _) in zip(out, plan.ops):
        for name, ctype in p._fields_:
            if ctype is ctypes.c_void_p and getattr(p, name):
                rec[name] = seen.setdefault(getattr(p, name), len(seen) + 1)
    return out


def wiring_sha256(plan) -> str:
    return hashlib.sha256(json.dumps(wired_records(plan), sort_keys=True).encode()).hexdigest()


def _engines():
    """(name, engine) of every covered model, one at a time (the 256^2 engine alone holds a few GB of CPU buffers)."""
    from imagen_pytorch_amd import Unet, Unet3D
    from imagen_pytorch_amd.engine import UnetEngine
    from imagen_pytorch_amd.engine3d import UnetEngine3D

    for name, kw, S, rows, src in (("unet1_64_r16", README_U1, 64, 16, 8), ("unet2_256_r16", README_U2, 256, 16, 8),
                                   ("c2_64_r16", C2_BASE, 64, 16, 8), ("unet1_64_r96", README_U1, 64, 96, 48)):
        torch.manual_seed(0)   # (weight values reach a plan only through attention_logit_bound)
        yield name, UnetEngine(Unet(**kw).eval(), rows=rows, src_batch=src, size=S, device="cpu", dry=True)
    torch.manual_seed(0)
    yield "c5_unet3d_64_f16_r2", UnetEngine3D(Unet3D(dim=64, dim_mults=(1, 2, 4, 8)).eval(), 2, 1, 16, 64, "cpu", dry=True)
    for name in ("unet_tiny_base", "unet_tiny_sr"):   # (family 0's odd shapes)
        g = torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=False)
        u = Unet(**g["kwargs"]).eval()
        u.load_state_dict(g["state_dict"])
        yield name + "_r4", UnetEngine(u, 4, 2, g["x"].shape[-1], "cpu", dry=True)


def snapshot(wiring: dict = None) -> dict:
    """{plan name: [record of every op, in launch order]}: the step plan of every covered model, and the static plan of the 2D ones.
    `wiring`, if given, receives {plan name: wiring_sha256} of the same plans (every engine is built once)."""
    out = {}
    for name, eng in _engines():
        plans = {name + ".step": eng.step_plan}
        if not name.startswith("c5"):
            plans[name + ".static"] = eng._build_static_plan(STATIC_TOKENS)[0]
        for pname, plan in plans.items():
            out[pname] = plan_records(plan)
            if wiring is not None:
                wiring[pname] = wiring_sha256(plan)
    return out


def coverage(snap: dict) -> tuple:
    """(kernel families of the IGEMM launches, ROWCHAIN modes) over all plans."""
    from imagen_pytorch_amd import ops

    tab = ops.cfg_table()
    fams, modes = set(), set()
    for recs in snap.values():
        for r in recs:
            if r["kind"] == "IGEMM":
                fams.add(tab[r.get("cfg", 0)][3])
            elif r["kind"] == "ROWCHAIN":
                modes.add(r.get("mode", 0))
    return fams, modes


EXACT_KINDS = ("IGEMM", "ROWCHAIN", "ACT_PREP", "GCA_PARTIAL", "GCA_FINAL", "GCA_TAIL")   # kept record by record; the other kinds go into one SHA-256 per plan


def digest(recs: list) -> dict:
    """What the fixture holds of one plan: the records of the EXACT_KINDS in launch order, and the SHA-256 of the ordered JSON of ALL its ops with
    those records cut down to kind + label (so the hash pins every other op, and where the exact ones sit between them)."""
    exact = [r for r in recs if r["kind"] in EXACT_KINDS]
    rest = [{"kind": r["kind"], "label": r["label"]} if r["kind"] in EXACT_KINDS else r for r in recs]
    return {"exact": exact, "sha256": hashlib.sha256(json.dumps(rest, sort_keys=True).encode()).hexdigest()}


def _schema() -> dict:
    from imagen_pytorch_amd import _abi

    out = {}
    for k, v in _abi.ENUMS.items():
        if k.startswith("IMAGEN_OP_") and k[len("IMAGEN_OP_"):] in EXACT_KINDS:
            kind = k[len("IMAGEN_OP_"):]
            out[kind] = [n for n, _ in _abi.OP_STRUCT[v]._fields_] + (list(IGEMM_RESULTS) if kind == "IGEMM" else [])
    return out


def write(snap: dict, path: str = FIXTURE) -> None:
    """fields: the value order per kind; bodies: the DISTINCT records over all plans as [kind, value ...] (null-ness as 0 / 1, trailing zeros cut), one
    per line; labels; per plan the ordered [label index, body index, ...] of its exact records and the SHA-256 of the rest."""
    fields, bodies, labels, plans = _schema(), {}, {}, {}
    for name, recs in snap.items():
        d = digest(recs)
        flat = []
        for r in d["exact"]:
            assert set(r) <= set(fields[r["kind"]]) | {"kind", "label"}, r
            vals = [r.get(f, 0) for f in fields[r["kind"]]]
            while vals and vals[-1] == 0:
                vals.pop()
            body = json.dumps([r["kind"]] + [int(v) if isinstance(v, bool) else v for v in vals], separators=(",", ":"))
            flat += [labels.setdefault(r["label"], len(labels)), bodies.setdefault(body, len(bodies))]
        plans[name] = {"exact": flat, "sha256": d["sha256"]}
    with open(path, "w") as f:
        f.write('{"fields": ' + json.dumps(fields) + ',\n"bodies": [\n' + ",\n".join(bodies) + '\n],\n"labels": ' + json.dumps(list(labels))
                + ',\n"plans": {\n' + ",\n".join(f"{json.dumps(n)}: {json.dumps(v, separators=(',', ':'))}" for n, v in plans.items()) + "\n}}\n")


def load(path: str = FIXTURE) -> dict:
    """{plan name: digest} as written."""
    with open(path) as f:
        fx = json.load(f)
    out = {}
    for name, pl in fx["plans"].items():
        exact = []
        for li, bi in zip(pl["exact"][::2], pl["exact"][1::2]):
            kind, *vals = fx["bodies"][bi]
            rec = {"kind": kind, "label": fx["labels"][li]}
            rec.update((f, v) for f, v in zip(fx["fields"][kind], vals) if v not in (0, "0.0"))
            exact.append(rec)
        out[name] = {"exact": exact, "sha256": pl["sha256"]}
    return out


def first_difference(old: dict, snap: dict):
    """None if the launch lists `snap` (snapshot()) equal the fixture `old` (load()), else a line naming the first op that differs (plan, index
    among the plan's exact records, label, field, old, new)."""
    new = {name: digest(recs) for name, recs in snap.items()}
    if list(old) != list(new):
        return f"plans differ: {sorted(set(old) ^ set(new)) or 'order'}"
    for name in old:
        a_all, b_all = old[name]["exact"], new[name]["exact"]
        for i, (a, b) in enumerate(zip(a_all, b_all)):
            if a != b:
                field = next(k for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0))
                return f"{name} exact op {i} '{a['label']}': {field} was {a.get(field, 0)!r}, is {b.get(field, 0)!r}"
        if len(a_all) != len(b_all):
            return f"{name}: {len(a_all)} exact ops before, {len(b_all)} now (the first {min(len(a_all), len(b_all))} agree)"
        if old[name]["sha256"] != new[name]["sha256"]:
            return f"{name}: an op of another kind than {', '.join(EXACT_KINDS)}, or the order of the ops, changed (sha256 {old[name]['sha256'][:12]} -> {new[name]['sha256'][:12]})"
    return None


def cfg_table_answers() -> dict:
    """What the library tells the planner about every tile cfg id (tests/golden/conv_cfg_table_abi15.json): config_info, _family, _ring, _stage_slots
    and _lds_bytes for 3x3 and 1x1 kernels at stride 1 and 2 on every tile shape ops.launchable_shapes() tries (a map of one row included)."""
    from imagen_pytorch_amd import ops

    lib = ops.load_library()
    rows = []
    for cfg in range(-1, lib.imagen_igemm_num_configs() + 1):   # (one id outside on either side)
        tp, bn, g = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.imagen_igemm_config_info(cfg, ctypes.byref(tp), ctypes.byref(bn), ctypes.byref(g))
        shapes = sorted(set(ops._tile_shapes(tp.value, 64, 64) + ops._tile_shapes(tp.value, 1, 64))) if rc == 0 else [(8, 8)]
        rows.append({"cfg": cfg, "info": [rc, tp.value, bn.value, g.value], "family": lib.imagen_igemm_config_family(cfg), "ring": lib.imagen_igemm_config_ring(cfg),
                     "stage_slots": [lib.imagen_igemm_stage_slots(cfg, k, k) for k in (3, 1)],
                     "lds_bytes": [[k, st, th, tw, lib.imagen_igemm_lds_bytes(cfg, k, k, st, th, tw)] for k in (3, 1) for st in (1, 2) for th, tw in shapes]})
    return {"num_configs": lib.imagen_igemm_num_configs(), "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate tests/golden/routing_snapshot.json and routing_wiring.json from this tree")
    ap.add_argument("--write-cfg-table", action="store_true", help="regenerate tests/golden/conv_cfg_table_abi15.json from the loaded library")
    args = ap.parse_args()
    if args.write_cfg_table:
        with open(CFG_TABLE_FIXTURE, "w") as f:
            json.dump(cfg_table_answers(), f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {CFG_TABLE_FIXTURE}")
        return 0
    wiring = {}
    snap = snapshot(wiring)
    fams, modes = coverage(snap)
    print(f"{len(snap)} plans, {sum(map(len, snap.values()))} ops, {sum(r['kind'] == 'IGEMM' for v in snap.values() for r in v)} igemm launches; "
          f"families {sorted(fams)}, rowchain modes {sorted(modes)}")
    if args.write:
        write(snap)
        with open(WIRING_FIXTURE, "w") as f:
            json.dump(wiring, f, indent=0)
            f.write("\n")
        print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes) and {WIRING_FIXTURE}")
        return 0
    with open(WIRING_FIXTURE) as f:
        moved = [n for n, h in json.load(f).items() if wiring.get(n) != h]
    diff = first_difference(load(), snap) or (f"buffer wiring changed (same launch lists): {moved}" if moved else None)
    print(diff or "launch lists and buffer wiring unchanged")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
