"""MI355X (-m gpu; the kernel cases also on the CPU emulation, IMAGEN_EMUL_TESTS=1): rectangular images.

 * conv_small (family 8) on the blocks with a masked edge that ops.small_tile now answers for the maps of a rectangular image — 8x12, 12x8,
   16x24, 24x16, 4x6 (2 and 16 images) and 32x48 (2 images; 16 of them are past SMALL_MAX_ROWS) — per pixel against the fp64 IGEMM contract
   of tests/igemm_contract.py with the tile of ops.small_tile, at the bounds tests/test_conv_contract_gpu.py holds family 8 to: 3x3 and 1x1,
   Cin / Cout from {32, 64, 256, 384}, the Block prologue on two inputs, GlobalContext partials, full_cout (ssq_out / post), a ragged Cout,
   the pixel-shuffle epilogue; sentinels around every output;
 * PACK_IMAGE and LOWRES_PREP (16x24 -> 32x48, 24x16 -> 48x32) against torch in fp64;
 * the fixture forwards (tests/golden/rect_forward_*.pt) on the HIP path, both orientations, cond and null, at the 1e-2 that
   tests/test_model_gpu.py::test_unet_forward_vs_reference_fixture holds the tiny reference fixtures to;
 * the samplers against the recorded runs at the bars of their square twins (2e-2 DDPM, 3e-2 Karras; merged requests 2e-3 against each
   request's own sample()); graph == eager, sample_pipelined == sample, lane == default lane: bit for bit;
 * README unet1 at 64x96 and unet2 at 128x192, batch 2: finite, graph replay == eager launch by launch, bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_rect as fr  # noqa: E402
import igemm_contract  # noqa: E402
from conftest import EMULATED, gpu_device, record_parity  # noqa: E402
from fixtures_rect import SAMPLE_BAR, nerr  # noqa: E402
from igemm_contract import Verdict, run_case  # noqa: E402
from test_bench_shapes_gpu import README_U1, README_U2  # noqa: E402
from test_conv_contract_gpu import SSQ_AFF, cfg_of  # noqa: E402

pytestmark = pytest.mark.gpu
FORWARD_GPU_BAR = 1e-2      # tests/test_model_gpu.py::test_unet_forward_vs_reference_fixture (cond, null)
MERGED_BAR = 2e-3           # tests/test_model_gpu.py::test_merged_requests_match_separate_calls


@pytest.fixture(scope="module")
def ops():
    from imagen_pytorch_amd import ops as o

    return o


@pytest.fixture(scope="module")
def dev():
    return gpu_device()


@pytest.fixture()
def planner_tile(ops, monkeypatch):
    """The contract's cases launched with the tile ops.small_tile answers (igemm_contract.tile_shape restates the tiles of the square maps)."""
    real = igemm_contract.tile_shape
    monkeypatch.setattr(ops, "SMALL_RAGGED_MAPS", tuple(SHAPES))      # also the maps the planner keeps on the fallback

    def tile_shape(o, fam, cfg, OH, OW, K, stride):
        got = o.small_tile(OH, OW) if fam == 8 else None
        return got if got is not None else real(o, fam, cfg, OH, OW, K, stride)
    monkeypatch.setattr(igemm_contract, "tile_shape", tile_shape)


# ------------------------------------------------------------------------------------------------ conv_small, ragged blocks

SHAPES = [(8, 12), (12, 8), (16, 24), (24, 16), (4, 6), (32, 48)]


# (16 images of 32x48 are 24576 pixels, six times SMALL_MAX_ROWS; the cfg is forced here, so 16 images of 16x24 run although the planner
# keeps launches of more than SMALL_MAX_ROWS pixels off family 8)
CASES = [pytest.param(hw, B, id=f"{hw[0]}x{hw[1]}-B{B}") for hw in SHAPES for B in (2, 16) if (hw, B) != ((32, 48), 16)]


@pytest.mark.parametrize("hw,B", CASES)
def test_conv_small_ragged_blocks(ops, dev, planner_tile, hw, B):
    H, W = hw
    tile = ops.small_tile(H, W)
    assert tile is not None, hw
    v = Verdict(f"rect.conv_small[{H}x{W} B{B}]", 8)
    big = (H, W) in ((8, 12), (12, 8), (4, 6)) and not (EMULATED and B > 2)
    for K in (3, 1):
        b = dict(K=K, G=4, B=B, H=H, W=W)
        c32, c64, c128 = (cfg_of(ops, 8, bn=n) for n in (32, 64, 128))
        run_case(ops, dev, v, f"k{K}.full_cout.ssq", 8, c32, **b, C1=32, Cout=32, ssq_out=True)
        run_case(ops, dev, v, f"k{K}.full_cout.post", 8, c64, **b, C1=64, Cout=64, epilogue="post")
        run_case(ops, dev, v, f"k{K}.block_prologue", 8, c64, **b, C1=32, C2=32, Cout=64, ssq_out=True, **SSQ_AFF)
        run_case(ops, dev, v, f"k{K}.gca", 8, c128, **b, C1=64, Cout=124, gca=True, ssq_out=True)
        run_case(ops, dev, v, f"k{K}.ragged_cout.addend", 8, c32, **b, C1=32, Cout=36, epilogue="addend")
        run_case(ops, dev, v, f"k{K}.ragged_cout.res", 8, c32, **b, C1=64, Cout=20, epilogue="res", **SSQ_AFF)
        run_case(ops, dev, v, f"k{K}.shuffle", 8, c32, **b, C1=32, Cout=64, epilogue="shuffle", act_out="silu")
        if big:     # the deep layers of the 8x12 / 4x6 levels
            run_case(ops, dev, v, f"k{K}.384to256", 8, c32, **b, C1=256, C2=128, Cout=256, **SSQ_AFF)
            run_case(ops, dev, v, f"k{K}.256to384", 8, c32, **b, C1=256, Cout=384, epilogue="addend")
    v.done()


# ------------------------------------------------------------------------------------------------ PACK_IMAGE, LOWRES_PREP

@pytest.mark.parametrize("hw", [(16, 24), (24, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_image_rectangular(ops, dev, hw):
    H, W = hw
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(2, 3, H, W, generator=g), torch.randn(2, 3, H, W, generator=g)
    out = ops.new_act(4, H, W, 8, dev, zero=False)
    out.t.fill_(7.0)
    plan = ops.Plan("pack")
    ops.pack_image(plan, a.to(dev), b.to(dev), out, brep=2)
    plan.run()
    got = out.t.reshape(4, H, W, 8).float().cpu()
    want = torch.zeros(4, H, W, 8)
    want[..., :3] = a.repeat(2, 1, 1, 1).permute(0, 2, 3, 1).half().float()
    want[..., 3:6] = b.repeat(2, 1, 1, 1).permute(0, 2, 3, 1).half().float()
    assert torch.equal(got, want)


@pytest.mark.parametrize("src,dst", [((16, 24), (32, 48)), ((24, 16), (48, 32)), ((16, 24), (16, 24))], ids=("wide", "tall", "same"))
def test_lowres_prep_rectangular(ops, dev, src, dst):
    g = torch.Generator().manual_seed(5)
    img, noise = torch.rand(2, 3, *src, generator=g), torch.randn(2, 3, *dst, generator=g)
    out = torch.full((2, 3, *dst), 9.0, device=dev)
    plan = ops.Plan("prep")
    ops.lowres_prep(plan, img.to(dev), noise.to(dev), out, alpha=0.8, sigma=0.6)
    plan.run()
    want = 0.8 * (torch.nn.functional.interpolate(img.double(), dst, mode="nearest") * 2 - 1) + 0.6 * noise.double()
    assert float((out.cpu().double() - want).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ fixture forwards

@pytest.mark.skipif(EMULATED, reason="whole models run on the GPU (the CPU suite replays them through the plan interpreter)")
@pytest.mark.parametrize("name,shape", fr.forward_cases())
def test_forward_vs_reference_fixture(dev, name, shape):
    f = fr.forward_records(name)[shape]
    u = fr.unet(name, dev)
    kw = dict(text_embeds=f["text_embeds"].to(dev), text_mask=f["text_mask"].to(dev), **fr.low_kw(f, dev))
    errs = {}
    for branch, drop in (("cond", 0.), ("null", 1.)):
        out = u(f["x"].to(dev), f["time"].to(dev), cond_drop_prob=drop, **kw)
        assert tuple(out.shape) == tuple(f["x"].shape) and bool(torch.isfinite(out).all())
        errs[branch] = nerr(out, f["out_" + branch])
        # the square twin, measured in the same run: the same unet on the centre-cropped input against the reference's record of it (fp16)
        sq = {k: (fr.crop(v) if v.ndim == 4 else v) for k, v in kw.items() if k.startswith("lowres")}
        errs[branch + "_square"] = nerr(u(fr.crop(f["x"]).contiguous().to(dev), f["time"].to(dev), cond_drop_prob=drop, **{**kw, **sq}), f["out_" + branch + "_crop"].float())
    print(f"rect forward [{name} {shape}]: {errs}")
    record_parity(f"rect.forward[{name} {shape}]", **errs)
    assert errs["cond"] < FORWARD_GPU_BAR and errs["null"] < FORWARD_GPU_BAR, errs


# ------------------------------------------------------------------------------------------------ samplers

@pytest.mark.skipif(EMULATED, reason="whole models run on the GPU")
@pytest.mark.parametrize("run", fr.RUNS)
def test_sample_vs_recorded_run(dev, run):
    g, kw = fr.run_kwargs(run, dev)
    r = g["run"]
    model = fr.sample_model(r["kind"], dev)
    outs = model.sample(**kw)
    eager = model.sample(use_graph=False, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager)), "graph replay == eager"
    assert [tuple(o.shape) for o in outs] == [(2, 3, *s) for s in r["image_shapes"]]
    errs = [nerr(o, ref) for o, ref in zip(outs, r["outputs"])]
    print(f"rect sample [{run}] per stage: {errs}")
    record_parity(f"rect.sample[{run}]", **{f"stage{i}": e for i, e in enumerate(errs)})
    assert max(errs) < SAMPLE_BAR[r["kind"]], (run, errs)


@pytest.mark.skipif(EMULATED, reason="whole models run on the GPU")
def test_merged_pipelined_and_lane_calls(dev):
    """sample_requests with two requests against each request's own sample(); sample_pipelined and a second lane against sample(), bit
    for bit — all at image_shapes 16x24 -> 32x48 with the in-kernel Philox noise."""
    model = fr.sample_model("ddpm", dev)
    shapes = ((16, 24), (32, 48))
    tes = [torch.randn(b, 9, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(7 + b)) for b in (2, 3)]
    common = dict(cond_scale=3.0, image_shapes=shapes)
    alone = [model.sample(text_embeds=te, seed=40 + i, use_tqdm=False, **common) for i, te in enumerate(tes)]
    assert [tuple(a.shape) for a in alone] == [(2, 3, 32, 48), (3, 3, 32, 48)]
    merged = model.sample_requests([dict(text_embeds=te, seed=40 + i) for i, te in enumerate(tes)], **common)
    errs = [nerr(m, a) for m, a in zip(merged, alone)]
    record_parity("rect.merged_requests", **{f"request{i}": e for i, e in enumerate(errs)})
    assert max(errs) < MERGED_BAR, errs
    pipe = model.sample_pipelined([dict(text_embeds=te, seed=40 + i) for i, te in enumerate(tes)], **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, alone))
    with model.lane(3):
        lane = model.sample(text_embeds=tes[0], seed=40, use_tqdm=False, **common)
    assert torch.equal(lane, alone[0])
    with pytest.raises(AssertionError, match="must be the same for all merged requests"):
        model.sample_requests([dict(text_embeds=tes[0], image_shapes=shapes)], cond_scale=3.0)


# ------------------------------------------------------------------------------------------------ production-shaped

AUDIT_FACTOR = 2.0      # the factor tests/test_conv_contract_gpu.py allows between two correct plans of one computation: per op kind, the worst
                        # launch of the rectangular plan against the worst launch of the square plan of the same unet


# tools/op_audit.py: "a launch whose kernel follows its contract shows ~1e-5 .. 2e-4" — below the lower end two fp32 summation orders differ by
# rounding noise alone (a kind whose square twin is bit-exact is not held to 2 x 0); a kind the square plan does not launch is held to the upper end
AUDIT_BAND = (1e-5, 2e-4)


@pytest.mark.skipif(EMULATED, reason="whole models run on the GPU")
@pytest.mark.parametrize("config,rect,square", [("u1", (64, 96), 64), ("u2", (128, 192), 128)])
def test_readme_plans_audited_launch_by_launch(config, rect, square, tmp_path):
    """tools/op_audit.py: every launch of the README plan at 64x96 / 128x192 against the CPU plan interpreter FROM IDENTICAL INPUTS, beside
    the square plan of the same unet audited in the same run: per op kind the worst rectangular launch lies within AUDIT_FACTOR of the
    worst square one, nothing is NaN.  The worst launch is recorded."""
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worst = {}
    for tag, size in (("rect", rect), ("square", (square,))):
        path = tmp_path / f"{tag}.json"
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "op_audit.py"), "--config", config, "--size", *map(str, size), "--threads", "16",
                            "--json", str(path)], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        rows = [x for x in json.load(open(path))["rows"] if x["dtype"].startswith("float")]
        assert rows and not any(x["nan"] for x in rows)
        for x in rows:
            if x["err"] > worst.setdefault(tag, {}).get(x["kind"], {"err": -1})["err"]:
                worst[tag][x["kind"]] = dict(err=x["err"], label=x["label"])
    top = max(worst["rect"].items(), key=lambda kv: kv[1]["err"])
    record_parity(f"rect.op_audit[{config} {rect[0]}x{rect[1]}]", worst_launch_err=top[1]["err"],
                  worst_square_launch_err=max(v["err"] for v in worst["square"].values()))
    print(f"op audit [{config}]: worst rectangular launch {top[0]} {top[1]}; per kind rect / square: "
          + ", ".join(f"{k} {v['err']:.1e}/{worst['square'].get(k, {'err': float('nan')})['err']:.1e}" for k, v in sorted(worst["rect"].items())))
    bar = lambda k: max(AUDIT_FACTOR * worst["square"][k]["err"], AUDIT_BAND[0]) if k in worst["square"] else AUDIT_BAND[1]
    bad = {k: (v, worst["square"].get(k)) for k, v in worst["rect"].items() if v["err"] > bar(k)}
    assert not bad, bad


@pytest.mark.skipif(EMULATED, reason="whole models run on the GPU")
def test_readme_cascade_at_64x96(dev):
    """README unet1 at 64x96 (rows of 96, 48, 24, 12) and unet2 at 128x192, batch 2, two steps: finite, and the graph replay equals the
    eager launch-by-launch run bit for bit."""
    from imagen_pytorch_amd import Imagen, Unet, _abi
    from imagen_pytorch_amd import ops as o

    torch.manual_seed(11)
    u1 = Unet(**README_U1)
    u2 = Unet(**{k: v for k, v in README_U2.items() if k != "lowres_cond"})
    model = Imagen((u1, u2), image_sizes=(64, 256), timesteps=4, text_embed_dim=64, cond_drop_prob=0.1).to(dev).eval()
    for u in model.unets:
        torch.nn.init.normal_(u.final_conv.weight, std=0.05)
    te = torch.randn(2, 12, 64, device=dev)
    kw = dict(text_embeds=te, cond_scale=3.0, seed=9, use_tqdm=False, image_shapes=((64, 96), (128, 192)), max_steps=2, return_all_unet_outputs=True)
    outs = model.sample(**kw)
    assert [tuple(x.shape) for x in outs] == [(2, 3, 64, 96), (2, 3, 128, 192)] and all(bool(torch.isfinite(x).all()) for x in outs)
    eager = model.sample(use_graph=False, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    K = _abi.ENUMS["IMAGEN_OP_IGEMM"]
    st = next(s for k, s in model._stages.items() if k[0] == 0)
    rows = {p.OW for k, p, _ in st["plan"].ops if k == K and o.cfg_table()[p.cfg][3] == 8}
    assert (12 in rows) == bool(o.SMALL_RAGGED and (8, 12) in o.SMALL_RAGGED_MAPS), rows
