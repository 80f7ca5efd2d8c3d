"""CPU: the Unet planner's launch list, executed by the plan interpreter (tests/plan_interp.py: every op kind restated from its
documented contract, fp16 storage), reproduces the reference fixture — i.e. buffer wiring, strides, folded weights and op order
of imagen_pytorch_amd/engine.py are right, independent of the HIP kernels (which the -m gpu tests check)."""
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture()
def reference_weights():
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        yield ops
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


def nerr(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def test_interpreter_states_every_op_kind_of_the_abi():
    """One contract per op kind of include/imagen_hip.h (_abi.OP_STRUCT mirrors its enum): an op kind added to the header without a
    contract fails here, not deep inside a replay."""
    from imagen_pytorch_amd import _abi
    from plan_interp import Interpreter

    names = {v: k for k, v in _abi.ENUMS.items() if k.startswith("IMAGEN_OP_")}
    missing = sorted(names.get(k, k) for k in set(_abi.OP_STRUCT) - set(Interpreter.DISPATCH))
    extra = sorted(names.get(k, k) for k in set(Interpreter.DISPATCH) - set(_abi.OP_STRUCT))
    assert set(Interpreter.DISPATCH) == set(_abi.OP_STRUCT), (missing, extra)


@pytest.mark.parametrize("name", ["unet_tiny_base.pt", "unet_tiny_sr.pt"])
@pytest.mark.parametrize("cfg_rows", [False, True])
def test_unet_plan_on_cpu_matches_reference_fixture(name, cfg_rows, reference_weights):
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.engine import UnetEngine
    from plan_interp import run_engine

    g = torch.load(os.path.join(GOLDEN, name), weights_only=False)
    u = Unet(**g["kwargs"]).eval()
    u.load_state_dict(g["state_dict"])
    B, S = g["x"].shape[0], g["x"].shape[-1]
    rows = 2 * B if cfg_rows else B
    out_c, out_n, eng, it = run_engine(UnetEngine(u, rows, B, S, "cpu", dry=True), g["x"], g["time"], g["text_embeds"], g["text_mask"], **g["extra"])
    e_cond = nerr(out_c, g["out_cond"])
    assert e_cond < 1e-2, e_cond          # fp16 storage of every activation, as on the GPU (UNET_TOL of tests/test_model_gpu.py)
    if cfg_rows:
        e_null = nerr(out_n, g["out_null"])
        assert e_null < 1e-2, e_null
    assert len(it.trace) == len(eng.step_plan) + len(eng._static_plans[g["text_embeds"].shape[1]][0])


@pytest.mark.parametrize("name", ["unet_tiny_base.pt", "unet_tiny_sr.pt"])
def test_unet_plan_init_conv_shared_between_cfg_rows(name, reference_weights, monkeypatch):
    """Under classifier-free guidance the init conv runs on the B distinct images and its output (+ statistics) is copied to the null rows
    (engine._init_conv; on the GPU only the large stages take that path): forced onto the tiny fixtures."""
    from imagen_pytorch_amd import engine, ops

    monkeypatch.setattr(engine, "INIT_CONV_SHARED_MIN_PIXELS", 1)
    seen = []
    real = ops.rows_copy
    monkeypatch.setattr(ops, "rows_copy", lambda plan, *a, **k: (seen.append(k.get("label")), real(plan, *a, **k))[1])
    test_unet_plan_on_cpu_matches_reference_fixture(name, True, reference_weights)
    assert "init_conv.cfg_rows" in seen, seen


@pytest.mark.parametrize("tag", ["base", "sr"])
@pytest.mark.parametrize("mode", ["cond", "cfg", "ignore_time"])
def test_unet3d_plan_on_cpu_matches_reference_fixture(tag, mode, reference_weights):
    """SURVEY §8(f) NEXT-2, host logic: the Unet3D planner (engine3d.py) executed by the plan interpreter reproduces Unet3D.forward of the
    live reference on the tiny clip — frame-shifted temporal convolutions, temporal PEG / attention with the generated position bias,
    space-time attention, time token shift, temporal down / up-sampling.  (The two new HIP kernels are specified by the interpreter's
    restatement of their contract; they have not run on a GPU yet.)"""
    from imagen_pytorch_amd import Unet3D
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from plan_interp import run_engine

    g = torch.load(os.path.join(GOLDEN, "unet3d_tiny.pt"), weights_only=False)["runs"][tag]
    u = Unet3D(**g["kwargs"]).eval()
    u.load_state_dict(g["state_dict"])
    B, _, Fr, S, _ = g["x"].shape
    rows = 2 * B if mode == "cfg" else B
    eng = UnetEngine3D(u, rows, B, Fr, S, "cpu", ignore_time=mode == "ignore_time", dry=True)
    out_c, out_n, _, _ = run_engine(eng, g["x"], g["time"], g["text_embeds"], g["text_mask"], **g["extra"])      # (B, c, f, h, w) each
    ref = g["out_notime"] if mode == "ignore_time" else g["out_cond"]
    e = nerr(out_c, ref)
    assert e < 5e-3, e
    if mode == "cfg":
        e_null = nerr(out_n, g["out_null"])
        assert e_null < 5e-3, e_null


@pytest.mark.parametrize("tag", ["base", "sr"])
@pytest.mark.parametrize("prompts", ["pre", "post", "both"])
def test_unet3d_plan_with_prompt_frames_vs_oracle(tag, prompts, reference_weights):
    """Unet3D.forward(cond_video_frames=, post_cond_video_frames=) (iv.py:1682-1718, 1933-1939): the planner's static prompt slots,
    the per-step frame placement, the final conv's own low-res frame order and the output cut, executed by the interpreter, against
    the oracle (itself pinned to recorded runs of the live reference with these arguments)."""
    from imagen_pytorch_amd import Unet3D
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from oracle import unet3d_oracle as u3
    from plan_interp import Interpreter, register_engine

    g = torch.load(os.path.join(GOLDEN, "unet3d_tiny.pt"), weights_only=False)["runs"][tag]
    u = Unet3D(**g["kwargs"]).eval()
    u.load_state_dict(g["state_dict"])
    B, _, Fr, S, _ = g["x"].shape
    gen = torch.Generator().manual_seed(5)
    size = S if tag == "sr" else S // 2                   # the base unet resizes its prompt frames, the low-res one needs them at its size
    pre = torch.rand(B, 3, 2, size, size, generator=gen) if prompts in ("pre", "both") else None
    post = torch.rand(B, 3, 4, size, size, generator=gen) if prompts in ("post", "both") else None
    rows = 2 * B
    eng = UnetEngine3D(u, rows, B, Fr, S, "cpu", dry=True, pre_frames=0 if pre is None else 2, post_frames=0 if post is None else 4)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[B:] = False
    eng.set_conditioning(text_embeds=g["text_embeds"], text_mask=g["text_mask"], keep=keep, lowres_noise_times=g["extra"].get("lowres_noise_times"))
    eng.set_cond_video_frames(pre, post)
    it = Interpreter()
    register_engine(it, eng)
    it.run(eng._static_plans[g["text_embeds"].shape[1]][0])
    fm = lambda t: t.permute(0, 2, 1, 3, 4).contiguous()
    eng.x_in.copy_(fm(g["x"]))
    if eng.lowres:
        eng.lowres_in.copy_(fm(g["extra"]["lowres_cond_img"]))
    eng.times.copy_(g["time"].repeat(rows // B))
    it.run(eng.step_plan)
    out = fm(eng.out)
    kw = dict(text_embeds=g["text_embeds"], text_mask=g["text_mask"], cond_video_frames=pre, post_cond_video_frames=post, **g["extra"])
    with torch.no_grad():
        ref = u3.unet3d_forward(g["state_dict"], g["kwargs"], g["x"], g["time"], **kw)
        ref_null = u3.unet3d_forward(g["state_dict"], g["kwargs"], g["x"], g["time"], cond_drop_prob=1.0, **kw)
    assert out.shape[2] == Fr and tuple(ref.shape) == tuple(out[:B].shape)
    assert nerr(out[:B], ref) < 5e-3 and nerr(out[B:], ref_null) < 5e-3, (nerr(out[:B], ref), nerr(out[B:], ref_null))


@pytest.mark.parametrize("tag", ["base", "sr"])
def test_unet3d_plan_with_cond_images_vs_oracle(tag, reference_weights):
    """Unet3D(cond_images_channels=5): the static second input of the init conv (one image per sample on every frame, prompt frames
    included) and the permuted weight slice, executed by the interpreter, against the oracle (pinned to the live reference)."""
    from imagen_pytorch_amd import Unet3D
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from oracle import unet3d_oracle as u3
    from plan_interp import Interpreter, register_engine

    g = torch.load(os.path.join(GOLDEN, "unet3d_tiny.pt"), weights_only=False)["runs"][tag]
    kw = {**g["kwargs"], "cond_images_channels": 5}
    torch.manual_seed(6)
    u = Unet3D(**kw).eval()
    sd = {k: v.clone() for k, v in u.state_dict().items()}
    for k, v in g["state_dict"].items():          # the recorded weights wherever the shapes agree (everything but the init conv)
        if sd[k].shape == v.shape:
            sd[k] = v.clone()
    u.load_state_dict(sd)
    B, _, Fr, S, _ = g["x"].shape
    gen = torch.Generator().manual_seed(7)
    ci = torch.rand(B, 5, 8, 8, generator=gen)
    pre = torch.rand(B, 3, 2, S, S, generator=gen) if tag == "sr" else None
    rows = 2 * B
    eng = UnetEngine3D(u, rows, B, Fr, S, "cpu", dry=True, pre_frames=0 if pre is None else 2)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[B:] = False
    eng.set_conditioning(text_embeds=g["text_embeds"], text_mask=g["text_mask"], keep=keep, lowres_noise_times=g["extra"].get("lowres_noise_times"))
    if pre is not None:
        eng.set_cond_video_frames(pre, None)
    eng.set_cond_images(ci)
    it = Interpreter()
    register_engine(it, eng)
    it.run(eng._static_plans[g["text_embeds"].shape[1]][0])
    fm = lambda t: t.permute(0, 2, 1, 3, 4).contiguous()
    eng.x_in.copy_(fm(g["x"]))
    if eng.lowres:
        eng.lowres_in.copy_(fm(g["extra"]["lowres_cond_img"]))
    eng.times.copy_(g["time"].repeat(rows // B))
    it.run(eng.step_plan)
    out = fm(eng.out)
    okw = dict(text_embeds=g["text_embeds"], text_mask=g["text_mask"], cond_images=ci, cond_video_frames=pre, **g["extra"])
    with torch.no_grad():
        ref = u3.unet3d_forward(sd, kw, g["x"], g["time"], **okw)
        ref_null = u3.unet3d_forward(sd, kw, g["x"], g["time"], cond_drop_prob=1.0, **okw)
    assert nerr(out[:B], ref) < 5e-3 and nerr(out[B:], ref_null) < 5e-3, (nerr(out[:B], ref), nerr(out[B:], ref_null))
    eng.set_cond_images(ci.flip(0))
    it.run(eng.step_plan)
    assert nerr(fm(eng.out)[:B], ref) > 1e-2, "the conditioning image must matter"


def test_unet3d_plan_readme_structure_vs_oracle(reference_weights):
    """The README video config's structure (`Unet3D(dim = ..., dim_mults = (1, 2, 4, 8))`, README.md:587; dim 16 here) with temporal
    strides on two levels, a transformer block on the last level and memory_efficient off: planner + interpreter vs the fp32 oracle on
    randomised weights (the oracle itself is pinned to the live reference for this structure in tests/test_oracle_vs_reference.py)."""
    from imagen_pytorch_amd import Unet3D
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from oracle import unet3d_oracle as u3
    from oracle.make_golden import derandomise_unet3d
    from plan_interp import run_engine

    kw = dict(dim=16, dim_mults=(1, 2, 4, 8), temporal_strides=(1, 1, 2, 2), layer_attns=(False, False, False, True), text_embed_dim=32,
              cond_dim=32, max_text_len=16, attn_pool_num_latents=8, attn_heads=2)
    torch.manual_seed(3)
    u = Unet3D(**kw).eval()
    derandomise_unet3d(u)
    B, Fr, S = 1, 8, 16
    x, t = torch.randn(B, 3, Fr, S, S), torch.tensor([0.3])
    te = torch.randn(B, 9, 32)
    out_c, out_n, eng, _ = run_engine(UnetEngine3D(u, 2 * B, B, Fr, S, "cpu", dry=True), x, t, te)
    sd = u.state_dict()
    with torch.no_grad():
        ref_c = u3.unet3d_forward(sd, kw, x, t, text_embeds=te)
        ref_n = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=1.0)
    assert ref_c.abs().mean() > 0.05
    e_c, e_n = nerr(out_c, ref_c), nerr(out_n, ref_n)
    assert e_c < 5e-3 and e_n < 5e-3, (e_c, e_n)
    # the output stage reads its input twice against split-precision weights (engine3d.SPLIT_OUTPUT_STAGE): final_conv and block1 of final_res_block
    split = {label for _, p, label in eng.step_plan.ops if label in ("final_conv", "final_res_block.block1") and p.x2 == p.x1 and p.C2 == p.C1 > 0}
    assert split == {"final_conv", "final_res_block.block1"}, split


def test_split_output_stage_does_not_worsen_a_single_video_forward(reference_weights, monkeypatch):
    """the CPU replay of the Heun video trajectory moved 2.9e-2 -> 4.2e-2 when the output stage got split-precision weights, and
    its bar went 3e-2 -> 5e-2 with 'chaotic trajectory' as the reason.  This is the check that separates chaos from regression: ONE denoiser
    forward of that test's own stage-1 toy unet (tests/golden/sample_tiny_video.pt), through the planner + interpreter, against the fp32 oracle —
    with engine3d.SPLIT_OUTPUT_STAGE on it must not be further from the oracle than with it off."""
    from imagen_pytorch_amd import Unet3D, engine3d
    from imagen_pytorch_amd.engine3d import UnetEngine3D
    from oracle import unet3d_oracle as u3
    from plan_interp import run_engine

    g = torch.load(os.path.join(GOLDEN, "sample_tiny_video.pt"), weights_only=False)
    spec = g["unets"][0]
    kw, sd = spec["kwargs"], spec["state_dict"]
    B, Fr, S = 2, g["frames"], g["image_sizes"][0]
    torch.manual_seed(11)
    x, t, te = torch.randn(B, 3, Fr, S, S), torch.tensor([0.4, -0.8]), g["text_embeds"]
    with torch.no_grad():
        ref_c = u3.unet3d_forward(sd, kw, x, t, text_embeds=te)
        ref_n = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=1.0)
    errs = {}
    for split in (0, 1):
        monkeypatch.setattr(engine3d, "SPLIT_OUTPUT_STAGE", split)
        u = Unet3D(**kw).eval()
        u.load_state_dict(sd)
        out_c, out_n, eng, _ = run_engine(UnetEngine3D(u, 2 * B, B, Fr, S, "cpu", dry=True), x, t, te)
        n_split = sum(1 for _, p, label in eng.step_plan.ops if label in ("final_conv", "final_res_block.block1") and p.x2 == p.x1 and p.C2 == p.C1 > 0)
        assert n_split == (2 if split else 0), (split, n_split)
        errs[split] = (nerr(out_c, ref_c), nerr(out_n, ref_n))
    assert max(errs[1]) < 5e-3, errs
    assert errs[1][0] <= errs[0][0] * 1.02 and errs[1][1] <= errs[0][1] * 1.02, errs


def test_unet_plan_without_text_mask(reference_weights):
    """`text_mask=None` with fewer tokens than max_text_len: the zero-padded positions stay ZERO tokens (ip.py:1617-1632 only applies
    the null embedding through a mask); a plan that masked them out instead is what this test caught."""
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.engine import UnetEngine
    from oracle import unet_oracle as uo
    from plan_interp import run_engine

    g = torch.load(os.path.join(GOLDEN, "unet_tiny_base.pt"), weights_only=False)
    u = Unet(**g["kwargs"]).eval()
    u.load_state_dict(g["state_dict"])
    B, S = g["x"].shape[0], g["x"].shape[-1]
    assert g["text_embeds"].shape[1] < g["kwargs"]["max_text_len"]
    out, _, _, _ = run_engine(UnetEngine(u, B, B, S, "cpu", dry=True), g["x"], g["time"], g["text_embeds"], None)
    with torch.no_grad():
        ref = uo.unet_forward(g["state_dict"], g["kwargs"], g["x"], g["time"], text_embeds=g["text_embeds"], text_mask=None)
    assert nerr(out, ref) < 5e-3
    assert nerr(out, g["out_cond"]) > 2e-2     # the masked run of the fixture is a different function


@pytest.mark.parametrize("name", list(__import__("unet_config_sweep").SWEEP))
def test_unet_plan_config_sweep(name, reference_weights):
    """Planner + interpreter vs the oracle over constructor-flag combinations the GPU fixtures do not cover (memory-efficient layout,
    no attention pooling, unconditional, deeper transformer blocks, no final resnet block, plain init conv, three levels, ...)."""
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.engine import UnetEngine
    from oracle import unet_oracle as uo
    from plan_interp import Interpreter, register_engine
    from unet_config_sweep import SWEEP, cond_images_for, self_cond_for

    kw = SWEEP[name]
    torch.manual_seed(1)
    u = Unet(**kw).eval()
    torch.nn.init.normal_(u.final_conv.weight, std=0.05)
    torch.nn.init.normal_(u.final_conv.bias, std=0.05)
    B, S = 2, 16
    torch.manual_seed(5)
    x, t = torch.randn(B, 3, S, S), torch.tensor([0.4, -1.7])
    with_text = kw.get("cond_on_text", True)
    te = torch.randn(B, 7, kw["text_embed_dim"]) if with_text else None
    extra = dict(lowres_cond_img=torch.randn(B, 3, S, S), lowres_noise_times=torch.tensor([0.9, 0.9])) if kw.get("lowres_cond") else {}
    eng = UnetEngine(u, 2 * B, B, S, "cpu", with_text=with_text, dry=True)
    keep = torch.ones(2 * B, dtype=torch.bool)
    keep[B:] = False
    eng.set_conditioning(text_embeds=te, text_mask=None, keep=keep, lowres_noise_times=extra.get("lowres_noise_times"))
    it = Interpreter()
    register_engine(it, eng)
    it.run(eng._static_plans[te.shape[1] if with_text else 0][0])
    cond_images, self_cond = cond_images_for(kw, B), self_cond_for(kw, B)
    if cond_images is not None:
        eng.set_cond_images(cond_images)
        if eng._cond_pack is not None:       # (with self-conditioning the step plan packs both)
            it.run(eng._cond_pack)
        extra["cond_images"] = cond_images
    if self_cond is not None:
        eng.set_self_cond(self_cond)
        extra["self_cond"] = self_cond
    eng.x_in.copy_(x)
    if eng.lowres:
        eng.lowres_in.copy_(extra["lowres_cond_img"])
    eng.times.copy_(t.repeat(2))
    it.run(eng.step_plan)
    sd = u.state_dict()
    with torch.no_grad():
        ref_c = uo.unet_forward(sd, kw, x, t, text_embeds=te, **extra)
        ref_n = uo.unet_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=1.0, **extra)
    e_c, e_n = nerr(eng.out[:B], ref_c), nerr(eng.out[B:], ref_n)
    assert e_c < 1e-2 and e_n < 1e-2, (name, e_c, e_n)


def test_unet_plan_with_big_tile_family(reference_weights, monkeypatch):
    """The planner path of the big-tile all-DMA family (ops.big_cfg -> conv_big.hip; engine._resnet_block1 / _resnet_block2: ACT_PREP in front of it, with the
    statistics reduced by the pass itself where no producer emitted them), which the benchmark-sized layers take on the GPU, forced onto
    a small model (its workgroup threshold lowered): buffer wiring, folded gains and launch order vs the oracle."""
    from imagen_pytorch_amd import ops

    monkeypatch.setattr(ops, "BIG_MIN_WGS", 1)
    seen = dict(prep=0, self_stat=0, big=0, resprep=0, asked=0)
    real_prep, real_igemm, real_rp, real_req = ops.act_prep, ops.igemm, ops.rowchain_resprep, ops.request_prep

    def resprep(plan, *a, **k):
        seen["resprep"] += 1
        return real_rp(plan, *a, **k)

    def request(*a, **k):
        xa = real_req(*a, **k)
        seen["asked"] += xa is not None
        return xa

    def prep(plan, *a, **k):
        seen["prep"] += 1
        seen["self_stat"] += bool(k.get("self_stat"))
        return real_prep(plan, *a, **k)

    def igemm(plan, *a, **k):
        p = real_igemm(plan, *a, **k)
        seen["big"] += ops.cfg_table()[p.cfg][3] == 5
        return p

    monkeypatch.setattr(ops, "act_prep", prep)
    monkeypatch.setattr(ops, "igemm", igemm)
    monkeypatch.setattr(ops, "rowchain_resprep", resprep)
    monkeypatch.setattr(ops, "request_prep", request)
    test_unet_plan_config_sweep("dim32_three_levels", reference_weights)
    assert seen["big"] >= 4 and seen["prep"] >= 2, seen
    test_unet_plan_config_sweep("dim64_three_levels", reference_weights)      # 256-channel blocks: block2's prologue pass reduces its own statistics
    assert seen["self_stat"] >= 1, seen
    # round 5: on these levels the res_conv + gate tail of an up block is a ROWCHAIN launch (RESPREP), and the block behind it takes its
    # activated input from that launch instead of an ACT_PREP pass
    assert seen["resprep"] >= 2 and seen["asked"] >= 1, seen


def test_resprep_never_reads_skip_statistics_computed_behind_it(reference_weights, monkeypatch):
    """request_prep wires the skip tensor's sums of squares into the EARLIER launch that produced x (RESPREP).  When no producer
    emitted them, engine._ssq_of appends a ROWSTAT at the current plan position — behind that launch — so they must not be offered to it: the
    block falls back to its ACT_PREP pass.  Here the down path's convs are kept from emitting statistics; the plan must still match the oracle,
    and no request may carry a tensor that a late ROWSTAT fills."""
    from imagen_pytorch_amd import engine, ops

    monkeypatch.setattr(ops, "BIG_MIN_WGS", 1)
    real_igemm, real_req, real_ssq_of = ops.igemm, ops.request_prep, engine.UnetEngine._ssq_of
    late, seen = [], dict(offered_late=0, refused=0, stripped=0)

    def igemm(plan, *a, **k):
        if str(k.get("label", "")).startswith("downs.") and k.get("ssq_out") is not None:
            k = dict(k, ssq_out=None)
            seen["stripped"] += 1
        return real_igemm(plan, *a, **k)

    def ssq_of(self, plan, a, label):
        fresh = a.ssq is None
        t = real_ssq_of(self, plan, a, label)
        if fresh:
            late.append(t)
        return t

    def request(x, skip, ssq_skip, ssq_wb, pa):
        seen["offered_late"] += any(ssq_skip is t for t in late)
        seen["refused"] += skip is not None and ssq_skip is None
        return real_req(x, skip, ssq_skip, ssq_wb, pa)

    monkeypatch.setattr(ops, "igemm", igemm)
    monkeypatch.setattr(ops, "request_prep", request)
    monkeypatch.setattr(engine.UnetEngine, "_ssq_of", ssq_of)
    test_unet_plan_config_sweep("dim32_three_levels", reference_weights)
    assert seen["stripped"] >= 2 and seen["refused"] >= 1 and seen["offered_late"] == 0, seen


@pytest.mark.parametrize("name", ["cond_images_3", "self_cond_lowres_cond_images_5", "plain_init_conv_no_mid_attn", "memory_efficient_lowres"])
def test_init_conv_shared_between_cfg_rows_config_sweep(name, reference_weights, monkeypatch):
    """The init conv on the B distinct images (+ row copies) with a second input tensor (conditioning image / self-conditioning), a plain
    7x7 init conv and the memory-efficient layout, vs the oracle (threshold lowered: on the GPU only the large stages take the path)."""
    from imagen_pytorch_amd import engine

    monkeypatch.setattr(engine, "INIT_CONV_SHARED_MIN_PIXELS", 1)
    test_unet_plan_config_sweep(name, reference_weights)


@pytest.mark.parametrize("name", ["unconditional", "memory_efficient_lowres", "four_time_tokens_init_dim", "no_attn_pool", "head_dim_32",
                                  "three_levels_no_gca", "self_cond"])
def test_time_table_plan_equals_per_step_chain(name, reference_weights):
    """engine.enable_time_table over constructor-flag combinations: the batched all-steps pass + one STEP_SLICE copy per step gives the step
    plan exactly what the per-step conditioning chain computes (same op contracts on more rows), for several rows of a coefficient table."""
    from imagen_pytorch_amd import Unet
    from imagen_pytorch_amd.engine import UnetEngine
    from plan_interp import Interpreter, register_engine
    from unet_config_sweep import SWEEP, cond_images_for, self_cond_for

    kw = SWEEP[name]
    torch.manual_seed(1)
    u = Unet(**kw).eval()
    torch.nn.init.normal_(u.final_conv.weight, std=0.05)
    B, S = 2, 16
    torch.manual_seed(5)
    x = torch.randn(B, 3, S, S)
    with_text = kw.get("cond_on_text", True)
    te = torch.randn(B, 7, kw["text_embed_dim"]) if with_text else None
    lowres = dict(lowres_cond_img=torch.randn(B, 3, S, S), lowres_noise_times=torch.tensor([0.9, 0.9])) if kw.get("lowres_cond") else {}
    eng = UnetEngine(u, 2 * B, B, S, "cpu", with_text=with_text, dry=True)
    keep = torch.ones(2 * B, dtype=torch.bool)
    keep[B:] = False
    eng.set_conditioning(text_embeds=te, text_mask=None, keep=keep, lowres_noise_times=lowres.get("lowres_noise_times"))
    it = Interpreter()
    register_engine(it, eng)
    it.run(eng._static_plans[te.shape[1] if with_text else 0][0])
    if eng.self_cond_in is not None:
        eng.set_self_cond(self_cond_for(kw, B))
    coef = torch.zeros(5, 8)
    coef[:, 6] = torch.tensor([2.5, 0.7, -0.4, -1.9, -3.3])          # the log-SNR column the time embedding reads
    step_ptr = torch.zeros(1, dtype=torch.int32)
    fast = eng.enable_time_table(coef, step_ptr)
    assert fast is not None and len(fast) == len(eng.step_plan) - sum(l in eng._TIME_CHAIN for _, _, l in eng.step_plan.ops) + 1
    it.mem.register(step_ptr)
    it.run(eng._tt_plan)
    eng.x_in.copy_(x)
    if eng.lowres:
        eng.lowres_in.copy_(lowres["lowres_cond_img"])
    for row in (0, 3, 4):
        step_ptr.fill_(row)
        it.run(fast)
        got = eng.out.clone()
        eng.out.zero_()
        eng.times.fill_(float(coef[row, 6]))
        it.run(eng.step_plan)
        # bit-identical on the GPU (a GEMM's k-loop order does not depend on its row count: tests/test_model_gpu.py); torch's CPU kernels
        # behind the interpreter choose their blocking by problem size, so fp32 sums may differ in the last bits here
        assert nerr(got, eng.out) < 1e-3, (name, row, nerr(got, eng.out))   # (one flipped fp16 rounding upstream reaches the output at ~3e-4)


def _dry_engines(monkeypatch):
    """Make Imagen._stage build its engines on CPU memory without launching (test-side patch; the product has no such switch)."""
    import functools

    from imagen_pytorch_amd import engine

    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))


def test_time_table_pass_in_chunks(reference_weights, monkeypatch):
    """Round 6: the batched all-steps pass of the per-request time table runs in chunks of steps over ONE set of intermediates (the time MLPs' output
    alone is as large as both scale / shift tables).  Five steps in chunks of 2 + 2 + 1 and in five chunks of one: the tables are what the
    single-pass plan fills (the same kernels on fewer rows per launch), so the step plan still equals the per-step chain."""
    from imagen_pytorch_amd import engine

    seen = []
    real = engine.UnetEngine.enable_time_table

    def spy(self, coef, step_ptr):
        out = real(self, coef, step_ptr)
        seen.append(dict(self.time_table_layout))
        return out

    monkeypatch.setattr(engine.UnetEngine, "enable_time_table", spy)
    test_time_table_plan_equals_per_step_chain("memory_efficient_lowres", reference_weights)
    assert seen[-1]["chunks"] == 1
    work = seen[-1]["work_bytes_unchunked"]
    monkeypatch.setattr(engine, "TIME_TABLE_CHUNK_BYTES", work // 3 + 1)       # 3 chunks: 2 + 2 + 1 steps
    test_time_table_plan_equals_per_step_chain("memory_efficient_lowres", reference_weights)
    assert (seen[-1]["chunks"], seen[-1]["steps_per_chunk"]) == (3, 2), seen[-1]
    monkeypatch.setattr(engine, "TIME_TABLE_CHUNK_BYTES", 1)                   # one step per chunk
    test_time_table_plan_equals_per_step_chain("four_time_tokens_init_dim", reference_weights)
    assert (seen[-1]["chunks"], seen[-1]["steps_per_chunk"]) == (5, 1), seen[-1]



def test_sampler_stage_plan_without_time_table(reference_weights, monkeypatch):
    """The per-step conditioning chain inside the sampling plan (IMAGEN_TIME_TABLE=0; also what inpainting and the step-level API run)."""
    from imagen_pytorch_amd import imagen as _im

    monkeypatch.setattr(_im, "TIME_TABLE", 0)
    test_sampler_stage_plan_on_cpu("plain", reference_weights, monkeypatch)


def _stage0_loop(imagen, st, it, g, noise, *, resample_times=0, known=None, mask=None, init=None, skip=0):
    """The driver loop of Imagen.p_sample_loop for one stage (ip.py:2167-2289), with the per-step plan run by the interpreter."""
    eng, T = st['eng'], st['T']
    R = max(resample_times, 1)
    eng.x_in.copy_(noise[("init", 0)])
    if init is not None:
        eng.x_in.add_(init)
    if resample_times:
        st['known'].copy_(known)
        st['mask'].copy_(mask)
    st['step_ptr'].fill_(skip * R)
    for i in range(skip, T):
        for r in reversed(range(R)):
            if resample_times:
                st['noise_blend'].copy_(noise[("inpaint", 0, i, r)])
                st['noise'].copy_(noise[("step", 0, i, r)])
                if r > 0 and i < T - 1:
                    st['noise_renoise'].copy_(noise[("renoise", 0, i, r)])
            else:
                st['noise'].copy_(noise[("step", 0, i)])
            it.run(st['plan'])
    out = st['final']
    if resample_times:
        out = torch.where(st['mask'] != 0, (st['known'] + 1) * 0.5, out)
    return out


@pytest.mark.parametrize("run", ["plain", "init_skip", "inpaint"])
def test_sampler_stage_plan_on_cpu(run, reference_weights, monkeypatch):
    """Stage 1 of the tiny cascade: denoiser plan + CFG / x0 / exact quantile / posterior step (+ the inpainting blend and re-noising
    ops) wired by Imagen._stage, replayed on the CPU with the reference's recorded Gaussian draws, vs the reference's stage-1 image."""
    import torch.nn.functional as F

    from imagen_pytorch_amd import Imagen, Unet
    from plan_interp import Interpreter, register_engine

    _dry_engines(monkeypatch)
    if run == "plain":
        g = torch.load(os.path.join(GOLDEN, "sample_tiny_cascade.pt"), weights_only=False)
        r = dict(noise=g["noise"], outputs=g["outputs"])
    else:
        g = torch.load(os.path.join(GOLDEN, "sample_tiny_options.pt"), weights_only=False)
        r = g["runs"][run]
    unets = [Unet(**spec["kwargs"]).eval() for spec in g["unets"]]
    imagen = Imagen(unets, image_sizes=g["image_sizes"], timesteps=g["timesteps"], text_embed_dim=32, cond_drop_prob=0.1)
    for u, spec in zip(imagen.unets, g["unets"]):
        u.load_state_dict(spec["state_dict"])
    B, S = g["text_embeds"].shape[0], g["image_sizes"][0]
    R = r.get("inpaint_resample_times", 0) if run == "inpaint" else 0
    st = imagen._stage(0, B, torch.device("cpu"), cond_scale=g["cond_scale"], with_text=True, inject_noise=True, sample_offset=0, resample_times=R)
    eng = st['eng']
    keep = torch.ones(2 * B, dtype=torch.bool)
    keep[B:] = False
    te = g["text_embeds"]
    eng.set_conditioning(text_embeds=te, text_mask=torch.any(te != 0., dim=-1), keep=keep, lowres_noise_times=None)
    it = Interpreter()
    register_engine(it, eng)
    it.run(eng._static_plans[te.shape[1]][0])
    if eng._tt_plan is not None:               # the timestep-only conditioning of all steps in one batched pass (engine.enable_time_table)
        assert run != "inpaint" and any(l == "time_table_rows" for _, _, l in st['plan'].ops)
        it.run(eng._tt_plan)
    else:
        from imagen_pytorch_amd import imagen as _im
        assert run == "inpaint" or not _im.TIME_TABLE   # (the inpainting plan's counter runs over inner iterations: it keeps the per-step chain)
    kw = {}
    if run == "init_skip":
        kw = dict(init=r["init_images"] * 2 - 1, skip=r["skip_steps"])
    if run == "inpaint":
        known = F.interpolate(r["inpaint_images"] * 2 - 1, S, mode="nearest")
        mask = F.interpolate(r["inpaint_masks"][:, None].float(), S, mode="nearest").bool().expand(-1, 3, -1, -1).float()
        kw = dict(resample_times=R, known=known, mask=mask)
    out = _stage0_loop(imagen, st, it, g, r["noise"], **kw)
    e = nerr(out, r["outputs"][0])
    assert e < 2e-2, e                      # the bar of tests/test_model_gpu.py::test_sample_vs_reference_fixture


@pytest.mark.parametrize("tds", [(1, 1), (2, 1)])
def test_video_sampler_stage_plans_on_cpu(tds, reference_weights, monkeypatch):
    """Imagen-Video sampling, host logic: both Unet3D stages of the tiny video cascade (frame-major sampler state, per-clip dynamic
    threshold, low-res clip conditioning) wired by Imagen._stage and replayed on the CPU with the reference's recorded draws."""
    import functools

    import torch.nn.functional as F

    from imagen_pytorch_amd import Imagen, Unet3D, engine3d
    from plan_interp import Interpreter, register_engine

    monkeypatch.setattr(engine3d, "UnetEngine3D", functools.partial(engine3d.UnetEngine3D, dry=True))
    g = torch.load(os.path.join(GOLDEN, "sample_tiny_video.pt"), weights_only=False)
    unets = [Unet3D(**spec["kwargs"]).eval() for spec in g["unets"]]
    imagen = Imagen(unets, image_sizes=g["image_sizes"], timesteps=g["timesteps"], text_embed_dim=32, cond_drop_prob=0.1,
                    temporal_downsample_factor=tds)
    assert imagen.is_video
    run = g if tds == (1, 1) else g["tds"]
    for u, spec in zip(imagen.unets, g["unets"]):
        u.load_state_dict(spec["state_dict"])
    te = g["text_embeds"]
    B, T = te.shape[0], g["timesteps"]
    fm = lambda t: t.permute(0, 2, 1, 3, 4).contiguous()      # (b, c, f, h, w) <-> (b, f, c, h, w)
    prev = None
    for idx in range(2):
        Fr = g["frames"] // tds[idx]
        st = imagen._stage(idx, B, torch.device("cpu"), cond_scale=g["cond_scale"], with_text=True, inject_noise=True, sample_offset=0, frames=Fr)
        eng, S = st['eng'], g["image_sizes"][idx]
        assert st['video'] and tuple(eng.x_in.shape) == (B, Fr, 3, S, S)
        lowres_logsnr = None
        it = Interpreter()
        register_engine(it, eng)
        if idx > 0:   # what Imagen._sample does with LOWRES_PREP (ip.py:2443-2449): nearest resize per frame, normalise, augment at level 0.2
            a, s, lsnr = imagen.lowres_noise_schedule.q_sample_coefficients(imagen.lowres_sample_noise_level)
            if prev.shape[1] != Fr:                         # the frame-axis part of resize_video_to, as Imagen._sample does it
                prev = prev[:, (torch.arange(Fr) * prev.shape[1]) // Fr]
            up = F.interpolate(prev.reshape(-1, *prev.shape[-3:]), S, mode="nearest").reshape(B, Fr, 3, S, S)
            eng.lowres_in.copy_(a * (up * 2 - 1) + s * fm(run["noise"][("lowres", idx)]))
            lowres_logsnr = torch.full((B,), lsnr)
        keep = torch.ones(2 * B, dtype=torch.bool)
        keep[B:] = False
        eng.set_conditioning(text_embeds=te, text_mask=torch.any(te != 0., dim=-1), keep=keep, lowres_noise_times=lowres_logsnr)
        it.run(eng._static_plans[te.shape[1]][0])
        eng.x_in.copy_(fm(run["noise"][("init", idx)]))
        st['step_ptr'].zero_()
        for i in range(T):
            st['noise'].copy_(fm(run["noise"][("step", idx, i)]))
            it.run(st['plan'])
        prev = st['final'].clone()
        e = nerr(fm(prev), run["outputs"][idx])
        assert e < 2e-2, (idx, e)


def test_elucidated_stage_plan_on_cpu(reference_weights, monkeypatch):
    """ElucidatedImagen stage 1 (Karras schedule, churn, preconditioning through CFG_X0, dynamic threshold, Heun correction as LINCOMB
    ops over device tables): the two plans of ElucidatedImagen._stage replayed on the CPU vs the reference's recorded run."""
    from imagen_pytorch_amd import ElucidatedImagen, Unet
    from plan_interp import Interpreter, register_engine

    _dry_engines(monkeypatch)
    g = torch.load(os.path.join(GOLDEN, "sample_tiny_elucidated.pt"), weights_only=False)
    unets = []
    for spec in g["unets"]:
        kw = {k: v for k, v in spec["kwargs"].items() if k != "lowres_cond"}
        unets.append(Unet(**kw, lowres_cond=spec["kwargs"]["lowres_cond"]).eval())
    model = ElucidatedImagen(tuple(unets), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["hparams"]).eval()
    for m, spec in zip(model.unets, g["unets"]):
        m.load_state_dict(spec["state_dict"])
    te = g["text_embeds"]
    B = te.shape[0]
    st = model._stage(0, B, torch.device("cpu"), cond_scale=g["cond_scale"], with_text=True, inject_noise=True, sample_offset=0)
    eng, T, x = st['eng'], st['T'], st['x']
    keep = torch.ones(2 * B, dtype=torch.bool)
    keep[B:] = False
    eng.set_conditioning(text_embeds=te, text_mask=torch.any(te != 0., dim=-1), keep=keep, lowres_noise_times=None)
    it = Interpreter()
    register_engine(it, eng)
    for buf in (x, st['final']):
        it.mem.register(buf)
    it.run(eng._static_plans[te.shape[1]][0])
    assert eng._tt_plan is not None and sum(l == "time_table_rows" for _, _, l in st['plan'].ops) == 2   # both evaluations of a Heun step
    it.run(eng._tt_plan)                       # the timestep-only conditioning of all 2T evaluations in one batched pass
    x.copy_(g["noise"][("init", 0)] * float(st['w_init'][0, 0]))        # images = init_sigma * randn (el.py:440-442)
    st['step_ptr'].zero_()
    for i in range(T):
        st['noise'].copy_(g["noise"][("step", 0, i)])
        it.run(st['last'] if i == T - 1 else st['plan'])
    e = nerr(st['final'], g["outputs"][0])
    assert e < 3e-2, e     # 1.5e-2 here; the GPU path measures 6e-3 on this stage (the EDM loop amplifies per-evaluation fp16 noise, sigma_max = 80)
