"""CPU: self-conditioning under the Karras et al. sampler and in Unet3D stages (ABI 13: LINCOMB thr1_out / thr3_out).

  * an fp32 restatement of the reference's Karras loop WITH self-conditioning (el.py:451, 496, 518, 538), written out here over
    oracle/unet_oracle.py, against the recorded run of the live reference (tests/golden/selfcond_image_runs.pt) and, where its tree is
    present, against the live reference itself with the recorded draws injected — tolerances of tests/test_oracle_golden.py's Elucidated test;
  * the real drivers (ElucidatedImagen.sample, Imagen.sample) replayed through the plan interpreter (tests/plan_interp.py: LINCOMB with
    its thr1_out / thr3_out) against the recorded runs — bars of tests/test_sample_cpu_replay.py's Elucidated / video replays.
    Measured here: image plain 3.3e-3 / 5.4e-3 (stage 1 / stage 2 alone), skip 1.3e-3 / 7.0e-3, inpaint 1.8e-3 / 2.9e-3; video DDPM 1.2e-3,
    video EDM 3.0e-3; Unet3D forward with a clip 6.7e-4 (cond) / 1.9e-3 (CFG), without 2.4e-3; the restatement itself sits at 1.3e-5 / 5.4e-5 /
    9.1e-5 (plain: stage 1, stage 2 alone, chained; max abs), 6.0e-6 / 3.5e-5 / 1.6e-4 (skip), 6.3e-5 / 5.6e-5 / 3.1e-4 (inpaint);
  * the fixtures tell the feature from its absence: the same runs recorded with `self_cond` forced to None lie >= 10 bars away;
  * host logic: strict state_dict loading, an unchanged launch list for unets without self_cond, the launcher's refusals;
  * csrc/sampler.hip's lincomb_kernel on the functional emulation (tests/test_lincomb_thr_out_gpu.py in a child pytest)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_selfcond as sc  # noqa: E402
from fixtures_selfcond import nerr  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401  (the fixture that sends Plan.run / Graph to the interpreter)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


# ------------------------------------------------------------------------------------------------ 1. restatement

def karras_self_cond(net, shape, hp, noise_fn, stage, *, skip_steps=0, known=None, mask=None, R=1):
    """el.py:393-545 with self-conditioning, fp32.  net(x, c_noise, self_cond) -> guided network output."""
    from oracle import elucidated_oracle as eo

    table, init_sigma = eo.step_table(hp)
    images = init_sigma * noise_fn(("init", stage), shape)
    x_start = None                                                                  # el.py:451
    inpainting = known is not None
    R = R if inpainting else 1
    table = list(enumerate(table))[skip_steps:]
    kw = dict(clamp=True, dynamic_threshold=True, percentile=0.95)
    for n_done, (ind, (sigma, sigma_next, gamma)) in enumerate(table):
        is_last = n_done == len(table) - 1
        for r in reversed(range(R)):
            eps = hp["S_noise"] * noise_fn(("step", stage, ind, r) if inpainting else ("step", stage, ind), shape)
            sigma_hat = sigma + gamma * sigma
            added = math.sqrt(sigma_hat ** 2 - sigma ** 2) * eps
            images_hat = images + added
            self_cond = x_start                                                     # el.py:496
            if inpainting:
                images_hat = images_hat * ~mask + (known + added) * mask
            out = eo.preconditioned_forward(lambda x, t: net(x, t, self_cond), images_hat, sigma_hat, hp["sigma_data"], **kw)
            d = (images_hat - out) / sigma_hat
            images_next = images_hat + (sigma_next - sigma_hat) * d
            if sigma_next != 0:
                out_next = eo.preconditioned_forward(lambda x, t: net(x, t, out), images_next, sigma_next, hp["sigma_data"], **kw)   # el.py:518
                d2 = (images_next - out_next) / sigma_next
                images_next = images_hat + 0.5 * (sigma_next - sigma_hat) * (d + d2)
            images = images_next
            if inpainting and not (r == 0 or is_last):
                images = images + (sigma - sigma_next) * noise_fn(("renoise", stage, ind, r), shape)
            x_start = out if sigma_next == 0 else out_next                          # el.py:538
    images = images.clamp(-1.0, 1.0)
    if inpainting:
        images = images * ~mask + known * mask
    return (images + 1) * 0.5


def restated_cascade(run, g, specs, start=None):
    """Both stages (or, with `start` = a stage-1 image, stage 2 alone) of fixture (b)'s run by the restatement above."""
    from oracle import elucidated_oracle as eo
    from oracle import sampler_oracle as so
    from oracle.unet_oracle import unet_forward_with_cond_scale

    hp = dict(eo.DEFAULT_HPARAMS, **g["hparams"])
    te = g["text_embeds"]
    tm = torch.any(te != 0.0, dim=-1)
    b = te.shape[0]
    noise_fn = lambda tag, shape: run["noise"][tag]
    kw = run["kwargs"]
    outs, img = [], start
    for stage, (spec, size) in enumerate(zip(specs, g["image_sizes"])):
        if start is not None and stage == 0:
            continue
        sd, ukw = sc.unpack_state_dict(spec), spec["kwargs"]
        li = lt = None
        if ukw["lowres_cond"]:
            lt = torch.full((b,), 0.2)
            up = F.interpolate(img, size, mode="nearest") * 2 - 1
            a, s = so.alpha_sigma(so.SCHEDULES["linear"](lt).reshape(-1, 1, 1, 1))
            li = a * up + s * noise_fn(("lowres", stage), up.shape)
        net = lambda x, t, self_cond, _sd=sd, _kw=ukw, _li=li, _lt=lt: unet_forward_with_cond_scale(
            _sd, _kw, x, t, cond_scale=g["cond_scale"], text_embeds=te, text_mask=tm, lowres_cond_img=_li, lowres_noise_times=_lt, self_cond=self_cond)
        known = mask = None
        if "inpaint_images" in kw:
            resize = lambda im: im if im.shape[-1] == size else F.interpolate(im, size, mode="nearest")
            known = resize(kw["inpaint_images"] * 2 - 1)
            mask = resize(kw["inpaint_masks"][:, None].float()).bool()
        with torch.no_grad():
            img = karras_self_cond(net, (b, 3, size, size), hp, noise_fn, stage, skip_steps=kw.get("skip_steps", 0) or 0, known=known, mask=mask,
                                   R=kw.get("inpaint_resample_times", 1))
        outs.append(img)
    return outs


@pytest.mark.parametrize("tag", ["plain", "skip", "inpaint"])
def test_restated_karras_loop_matches_reference_fixture(tag):
    """Stage 1 to 2e-4, stage 2 alone (from the reference's stage-1 image) to 2e-4, chained to 2e-3: tests/test_oracle_golden.py
    ::test_elucidated_oracle_matches_reference_fixture's tolerances."""
    g, specs = sc.image_fixture()
    run = g["runs"][tag]
    outs = restated_cascade(run, g, specs)
    alone = restated_cascade(run, g, specs, start=run["outputs"][0])[0]
    d = [(outs[0] - run["outputs"][0]).abs().max().item(), (alone - run["outputs"][1]).abs().max().item(),
         (outs[1] - run["outputs"][1]).abs().max().item()]
    print(f"restated Karras loop with self-conditioning [{tag}]: max abs error stage 1 {d[0]:.2e}, stage 2 alone {d[1]:.2e}, chained {d[2]:.2e}")
    assert d[0] <= 2e-4 and d[1] <= 2e-4 and d[2] <= 2e-3, d
    # and it is the self-conditioning that is being restated: the plain loop is far off
    assert nerr(run["outputs_without_self_cond"][0], outs[0]) > 0.1


def test_restated_karras_loop_matches_live_reference():
    """The same restatement against the live reference run now, the fixture's draws injected into its torch.randn calls in order."""
    from oracle import ref_shim

    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    ip, el = ref_shim.load_reference("imagen_pytorch"), ref_shim.load_reference("elucidated_imagen")
    g, specs = sc.image_fixture()
    run = g["runs"]["plain"]
    unets = [ip.Unet(**{k: v for k, v in s["kwargs"].items()}) for s in specs]
    model = el.ElucidatedImagen(tuple(unets), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["hparams"]).eval()
    for u, s in zip(model.unets, specs):
        u.load_state_dict(sc.unpack_state_dict(s))
    draws = iter(run["noise"].values())               # recorded in call order
    real = torch.randn, torch.randn_like
    torch.randn = lambda *a, **k: next(draws).clone()
    torch.randn_like = lambda x, **k: next(draws).clone()
    try:
        live = model.sample(text_embeds=g["text_embeds"], cond_scale=g["cond_scale"], use_tqdm=False, return_all_unet_outputs=True)
    finally:
        torch.randn, torch.randn_like = real
    assert all(torch.equal(a, b) for a, b in zip(live, run["outputs"])), "the fixture is the live reference's run"
    outs = restated_cascade(run, g, specs)
    assert torch.allclose(outs[0], live[0], atol=2e-4) and torch.allclose(outs[1], live[1], atol=2e-3)


# ------------------------------------------------------------------------------------------------ 2. driver replay

@pytest.mark.parametrize("tag", ["plain", "skip", "inpaint"])
def test_elucidated_self_cond_sample_driver(cpu_backend, tag):
    """ElucidatedImagen.sample over Unet(self_cond=True) stages through the real driver, graph objects and eager, against fixture (b); a
    second call on the cached stage gives the same images (self_cond_in is zeroed again).  Bar: 3e-2
    (tests/test_sample_cpu_replay.py::test_elucidated_sample_driver / test_elucidated_sample_options_driver)."""
    g, _ = sc.image_fixture()
    run = g["runs"][tag]
    model = sc.image_model()
    nf = lambda t, shape: run["noise"][t]
    common = dict(text_embeds=g["text_embeds"], cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=nf, device="cpu", **run["kwargs"])
    outs = model.sample(return_all_unet_outputs=True, **common)
    eager = model.sample(return_all_unet_outputs=True, use_graph=False, **common)
    assert all(torch.equal(a, b) for a, b in zip(outs, eager))
    e0 = nerr(outs[0], run["outputs"][0])
    alone = model.sample(start_at_unet_number=2, start_image_or_video=run["outputs"][0], **common)
    e1 = nerr(alone, run["outputs"][1])
    print(f"self-conditioning EDM replay [{tag}]: stage 1 {e0:.2e}, stage 2 alone {e1:.2e}")
    assert e0 < 3e-2 and e1 < 3e-2, (tag, e0, e1)
    far = nerr(outs[0], run["outputs_without_self_cond"][0])
    assert far > 10 * 3e-2, far


@pytest.mark.parametrize("kind,bar", [("ddpm", 2e-2), ("edm", 5e-2)])
def test_video_self_cond_sample_driver(cpu_backend, kind, bar):
    """Imagen.sample / ElucidatedImagen.sample over a Unet3D(self_cond=True) stage against fixture (c).  Bars: 2e-2
    (test_sample_cpu_replay.py's video DDPM replays) and 5e-2 (::test_video_elucidated_sample_driver)."""
    g, _ = sc.video_fixture()
    run = g[kind]
    model = sc.video_model(kind)
    nf = lambda t, shape: run["noise"][t]
    common = dict(text_embeds=g["text_embeds"], video_frames=g["frames"], cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=nf, device="cpu")
    out = model.sample(**common)
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    assert torch.equal(out, model.sample(use_graph=False, **common))
    e = nerr(out, run["outputs"][0])
    print(f"self-conditioning video {kind} replay: {e:.2e}")
    assert e < bar, (kind, e)


def test_unet3d_self_cond_forward_on_cpu(cpu_backend):
    """Unet3D(self_cond=True).forward through the interpreter against fixture (a), with and without a clip.  Bar of the video forwards: 1e-2
    (2e-2 under CFG), tests/test_video_gpu.py::test_unet3d_forward_vs_reference_fixture."""
    g, _ = sc.video_fixture()
    f = g["forward"]
    u = sc.video_unet()
    kw = dict(text_embeds=f["text_embeds"], text_mask=f["text_mask"])
    e = [nerr(u(f["x"], f["time"], self_cond=f["self_cond"], **kw), f["out_cond"]),
         nerr(u(f["x"], f["time"], **kw), f["out_cond_no_clip"]),
         nerr(u.forward_with_cond_scale(f["x"], f["time"], self_cond=f["self_cond"], cond_scale=3.0, **kw), f["out_cfg"])]
    print(f"Unet3D(self_cond=True) forward: with clip {e[0]:.2e}, without {e[1]:.2e}, cfg {e[2]:.2e}")
    assert e[0] < 1e-2 and e[1] < 1e-2 and e[2] < 2e-2, e


# ------------------------------------------------------------------------------------------------ 3. discrimination

def test_fixtures_tell_self_conditioning_from_its_absence():
    """From the stored tensors alone: every recorded run differs from its twin recorded with `self_cond` forced to None by at least 10x the
    bar the tests above and the GPU tests hold against it (the generator asserts the same when it writes the fixtures)."""
    g, _ = sc.image_fixture()
    assert g["discrimination"] == 10.0 and g["bar"] == 3e-2
    for tag, run in g["runs"].items():
        for a, b in zip(run["outputs_without_self_cond"], run["outputs"]):
            assert nerr(a, b) >= 10 * 3e-2, (tag, nerr(a, b))
    v, _ = sc.video_fixture()
    for kind, bar in (("ddpm", 2e-2), ("edm", 5e-2)):
        assert v[kind]["bar"] == bar
        assert nerr(v[kind]["outputs_without_self_cond"][0], v[kind]["outputs"][0]) >= 10 * bar, kind
    f = v["forward"]
    assert nerr(f["out_cond_no_clip"], f["out_cond"]) >= 10 * 1e-2 and nerr(f["out_cfg_no_clip"], f["out_cfg"]) >= 10 * 1e-2


# ------------------------------------------------------------------------------------------------ 4. host logic

def test_unet3d_self_cond_state_dict_loads_strictly():
    """Keys, order and shapes of a reference Unet3D(self_cond=True) state_dict (fixture (a)); the init conv takes channels * 2 inputs."""
    from imagen_pytorch_amd import Unet3D

    _, spec = sc.video_fixture()
    u = Unet3D(**spec["kwargs"])
    assert u.self_cond
    ours = u.state_dict()
    assert [k for k, _ in spec["index"]] == list(ours) and all(tuple(ours[k].shape) == tuple(s) for k, s in spec["index"])
    u.load_state_dict(sc.unpack_state_dict(spec), strict=True)
    assert all(shape[1] == 6 for k, shape in spec["index"] if k.startswith("init_conv.") and k.endswith("weight"))
    for name in ("cross_embed_downsample", "combine_upsample_fmaps", "init_conv_to_final_conv_residual"):
        with pytest.raises(NotImplementedError):
            Unet3D(**{**spec["kwargs"], name: True})
    with pytest.raises(NotImplementedError):
        Unet3D(**{**spec["kwargs"], "pixel_shuffle_upsample": False})


def test_unet3d_self_cond_refusals(cpu_backend):
    """What Unet3D(self_cond=True) does not take raises NotImplementedError where it is asked for: a conditioning image at construction,
    prompt frames when the stage (or the engine of a bare forward) is built."""
    from imagen_pytorch_amd import Unet3D

    g, spec = sc.video_fixture()
    with pytest.raises(NotImplementedError, match="cond_images_channels"):
        Unet3D(**{**spec["kwargs"], "cond_images_channels": 3})
    prompt = torch.zeros(2, 3, 2, 16, 16)
    for kind in ("ddpm", "edm"):
        for kw in (dict(cond_video_frames=prompt), dict(post_cond_video_frames=prompt)):
            with pytest.raises(NotImplementedError, match="cond_video_frames"):
                sc.video_model(kind).sample(text_embeds=g["text_embeds"], video_frames=g["frames"], cond_scale=g["cond_scale"], use_tqdm=False,
                                            device="cpu", **kw)
    f = g["forward"]
    with pytest.raises(NotImplementedError, match="cond_video_frames"):
        sc.video_unet()(f["x"], f["time"], text_embeds=f["text_embeds"], text_mask=f["text_mask"], cond_video_frames=prompt)


def _dry(monkeypatch):
    import functools

    from imagen_pytorch_amd import engine

    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))


def test_plain_unet_launch_list_is_the_parent_commits(monkeypatch):
    """A stage built for unets without self_cond: op kinds and labels of both plans, plain and inpainting, equal the lists recorded from the
    commit before this feature (tests/golden/elucidated_launch_list_abi12.json), and every LINCOMB carries NULL in the two new fields."""
    from imagen_pytorch_amd import ElucidatedImagen, Unet, _abi

    _dry(monkeypatch)
    g = torch.load(os.path.join(sc.GOLDEN, "sample_tiny_elucidated.pt"), weights_only=False)
    want = json.load(open(os.path.join(sc.GOLDEN, "elucidated_launch_list_abi12.json")))
    model = ElucidatedImagen(tuple(Unet(**s["kwargs"]).eval() for s in g["unets"]), image_sizes=g["image_sizes"], text_embed_dim=32,
                             cond_drop_prob=0.1, **g["hparams"]).eval()
    for m, s in zip(model.unets, g["unets"]):
        m.load_state_dict(s["state_dict"])
    for tag, R in (("plain", 0), ("inpaint", 2)):
        st = model._stage(0, 2, torch.device("cpu"), cond_scale=3.0, with_text=True, inject_noise=True, sample_offset=0,
                          **({"resample_times": R} if R else {}))
        assert st["self_cond"] is None
        for name in ("plan", "last"):
            got = [[int(k), l] for k, _, l in st[name].ops]
            assert got == want[f"{tag}.{name}"], (tag, name)
            lin = [p for k, p, _ in st[name].ops if k == _abi.ENUMS["IMAGEN_OP_LINCOMB"]]
            assert lin and all(not p.thr1_out and not p.thr3_out for p in lin)


def test_self_cond_stage_plans(monkeypatch):
    """With self_cond: the Euler op writes the engine's self_cond_in through thr1_out, the Heun op through thr3_out, the last plan emits
    nothing without resampling and its Euler op does with it; no other launch is added."""
    from imagen_pytorch_amd import _abi

    _dry(monkeypatch)
    model = sc.image_model()
    want = json.load(open(os.path.join(sc.GOLDEN, "elucidated_launch_list_abi12.json")))
    for tag, R in (("plain", 0), ("inpaint", 2)):
        st = model._stage(0, 2, torch.device("cpu"), cond_scale=3.0, with_text=True, inject_noise=True, sample_offset=0,
                          **({"resample_times": R} if R else {}))
        dst = st["eng"].self_cond_in.data_ptr()
        by = {l: p for k, p, l in st["plan"].ops if k == _abi.ENUMS["IMAGEN_OP_LINCOMB"]}
        assert by["edm.euler"].thr1_out == dst and not by["edm.euler"].thr3_out
        assert by["edm.heun"].thr3_out == dst and not by["edm.heun"].thr1_out
        assert not by["edm.x_hat"].thr1_out and not by["edm.x_hat"].thr3_out
        last = {l: p for k, p, l in st["last"].ops if k == _abi.ENUMS["IMAGEN_OP_LINCOMB"]}
        assert (last["edm.euler.final"].thr1_out == dst) if R > 1 else not last["edm.euler.final"].thr1_out
        labels = [l for _, _, l in st["plan"].ops]
        assert labels.count("pack_self_cond") == 2 and labels.index("pack_self_cond") == labels.index("pack_image") + 1
        assert len(labels) == len(want[f"{tag}.plan"]) + 2          # the two packs of the self-conditioning image, nothing else


def _emul_lib():
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    return os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_launcher_refuses_thr_out_without_its_operand():
    """launch_lincomb's host-side checks (the same source the GPU library is built from, here in the emulated library, in a child process):
    thr1_out without t1 and thr3_out without t3 are refused with the message of that check, and nothing is launched."""
    code = ("import torch; from imagen_pytorch_amd import ops; from imagen_pytorch_amd._abi import ImagenHipError\n"
            "ops.current_stream_handle = lambda: 0\n"
            "z = lambda: torch.zeros(2, 8); coef = torch.zeros(1, 8); step = torch.zeros(1, dtype=torch.int32)\n"
            "for kw, frag in ((dict(thr1_out=z()), 'thr1_out needs t1'), (dict(thr3_out=z(), t1=z()), 'thr3_out needs t3')):\n"
            "    plan = ops.Plan(); ops.lincomb(plan, z(), z(), coef, step, B=2, n_per_sample=8, **kw)\n"
            "    try:\n        plan.run(); raise SystemExit('not refused')\n"
            "    except ImagenHipError as e:\n        assert frag in str(e), str(e)\n"
            "print('refused twice')\n")
    env = dict(os.environ, IMAGEN_LIB_PATH=_emul_lib())
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and "refused twice" in r.stdout.decode(), r.stdout.decode()[-2000:]


# ------------------------------------------------------------------------------------------------ 5. the kernel itself, emulated

@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_lincomb_thr_outputs():
    """csrc/sampler.hip's lincomb_kernel, compiled by tools/emul, on every combination of thr_mode 0 / 1 / 2, each output NULL or set and
    mask set or not, against fp64 with sentinels around both outputs (tests/test_lincomb_thr_out_gpu.py in a child pytest)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_emul_lib(), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_lincomb_thr_out_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]
    assert int(out.split(" passed")[0].split()[-1]) >= 3 * 3 * 4 * 2, out[-800:]
