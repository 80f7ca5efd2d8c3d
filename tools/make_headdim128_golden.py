#!/usr/bin/env python
"""tests/golden/headdim128_*.pt: recorded runs of the LIVE REFERENCE on unets with attn_dim_head = 128, every Gaussian draw recorded.

    python tools/make_headdim128_golden.py        # needs the reference's tree (oracle/ref_shim.py); CPU only

  headdim128_forward.pt   two tiny unets at 16^2, batch 2 — `hd128` (dim 16, dim_mults (1, 2), 2 heads x 128, layer_attns and
                          layer_cross_attns (False, True), cond_dim 32, 8 pooled latents) and `hd128_lin` (the same with
                          use_linear_cross_attn=(True, False)) — each with its inputs and the reference's fp32 forward on the cond and the null branch
  headdim128_sample.pt    a 2-stage cascade (16 -> 32), `hd128` and `sr` (the same unet with lowres_cond): Imagen.sample (3 DDPM steps) and
                          ElucidatedImagen.sample (3 Karras steps) at cond_scale 3
  headdim128_w_<unet>_<0|1>.pt  the parameters of `hd128`, `hd128_lin` and `sr`, each in two halves (572 k parameters are 1.1 MiB of fp16; a
                          committed file holds at most 1 MiB)

Only tensors and constructor kwargs are stored.  The weights are rounded to fp16 BEFORE the reference runs and stored as ONE flat fp16 tensor
per unet plus the ordered (key, shape) index (tools/make_selfcond_golden.py).

Every case is also run at attn_dim_head = 64 from the same seeds (`*_hd64` entries: outputs only).  The two widths must lie further apart than
DISCRIMINATION times the bar of the tests that compare with them, so that no test passes on the wrong width: asserted here, re-asserted by
the tests from the stored tensors.  Everything is recorded twice and must come out equal bit for bit."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from make_selfcond_golden import edm_tags, pack_unet, round_to_half  # noqa: E402
from oracle.make_golden import ELUCIDATED_HP, _derandomise, _record_draws  # noqa: E402
from oracle.ref_shim import load_reference  # noqa: E402
from fixtures_common import nerr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DISCRIMINATION = 10.0
# the bars of the tests that compare with each run: the tiny-unet forward bar of the head-dim-32 planner tests (tests/test_linear_xattn_cpu.py)
# and the sampler bars of tests/test_sample_cpu_replay.py
BAR = {"forward": 1e-2, "ddpm": 2e-2, "edm": 3e-2}
BASE = dict(dim=16, dim_mults=(1, 2), num_resnet_blocks=1, attn_heads=2, layer_attns=(False, True), layer_cross_attns=(False, True), cond_dim=32,
            text_embed_dim=32, attn_pool_num_latents=8, max_text_len=16)
MODELS = {"hd128": dict(BASE), "hd128_lin": dict(BASE, use_linear_cross_attn=(True, False)), "sr": dict(BASE, lowres_cond=True)}
SEED = {"hd128": 131, "hd128_lin": 137, "sr": 163}
T = 3
HP = dict(ELUCIDATED_HP, num_sample_steps=T)


def build(ip, name, dh):
    torch.manual_seed(SEED[name])
    u = ip.Unet(**MODELS[name], attn_dim_head=dh).eval()
    _derandomise(u)
    round_to_half(u)
    return u


def forward_record(u):
    g = torch.Generator().manual_seed(139)
    B, S = 2, 16
    x = torch.randn(B, 3, S, S, generator=g)
    time = torch.tensor([0.6, -1.9])
    text_embeds = torch.randn(B, 11, 32, generator=g)
    text_mask = torch.ones(B, 11, dtype=torch.bool)
    text_mask[1, 6:] = False
    rec = dict(x=x, time=time, text_embeds=text_embeds, text_mask=text_mask)
    with torch.no_grad():
        rec["out_cond"] = u(x, time, text_embeds=text_embeds, text_mask=text_mask)
        rec["out_null"] = u(x, time, text_embeds=text_embeds, text_mask=text_mask, cond_drop_prob=1.)
    return rec


def forward_file(ip):
    models = {}
    for name in ("hd128", "hd128_lin"):
        rec = forward_record(build(ip, name, 128))
        far = forward_record(build(ip, name, 64))
        for branch in ("out_cond", "out_null"):
            gap = nerr(rec[branch], far[branch])
            print(f"forward [{name}] {branch}: |head dim 128 - head dim 64| / |64| = {gap:.3f}")
            assert gap >= DISCRIMINATION * BAR["forward"], (name, branch, gap)
            rec[branch + "_hd64"] = far[branch]
        models[name] = rec
    assert any(type(m).__name__ == "LinearCrossAttention" for m in build(ip, "hd128_lin", 128).modules())
    return dict(models=models, forward_bar=BAR["forward"], discrimination=DISCRIMINATION, generator="tools/make_headdim128_golden.py",
                reference="lucidrains/imagen-pytorch v2.0.0 Unet.forward at attn_dim_head = 128 (imagen_pytorch.py:1524-1725)")


def weight_files(ip):
    """{file name: record}: the flat fp16 parameters of each unet in two halves, kwargs and index in the first."""
    files = {}
    for name in MODELS:
        spec = pack_unet(build(ip, name, 128), dict({"lowres_cond": False, **MODELS[name]}, attn_dim_head=128))
        half = spec["flat"].numel() // 2
        files[f"headdim128_w_{name}_0.pt"] = dict(kwargs=spec["kwargs"], index=spec["index"], flat=spec["flat"][:half].clone())
        files[f"headdim128_w_{name}_1.pt"] = dict(flat=spec["flat"][half:].clone())
    return files


def ddpm_tags(draws, steps):
    """Order of the draws (ip.py:2449, 2195, 2160): per stage [low-res augmentation], init, one per step."""
    noise, it = {}, iter(draws)
    for stage in range(2):
        if stage > 0:
            noise[("lowres", stage)] = next(it)
        noise[("init", stage)] = next(it)
        for i in range(steps):
            noise[("step", stage, i)] = next(it)
    assert next(it, None) is None
    return noise


def sample_file(ip, el):
    te = torch.randn(2, 9, 32, generator=torch.Generator().manual_seed(149))
    common = dict(text_embeds=te, cond_scale=3., use_tqdm=False, return_all_unet_outputs=True)
    makers = {"ddpm": lambda us: ip.Imagen(us, image_sizes=(16, 32), timesteps=T, text_embed_dim=32, cond_drop_prob=0.1),
              "edm": lambda us: el.ElucidatedImagen(us, image_sizes=(16, 32), text_embed_dim=32, cond_drop_prob=0.1, **HP)}
    tags = {"ddpm": ddpm_tags, "edm": lambda d, n: edm_tags(d, n, 2)}
    runs = {}
    for kind in ("ddpm", "edm"):
        outs, first = {}, None
        for dh in (128, 64):
            stages = [build(ip, "hd128", dh), build(ip, "sr", dh)]
            model = makers[kind]((ip.Unet(**BASE, attn_dim_head=dh), ip.Unet(**BASE, attn_dim_head=dh))).eval()
            for u, src in zip(model.unets, stages):
                u.load_state_dict(src.state_dict())      # (cast_model_parameters re-instantiated the second unet with lowres_cond)
            torch.manual_seed(157)
            outs[dh], draws = _record_draws(lambda: model.sample(**common))
            first = draws if first is None else first
            assert len(draws) == len(first) and all(torch.equal(a, b) for a, b in zip(draws, first))
        gaps = [nerr(a, b) for a, b in zip(outs[128], outs[64])]
        print(f"{kind}: {len(first)} draws, |head dim 128 - head dim 64| / |64| per stage = {['%.3f' % g for g in gaps]}")
        assert min(gaps) >= DISCRIMINATION * BAR[kind], (kind, gaps)
        runs[kind] = dict(noise=tags[kind](first, T), outputs=[o.clone() for o in outs[128]], outputs_hd64=[o.clone() for o in outs[64]], bar=BAR[kind])
    return dict(unets=("hd128", "sr"), image_sizes=(16, 32), timesteps=T, hparams=dict(HP), cond_scale=3., text_embeds=te, runs=runs,
                discrimination=DISCRIMINATION, generator="tools/make_headdim128_golden.py",
                reference="lucidrains/imagen-pytorch v2.0.0 Imagen.sample / ElucidatedImagen.sample over two Unet(attn_dim_head=128) stages")


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def main():
    ip, el = load_reference("imagen_pytorch"), load_reference("elucidated_imagen")
    w, w2 = weight_files(ip), weight_files(ip)
    jobs = [("headdim128_forward.pt", lambda: forward_file(ip)), ("headdim128_sample.pt", lambda: sample_file(ip, el))]
    jobs += [(name, (lambda name=name, it=iter((w, w2)): next(it)[name])) for name in w]
    for fname, make in jobs:
        rec, again = make(), make()
        assert same(rec, again), f"{fname}: two recordings differ"
        blobs = []
        for r in (rec, again):
            buf = io.BytesIO()
            torch.save(r, buf)
            blobs.append(buf.getvalue())
        assert blobs[0] == blobs[1], f"{fname}: two recordings serialise to different bytes"
        path = os.path.join(GOLDEN, fname)
        with open(path, "wb") as f:
            f.write(blobs[0])
        print(f"wrote {path} ({os.path.getsize(path)} bytes), recorded twice: identical")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
