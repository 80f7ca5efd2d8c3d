#!/usr/bin/env python
"""tests/golden/linxattn_*.pt: recorded runs of the LIVE REFERENCE on unets with Unet(use_linear_cross_attn=...) (LinearCrossAttention,
ip.py:836-874), every Gaussian draw recorded.

    python tools/make_linear_xattn_golden.py        # needs the reference's tree (oracle/ref_shim.py); CPU only

  linxattn_unet.pt    two tiny unets at 16^2 — `lin64` (dim 16, dim_mults (1, 2), layer_cross_attns (False, True), use_linear_cross_attn
                      (True, False), 2 heads x 64) and `twin` (the flag off, layer_cross_attns (True, True); same seed, hence the same weights
                      as `lin64`, stored once) — each with its inputs and the reference's fp32 forward on the cond and the null branch; for
                      `lin64` also the input, context and output of its first LinearCrossAttention module
  linxattn_unet_hd32.pt  `lin32`, the same at 4 heads x 32 (a file of its own: a committed file holds at most 1 MiB)
  linxattn_sample.pt  Imagen.sample (4 DDPM steps) and ElucidatedImagen.sample (4 Karras steps) over `lin64` at cond_scale 3, and the same two
                      runs over `twin` from the same draws

Only tensors and constructor kwargs are stored.  The weights are rounded to fp16 BEFORE the reference runs and stored as ONE flat fp16 tensor
per unet plus the ordered (key, shape) index (tools/make_selfcond_golden.py).

The flag-on and the flag-off recordings must lie further apart than DISCRIMINATION times the bar of the tests that compare with them, so that
no test passes by ignoring the flag: asserted here, re-asserted by the tests from the stored tensors."""
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
# forward: the tests' bar is 1.5 x what the twin measures in the same run — below the 1e-2 every tiny-unet forward test of the suite uses, which
# stands in for it here; samplers: the bars of tests/test_selfcond_gpu.py for the same kind of tiny run
BAR = {"forward": 1e-2, "ddpm": 2e-2, "edm": 3e-2}
BASE = dict(dim=16, cond_dim=16, text_embed_dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), max_text_len=16,
            attn_pool_num_latents=8)
MODELS = {
    "lin64": dict(BASE, layer_cross_attns=(False, True), use_linear_cross_attn=(True, False), attn_heads=2, attn_dim_head=64),
    "lin32": dict(BASE, layer_cross_attns=(False, True), use_linear_cross_attn=(True, False), attn_heads=4, attn_dim_head=32),
    "twin": dict(BASE, layer_cross_attns=(True, True), use_linear_cross_attn=False, attn_heads=2, attn_dim_head=64),
}
SEED = {"lin64": 71, "lin32": 73, "twin": 71}
T = 4
SITE_GAIN = 2.0
HP = dict(ELUCIDATED_HP, num_sample_steps=T)


def build(ip, name):
    torch.manual_seed(SEED[name])
    u = ip.Unet(**MODELS[name]).eval()
    _derandomise(u)
    # the first block of level 0 (down and up side) is where the flag acts: raise the gain of its cross-attention's out-norm (1 in a fresh
    # unet) on every model alike, so that the site's branch weighs against the residual and the two attention forms are told apart
    for blk in (u.downs[0][1], u.ups[-1][0]):
        blk.cross_attn.to_out[1].g.data.mul_(SITE_GAIN)
    round_to_half(u)
    return u


def forward_record(u, name):
    g = torch.Generator().manual_seed(79)
    B, S = 2, 16
    x = torch.randn(B, 3, S, S, generator=g)
    time = torch.tensor([0.6, -1.9])
    text_embeds = torch.randn(B, 11, 32, generator=g)
    text_mask = torch.ones(B, 11, dtype=torch.bool)
    text_mask[1, 6:] = False
    rec = dict(x=x, time=time, text_embeds=text_embeds, text_mask=text_mask)
    site = {}
    handle = None
    if name == "lin64":
        mod = u.downs[0][1].cross_attn
        assert type(mod).__name__ == "LinearCrossAttention"

        def hook(m, args, kwargs, out):
            site.setdefault("x", args[0].detach().clone())
            site.setdefault("context", kwargs["context"].detach().clone())
            site.setdefault("out", out.detach().clone())
        handle = mod.register_forward_hook(hook, with_kwargs=True)
    with torch.no_grad():
        rec["out_cond"] = u(x, time, text_embeds=text_embeds, text_mask=text_mask)
        if handle is not None:
            handle.remove()
        rec["out_null"] = u(x, time, text_embeds=text_embeds, text_mask=text_mask, cond_drop_prob=1.)
    if site:
        rec["site"] = dict(site, module="downs.0.1.cross_attn", heads=MODELS[name]["attn_heads"], dim_head=MODELS[name]["attn_dim_head"])
    return rec


def ddpm_tags(draws, steps):
    noise, it = {("init", 0): draws[0]}, iter(draws[1:])
    for i in range(steps):
        noise[("step", 0, i)] = next(it)
    assert next(it, None) is None
    return noise


def sample_runs(ip, el, units):
    te = torch.randn(2, 9, 32, generator=torch.Generator().manual_seed(83))
    common = dict(text_embeds=te, cond_scale=3., use_tqdm=False, return_all_unet_outputs=True)
    runs = {}
    for kind, make, tags in (("ddpm", lambda u: ip.Imagen((u,), image_sizes=(16,), timesteps=T, text_embed_dim=32, cond_drop_prob=0.1), ddpm_tags),
                             ("edm", lambda u: el.ElucidatedImagen((u,), image_sizes=(16,), text_embed_dim=32, cond_drop_prob=0.1, **HP),
                              lambda d, n: edm_tags(d, n, 1))):
        outs = {}
        for name in ("lin64", "twin"):
            model = make(units[name]).eval()
            model.unets[0].load_state_dict(units[name].state_dict())      # (cast_model_parameters may have re-instantiated the unet)
            torch.manual_seed(107)
            outs[name], draws = _record_draws(lambda: model.sample(**common))
            if name == "lin64":
                first = draws
            assert len(draws) == len(first) and all(torch.equal(a, b) for a, b in zip(draws, first))
        gap = nerr(outs["lin64"][0], outs["twin"][0])
        print(f"{kind}: {len(first)} draws, |flag on - flag off| / |flag off| = {gap:.3f}")
        assert gap >= DISCRIMINATION * BAR[kind], (kind, gap)
        runs[kind] = dict(noise=tags(first, T), outputs=[o.clone() for o in outs["lin64"]], outputs_twin=[o.clone() for o in outs["twin"]], bar=BAR[kind])
    return dict(weights_from=("linxattn_unet.pt", "lin64"), twin_from=("linxattn_unet.pt", "twin"), image_sizes=(16,), timesteps=T, hparams=dict(HP),
                cond_scale=3., text_embeds=te, runs=runs, discrimination=DISCRIMINATION, generator="tools/make_linear_xattn_golden.py",
                reference="lucidrains/imagen-pytorch v2.0.0 Imagen.sample / ElucidatedImagen.sample over Unet(use_linear_cross_attn=(True, False))")


def main():
    ip, el = load_reference("imagen_pytorch"), load_reference("elucidated_imagen")
    units = {name: build(ip, name) for name in MODELS}
    sd_a, sd_t = units["lin64"].state_dict(), units["twin"].state_dict()
    assert list(sd_a) == list(sd_t) and all(torch.equal(sd_a[k], sd_t[k]) for k in sd_a), "the twin carries the weights of lin64"
    models = {}
    for name, u in units.items():
        kw = dict(MODELS[name], lowres_cond=False)
        models[name] = dict(pack_unet(u, kw), forward=forward_record(u, name))
    models["twin"] = dict(kwargs=models["twin"]["kwargs"], weights_of="lin64", forward=models["twin"]["forward"])
    for name in ("lin64", "lin32"):
        assert any(type(m).__name__ == "LinearCrossAttention" for m in units[name].modules())
    for branch in ("out_cond", "out_null"):
        gap = nerr(models["lin64"]["forward"][branch], models["twin"]["forward"][branch])
        print(f"forward {branch}: |flag on - flag off| / |flag off| = {gap:.3f}")
        assert gap >= DISCRIMINATION * BAR["forward"], (branch, gap)
    common = dict(forward_bar_stand_in=BAR["forward"], discrimination=DISCRIMINATION, generator="tools/make_linear_xattn_golden.py",
                  reference="lucidrains/imagen-pytorch v2.0.0 Unet.forward with LinearCrossAttention sites (imagen_pytorch.py:836-874, 1524-1725)")
    path = os.path.join(GOLDEN, "linxattn_unet_hd32.pt")
    torch.save(dict(models={"lin32": models.pop("lin32")}, **common), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)
    path = os.path.join(GOLDEN, "linxattn_unet.pt")
    torch.save(dict(models=models, **common), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)
    path = os.path.join(GOLDEN, "linxattn_sample.pt")
    torch.save(sample_runs(ip, el, units), path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
