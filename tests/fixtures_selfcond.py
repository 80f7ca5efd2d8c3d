"""The loaders and model builders of the self-conditioning fixtures (tests/golden/selfcond_*.pt, tools/make_selfcond_golden.py).
TEST INFRASTRUCTURE, never imported by the product."""
from __future__ import annotations

from fixtures_common import GOLDEN, load, nerr, unpack_state_dict  # noqa: F401


def image_fixture():
    """(runs record, [unet record per stage]) of fixture (b): ElucidatedImagen over two Unet(self_cond=True) stages."""
    g = load("selfcond_image_runs.pt")
    return g, [load(n) for n in g["weights_from"]]


def video_fixture():
    """(record, unet record) of fixtures (a) and (c): one Unet3D(self_cond=True)."""
    g = load("selfcond_video.pt")
    return g, load(g["weights_from"])


def image_model(device="cpu", **over):
    from imagen_pytorch_amd import ElucidatedImagen, Unet

    g, specs = image_fixture()
    unets = [Unet(**{**s["kwargs"], **over}).eval() for s in specs]
    model = ElucidatedImagen(tuple(unets), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["hparams"])
    if str(device) != "cpu":
        model = model.to(device)
    for u, s in zip(model.unets, specs):
        u.load_state_dict(unpack_state_dict(s))
    return model.eval()


def video_unet():
    from imagen_pytorch_amd import Unet3D

    _, spec = video_fixture()
    u = Unet3D(**spec["kwargs"]).eval()
    u.load_state_dict(unpack_state_dict(spec))
    return u


def video_model(kind, device="cpu"):
    """kind 'ddpm': Imagen, 'edm': ElucidatedImagen over the one video unet."""
    from imagen_pytorch_amd import ElucidatedImagen, Imagen

    g, spec = video_fixture()
    if kind == "ddpm":
        model = Imagen((video_unet(),), image_sizes=g["image_sizes"], timesteps=g["ddpm"]["timesteps"], text_embed_dim=32, cond_drop_prob=0.1)
    else:
        model = ElucidatedImagen((video_unet(),), image_sizes=g["image_sizes"], text_embed_dim=32, cond_drop_prob=0.1, **g["edm"]["hparams"])
    if str(device) != "cpu":
        model = model.to(device)
    model.unets[0].load_state_dict(unpack_state_dict(spec))
    return model.eval()

