#!/usr/bin/env python
"""tests/golden/sample_tiny_video_hd32.pt: Imagen.sample of the LIVE REFERENCE over two tiny Unet3D stages with 2 attention heads of 32 dims
(8 -> 16 pixels, 4 frames, 2 steps, CFG 3), every Gaussian draw recorded — the head-dim-32 sibling of sample_tiny_video.pt.

    python tools/make_video_headdim32_fixture.py        # needs the reference's tree (oracle/ref_shim.py); CPU only

Only tensors and constructor kwargs are stored.  The weights are rounded to fp16 BEFORE the reference runs and stored as fp16, so the fixture
holds exactly the weights the recorded outputs were computed from at half the size; each stage's state_dict is ONE flat fp16 tensor plus the
ordered (key, shape) index (900 small tensors cost a quarter of a megabyte in container overhead): tests/fixtures_common.py unpack_state_dict()
restores it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from fixtures_common import unpack_state_dict  # noqa: E402
from oracle.make_golden import TINY_3D, _record_draws, derandomise_unet3d  # noqa: E402
from oracle.ref_shim import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sample_tiny_video_hd32.pt")
HEADS = dict(attn_heads=2, attn_dim_head=32, cond_dim=16)   # (cond_dim 16: the fixture stays under the 1 MiB limit of a committed file)


def main(seed=29, T=2, frames=4):
    ip, iv = load_reference("imagen_pytorch"), load_reference("imagen_video")
    torch.manual_seed(seed)
    kw1 = {**TINY_3D, **HEADS, "temporal_strides": (1, 2)}
    kw2 = {**TINY_3D, **HEADS, "temporal_strides": (2, 1), "num_resnet_blocks": (1, 2)}
    imagen = ip.Imagen((iv.Unet3D(**kw1), iv.Unet3D(**kw2)), image_sizes=(8, 16), timesteps=T, text_embed_dim=32, cond_drop_prob=0.1).eval()
    for u in imagen.unets:
        derandomise_unet3d(u)
        for prm in u.parameters():
            prm.data.copy_(prm.data.half().float())
        for buf in u.buffers():
            if buf.is_floating_point():
                buf.data.copy_(buf.data.half().float())
    text_embeds = torch.randn(2, 9, 32)
    outs, draws = _record_draws(lambda: imagen.sample(text_embeds=text_embeds, video_frames=frames, cond_scale=3., use_tqdm=False,
                                                      return_all_unet_outputs=True))
    noise, it = {}, iter(draws)
    for stage in range(2):
        if stage > 0:
            noise[("lowres", stage)] = next(it)
        noise[("init", stage)] = next(it)
        for i in range(T):
            noise[("step", stage, i)] = next(it)
    assert next(it, None) is None
    unets = []
    for i, (u, kw) in enumerate(zip(imagen.unets, (kw1, kw2))):
        sd = u.state_dict()
        assert all(v.is_floating_point() for v in sd.values())
        spec = dict(kwargs={**kw, "lowres_cond": i > 0}, flat=torch.cat([v.reshape(-1).half() for v in sd.values()]),
                    index=[(k, tuple(v.shape)) for k, v in sd.items()])
        back = unpack_state_dict(spec)
        assert list(back) == list(sd) and all(torch.equal(back[k], v) for k, v in sd.items())
        unets.append(spec)
    torch.save(dict(unets=unets, image_sizes=(8, 16), timesteps=T, frames=frames, cond_scale=3., text_embeds=text_embeds, noise=noise,
                    outputs=[o.clone() for o in outs], generator="tools/make_video_headdim32_fixture.py",
                    reference="lucidrains/imagen-pytorch v2.0.0 Imagen.sample over Unet3D stages, attn_heads = 2, attn_dim_head = 32"), OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): outputs {[tuple(o.shape) for o in outs]}, std {outs[-1].std():.4f}, {len(draws)} draws")


if __name__ == "__main__":
    main()
