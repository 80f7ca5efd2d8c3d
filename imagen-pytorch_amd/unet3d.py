"""Drop-in `Unet3D` (Imagen-Video denoiser): constructor kwargs, attributes and `state_dict` layout of the reference
`Unet3D` (imagen_pytorch/imagen_video.py:1225-1941 = "iv.py"), SURVEY.md §8(f) NEXT-2.

STATUS: the parameter surface (this file, modules3d.py) is checked on CPU against the live reference's state_dict; the kernel
plan is built by engine3d.py and checked on CPU through the plan interpreter against oracle/unet3d_oracle.py; the two kernels the
video path adds (csrc/temporal.hip), `forward` and both video samplers run on MI355X in tests/test_video_gpu.py (measurements:
profiles/r0*_c5*) — see DESIGN.md §8 NEXT-2.
As for `Unet`, there is no PyTorch fallback: `forward` needs libimagen_hip.so and a CUDA/HIP tensor.

What it shares with `Unet` lives in unet.UnetBase; here are the reference's signature, the scope gates, the video levels (8 modules
down, 7 up: a temporal PEG, a temporal attention and the temporal resampling behind each level's transformer) and the frame-major `_run`.
"""
from __future__ import annotations

import functools
import operator

import torch
from torch import nn

from .modules import Holder
from .modules3d import (Attention3dP, CrossEmbed3dP, Parallel3dP, PixelShuffleUpsample3dP, ResidualP, ResnetBlock3dP,
                        TemporalPixelShuffleUpsampleP, TransformerBlock3dP, conv_frames_p, downsample3d_p, temporal_attn_p,
                        temporal_downsample_p, temporal_peg_p)
from .unet import DEFAULT_TEXT_EMBED_DIM, UnetBase, _cast_tuple, _unsupported, check_negative_prompt


class Unet3D(UnetBase):
    _CrossEmbed, _Conv, _Resnet, _Parallel = CrossEmbed3dP, staticmethod(conv_frames_p), ResnetBlock3dP, Parallel3dP
    _downsample = staticmethod(downsample3d_p)
    _PER_LEVEL = UnetBase._PER_LEVEL + ('temporal_strides',)
    _NO_CPU_PATH = "imagen_pytorch_amd.Unet3D runs on MI355X through libimagen_hip.so only; there is no CPU path"

    def __init__(
        self,
        *,
        dim,
        text_embed_dim=DEFAULT_TEXT_EMBED_DIM,
        num_resnet_blocks=1,
        cond_dim=None,
        num_image_tokens=4,
        num_time_tokens=2,
        learned_sinu_pos_emb_dim=16,
        out_dim=None,
        dim_mults=(1, 2, 4, 8),
        temporal_strides=1,
        cond_images_channels=0,
        channels=3,
        channels_out=None,
        attn_dim_head=64,
        attn_heads=8,
        ff_mult=2.,
        ff_time_token_shift=True,
        lowres_cond=False,
        layer_attns=False,
        layer_attns_depth=1,
        layer_attns_add_text_cond=True,
        attend_at_middle=True,
        time_rel_pos_bias_depth=2,
        time_causal_attn=True,
        layer_cross_attns=True,
        use_linear_attn=False,
        use_linear_cross_attn=False,
        cond_on_text=True,
        max_text_len=256,
        init_dim=None,
        init_conv_kernel_size=7,
        init_cross_embed=True,
        init_cross_embed_kernel_sizes=(3, 7, 15),
        cross_embed_downsample=False,
        cross_embed_downsample_kernel_sizes=(2, 4),
        attn_pool_text=True,
        attn_pool_num_latents=32,
        dropout=0.,
        memory_efficient=False,
        init_conv_to_final_conv_residual=False,
        use_global_context_attn=True,
        scale_skip_connection=True,
        final_resnet_block=True,
        final_conv_kernel_size=3,
        self_cond=False,
        combine_upsample_fmaps=False,
        pixel_shuffle_upsample=True,
        resize_mode='nearest',
    ):
        super().__init__(locals())

        for name in ('use_linear_attn', 'use_linear_cross_attn'):
            if any(_cast_tuple(self._locals[name])):
                _unsupported(name)
        for name in ('cross_embed_downsample', 'combine_upsample_fmaps', 'init_conv_to_final_conv_residual'):
            if self._locals[name]:
                _unsupported(name)
        if not pixel_shuffle_upsample:
            _unsupported('pixel_shuffle_upsample=False')
        if self_cond and cond_images_channels:
            _unsupported('self_cond together with cond_images_channels')
        if attn_dim_head not in (32, 64):
            raise NotImplementedError(f"attn_dim_head = {attn_dim_head}: the attention kernels (temporal attention included) are built for head dims 64 "
                                      "(every README config) and 32 (the reference's Unet3DConfig default, configs.py:61-62)")

        self.time_causal_attn, self.ff_time_token_shift = time_causal_attn, ff_time_token_shift
        self._build_front()
        self.total_temporal_divisor = functools.reduce(operator.mul, self._layer_cfg['temporal_strides'], 1)
        self.init_temporal_peg = temporal_peg_p(self._layer_cfg['init_dim'])                  # iv.py:1413-1416
        self.init_temporal_attn = self._temporal_attn(self._layer_cfg['init_dim'])
        self._build_levels()
        self.upsample_combiner = Holder()
        self.init_conv_to_final_conv_residual = False
        self._build_tail(dim)

    def _temporal_attn(self, dim):
        kw = self._locals
        return temporal_attn_p(dim, kw['attn_heads'], kw['attn_dim_head'], kw['time_causal_attn'], kw['time_rel_pos_bias_depth'])

    def _level_modules(self, lvl: dict, dim_in: int, dim_out: int) -> list:
        """[first block, blocks, transformer, temporal PEG, temporal attention] (iv.py:1471-1475, 1513-1517)."""
        kw = self._locals
        return [*self._level_blocks(lvl, dim_in, dim_out, bool(lvl['layer_cross_attns'])),
                (TransformerBlock3dP(dim=dim_out, depth=lvl['layer_attns_depth'], ff_mult=kw['ff_mult'], ff_time_token_shift=kw['ff_time_token_shift'],
                                     context_dim=self.cond_dim, **self._attn_kwargs) if lvl['layer_attns'] else nn.Identity()),
                temporal_peg_p(dim_out),
                self._temporal_attn(dim_out)]

    def _down_level(self, lvl, dim, pre, post):
        t_stride = lvl['temporal_strides']
        return [pre, *self._level_modules(lvl, dim, dim), temporal_downsample_p(dim, stride=t_stride) if t_stride > 1 else None, post]

    def _build_mid(self, dim):                                          # iv.py:1481-1487
        tcd = self.time_cond_dim
        self.mid_block1 = ResnetBlock3dP(dim, dim, cond_dim=self.cond_dim, time_cond_dim=tcd)
        self.mid_attn = ResidualP(Attention3dP(dim, **self._attn_kwargs)) if self._locals['attend_at_middle'] else None
        self.mid_temporal_peg = temporal_peg_p(dim)
        self.mid_temporal_attn = self._temporal_attn(dim)
        self.mid_block2 = ResnetBlock3dP(dim, dim, cond_dim=self.cond_dim, time_cond_dim=tcd)

    def _up_level(self, lvl, dim_cat, dim_out, upsample_to):
        t_stride = lvl['temporal_strides']
        return [*self._level_modules(lvl, dim_cat, dim_out),
                TemporalPixelShuffleUpsampleP(dim_out, stride=t_stride) if t_stride > 1 else None,
                PixelShuffleUpsample3dP(dim_out, upsample_to) if upsample_to is not None else nn.Identity()]

    # ---- execution ------------------------------------------------------------------------------------
    def engine(self, batch_rows: int, src_batch: int, frames: int, image_size: int, device, with_text: bool = True, ignore_time: bool = False,
               pre_frames: int = 0, post_frames: int = 0):
        from .engine3d import UnetEngine3D

        device = torch.device(device)
        key = (batch_rows, src_batch, frames, image_size, device.index or 0, bool(with_text), bool(ignore_time), pre_frames, post_frames)
        return self._cached_engine(key, device, lambda: UnetEngine3D(self, batch_rows, src_batch, frames, image_size, device, with_text=with_text,
                                                                     ignore_time=ignore_time, pre_frames=pre_frames, post_frames=post_frames))

    def forward(self, x, time, *, lowres_cond_img=None, lowres_noise_times=None, text_embeds=None, text_mask=None, cond_images=None,
                cond_video_frames=None, post_cond_video_frames=None, self_cond=None, cond_drop_prob=0., ignore_time=False):
        """iv.py:1650-1941.  x: (b, c, f, h, w); returns fp32 (b, c_out, f, h, w)."""
        return self._run(x, time, lowres_cond_img=lowres_cond_img, lowres_noise_times=lowres_noise_times, text_embeds=text_embeds,
                         text_mask=text_mask, cond_drop_prob=cond_drop_prob, ignore_time=ignore_time, cfg=False, cond_images=cond_images,
                         cond_video_frames=cond_video_frames, post_cond_video_frames=post_cond_video_frames, self_cond=self_cond)

    @torch.no_grad()
    def _run(self, x, time, *, lowres_cond_img=None, lowres_noise_times=None, text_embeds=None, text_mask=None, cond_drop_prob=0.,
             ignore_time=False, cfg=False, cond_images=None, cond_video_frames=None, post_cond_video_frames=None, self_cond=None,
             negative_text_embeds=None, negative_text_mask=None):
        assert not (self.has_cond_image ^ (cond_images is not None)), \
            'you either requested to condition on an image on the unet, but the conditioning image is not supplied, or vice versa'   # iv.py:1722
        if cond_images is not None:
            assert cond_images.ndim == 4, 'conditioning images must have 4 dimensions only, if you want to condition on frames of video, ' \
                                          'use `cond_video_frames` instead'                                                   # iv.py:1725
        assert x.ndim == 5, 'input to 3d unet must have 5 dimensions (batch, channels, time, height, width)'
        assert not (self.lowres_cond and lowres_cond_img is None), 'low resolution conditioning image must be present'
        assert not (self.lowres_cond and lowres_noise_times is None), 'low resolution conditioning noise time must be present'
        if self.training:
            raise RuntimeError("the MI355X path implements sampling (eval mode) only; call .eval() first")
        B, _, Fr, H, W = x.shape
        assert H == W, 'square frames only'
        check_negative_prompt(negative_text_embeds, negative_text_mask, B,       # before an engine is built or anything is launched
                              None if text_embeds is None else text_embeds.shape[-1])
        assert ignore_time or Fr % self.total_temporal_divisor == 0, \
            f'number of input frames {Fr} must be divisible by {self.total_temporal_divisor}'
        rows = 2 * B if cfg else B
        with_text = bool(self.cond_on_text and text_embeds is not None)
        n_pre = 0 if cond_video_frames is None else cond_video_frames.shape[2]
        n_post = 0 if post_cond_video_frames is None else post_cond_video_frames.shape[2]
        eng = self.engine(rows, B, Fr, H, x.device, with_text=with_text, ignore_time=ignore_time, pre_frames=n_pre, post_frames=n_post)
        if n_pre or n_post:
            eng.set_cond_video_frames(cond_video_frames, post_cond_video_frames)
        if cond_images is not None:
            eng.set_cond_images(cond_images)
        if self.self_cond:                           # None: zeros (iv.py:1674-1676); a unet built without self_cond ignores the argument
            eng.set_self_cond(None if self_cond is None else self_cond.float().permute(0, 2, 1, 3, 4))
        eng.set_conditioning(text_embeds=text_embeds if with_text else None, text_mask=text_mask, keep=self._keep_mask(B, cfg, cond_drop_prob),
                             lowres_noise_times=lowres_noise_times, negative_text_embeds=negative_text_embeds,
                             negative_text_mask=negative_text_mask)
        # the engine's image layout is frame-major (b, f, c, h, w): frames of one clip are consecutive NHWC images
        to_fm = lambda t: t.float().permute(0, 2, 1, 3, 4).contiguous()
        out = eng.forward(to_fm(x), time.float().contiguous(), lowres_cond_img=None if lowres_cond_img is None else to_fm(lowres_cond_img))
        return out.permute(0, 2, 1, 3, 4).contiguous()
