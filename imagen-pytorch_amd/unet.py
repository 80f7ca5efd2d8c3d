"""Drop-in `Unet` (constructor kwargs, attributes, `state_dict` layout, `forward` / `forward_with_cond_scale`
signatures of the reference `Unet`, imagen_pytorch/imagen_pytorch.py:1112-1725 = "ip.py") whose arithmetic
runs entirely in the gfx950 kernels of libimagen_hip.so (see engine.py).  There is no PyTorch fallback:
calling `forward` on a CPU tensor, or without the HIP extension, raises.

`UnetBase` is what `Unet` and the video `Unet3D` (unet3d.py) share: the conditioning nets, the per-level configuration, the
down / mid / up construction loop, the tail, the cascade plumbing and everything of the execution path that does not depend on
the layout of the images.  Neither class derives from the other: imagen.py tells them apart with `isinstance`.
"""
from __future__ import annotations

from pathlib import Path
import sys
import torch
from torch import nn

from .modules import (CrossEmbedP, ParallelP, PerceiverResamplerP, PixelShuffleUpsampleP, ResnetBlockP, SinuPosEmbP,
                      TransformerBlockP, UpsampleCombinerP, downsample_p, upsample_conv_p)

DEFAULT_TEXT_EMBED_DIM = 768  # d_model of the reference's default T5 ('google/t5-v1_1-base', t5.py:47-58, ip.py:1117)

_printed_dim_hint = False


_ENGINE_DEVICE_TYPES = ('cuda',)   # where plans can be launched; tests/test_sample_cpu_replay.py widens it after replacing the launcher


def _cast_tuple(val, length=None):
    if isinstance(val, list):
        val = tuple(val)
    out = val if isinstance(val, tuple) else ((val,) * (length or 1))
    if length is not None:
        assert len(out) == length
    return out


def _unsupported(flag):
    raise NotImplementedError(
        f"Unet({flag}=...) is accepted by the reference but lies outside the MI355X hot-path scope of this build "
        f"(SURVEY.md §2 'optional L1 variants'); no HIP kernel plan exists for it and there is no PyTorch fallback."
    )


def check_negative_prompt(embeds, masks, batch, width, *, kw='negative_text_embeds', whose="the prompts'"):
    """The shape rules of a negative prompt, stated once for every entry point that takes one (the unets, Imagen.sample and its relatives,
    distributed.sample_sharded): (b, n, width) embeddings with b = 1 (it serves every sample) or b = `batch`, and a mask, if there is
    one, of the embeddings' (b, n).  `kw` is the keyword the caller used; `width` / `batch` None: not known here, not checked."""
    if embeds is None:
        if masks is not None:
            raise ValueError('negative_text_masks given without negative_texts / negative_text_embeds')
        return
    if embeds.ndim != 3 or (width is not None and embeds.shape[-1] != width):
        raise ValueError(f"{kw}: invalid text embedding shape {tuple(embeds.shape)} (should be (b, n, {'d' if width is None else width}))")
    if batch is not None and embeds.shape[0] not in (1, batch):
        raise ValueError(f"{kw}: batch {embeds.shape[0]} is neither 1 nor {whose} {batch}")
    if masks is not None and tuple(masks.shape) != tuple(embeds.shape[:2]):
        raise ValueError(f"negative_text_masks: shape {tuple(masks.shape)} does not match the negative prompt's {tuple(embeds.shape[:2])}")


def _guided_negative(unet, cond_scale, text_embeds, negative_texts, negative_text_embeds, negative_text_masks):
    """What forward_with_cond_scale refuses of a negative prompt before it runs anything.  `negative_texts` is part of the
    signature so that the keywords are the same at every level, but only Imagen has the `encode_text` hook that can serve it."""
    if negative_texts is not None:
        raise ValueError("negative_texts: a unet has no text encoder; pass negative_text_embeds (Imagen.sample encodes negative_texts)")
    if negative_text_embeds is None:
        return check_negative_prompt(None, negative_text_masks, None, None)
    if not unet.cond_on_text or text_embeds is None:
        raise ValueError("negative_text_embeds: this unet is not conditioned on text (cond_on_text=False, or no text_embeds given)")
    if cond_scale == 1:
        raise ValueError("negative_text_embeds: cond_scale is 1, the negative prompt would be ignored")


class UnetBase(nn.Module):
    """What `Unet` and `Unet3D` have in common.  A subclass keeps its own `__init__` signature (the reference's) and scope gates, and calls,
    in this order — modules are created in the reference's order, which fixes the `state_dict` key order and what a seeded construction
    draws: `super().__init__(locals())`, `_build_front()`, `_build_levels()`, `_build_tail(...)`.  It names the module classes of its
    layout below, and supplies a level's module list through `_down_level` / `_up_level` and the middle through `_build_mid`."""

    _CrossEmbed = _Conv = _Resnet = _Parallel = _downsample = None     # the layout's module classes / factories
    _PER_LEVEL = ('num_resnet_blocks', 'layer_attns', 'layer_attns_depth', 'layer_cross_attns')   # kwargs cast to one value per level
    _CFG_FLAGS = ('memory_efficient', 'attend_at_middle')                                         # kwargs `_layer_cfg` carries as they are
    _NO_CPU_PATH = None                                                 # the message of an engine asked for on another device type

    def __init__(self, ctor_locals: dict):
        super().__init__()
        # constructor kwargs are kept for cast_model_parameters / persistence (ip.py:1173-1175; iv.py:1291-1293)
        self._locals = {k: v for k, v in ctor_locals.items() if k not in ('self', '__class__')}
        assert self._locals['attn_heads'] > 1, 'you need to have more than 1 attention head, ideally at least 4 or 8'

    # ---- construction ----------------------------------------------------------------------------------

    def _build_front(self):
        """Everything ahead of the levels: the init conv, the conditioning nets, `_layer_cfg` and the init resnet block."""
        kw = self._locals
        dim, channels, lowres_cond, self_cond = kw['dim'], kw['channels'], kw['lowres_cond'], kw['self_cond']
        self.channels = channels
        self.channels_out = kw['channels_out'] if kw['channels_out'] is not None else channels
        init_channels = channels * (1 + int(lowres_cond) + int(self_cond))          # ip.py:1186; iv.py:1302
        init_dim = kw['init_dim'] if kw['init_dim'] is not None else dim
        self.self_cond = self_cond
        self.has_cond_image = kw['cond_images_channels'] > 0          # ip.py:1191-1194; iv.py:1307-1310: extra input channels of the init conv
        self.cond_images_channels = kw['cond_images_channels']
        init_channels += self.cond_images_channels

        # initial convolution (ip.py:1198)
        k = kw['init_conv_kernel_size']
        self.init_conv = (self._CrossEmbed(init_channels, kernel_sizes=kw['init_cross_embed_kernel_sizes'], dim_out=init_dim, stride=1)
                          if kw['init_cross_embed'] else self._Conv(init_channels, init_dim, k, padding=k // 2))

        dims = [init_dim, *[dim * m for m in kw['dim_mults']]]
        in_out = list(zip(dims[:-1], dims[1:]))
        self.cond_dim = kw['cond_dim'] if kw['cond_dim'] is not None else dim
        self.time_cond_dim = dim * 4 * (2 if lowres_cond else 1)
        self._build_cond_nets()

        n = len(in_out)
        self._layer_cfg = dict(in_out=in_out, init_dim=init_dim, dim=dim, **{k: _cast_tuple(kw[k], n) for k in self._PER_LEVEL},
                               **{k: kw[k] for k in self._CFG_FLAGS})
        self.init_resnet_block = (self._Resnet(init_dim, init_dim, time_cond_dim=self.time_cond_dim, use_gca=kw['use_global_context_attn'],
                                               **self._attn_kwargs) if kw['memory_efficient'] else None)
        self.skip_connect_scale = 1. if not kw['scale_skip_connection'] else (2 ** -0.5)

    def _build_cond_nets(self):
        """The time / noise-level embedding (ip.py:1210-1248; iv.py:1326-1369) and the text conditioning (ip.py:1254-1287)."""
        kw, cond_dim, time_cond_dim = self._locals, self.cond_dim, self.time_cond_dim
        sinu_dim, num_time_tokens, cond_on_text = kw['learned_sinu_pos_emb_dim'], kw['num_time_tokens'], kw['cond_on_text']

        def time_nets():
            hiddens = nn.Sequential(SinuPosEmbP(sinu_dim), nn.Linear(sinu_dim + 1, time_cond_dim), nn.SiLU())
            cond = nn.Sequential(nn.Linear(time_cond_dim, time_cond_dim))
            tokens = nn.Sequential(nn.Linear(time_cond_dim, cond_dim * num_time_tokens), nn.Identity())
            return hiddens, cond, tokens

        self.to_time_hiddens, self.to_time_cond, self.to_time_tokens = time_nets()
        self.num_time_tokens = num_time_tokens
        self.lowres_cond = kw['lowres_cond']
        if self.lowres_cond:
            self.to_lowres_time_hiddens, self.to_lowres_time_cond, self.to_lowres_time_tokens = time_nets()

        self.norm_cond = nn.LayerNorm(cond_dim)

        self.text_to_cond = None
        if cond_on_text:
            assert kw['text_embed_dim'] is not None, 'text_embed_dim must be given to the unet if cond_on_text is True'
            self.text_to_cond = nn.Linear(kw['text_embed_dim'], cond_dim)
        self.cond_on_text = cond_on_text
        self.attn_pool = (PerceiverResamplerP(dim=cond_dim, depth=2, num_latents=kw['attn_pool_num_latents'], **self._attn_kwargs)
                          if kw['attn_pool_text'] else None)
        self.max_text_len = kw['max_text_len']
        self.null_text_embed = nn.Parameter(torch.randn(1, self.max_text_len, cond_dim))
        self.null_text_hidden = nn.Parameter(torch.randn(1, time_cond_dim))
        self.to_text_non_attn_cond = None
        if cond_on_text:
            self.to_text_non_attn_cond = nn.Sequential(nn.LayerNorm(cond_dim), nn.Linear(cond_dim, time_cond_dim), nn.SiLU(),
                                                       nn.Linear(time_cond_dim, time_cond_dim))

    @property
    def _attn_kwargs(self) -> dict:
        return dict(heads=self._locals['attn_heads'], dim_head=self._locals['attn_dim_head'])

    def _level(self, ind: int) -> dict:
        """The per-level configuration of level `ind` (of the down path; the up path walks the levels backwards)."""
        return {k: self._layer_cfg[k][ind] for k in self._PER_LEVEL}

    def _level_blocks(self, lvl: dict, dim_in: int, dim_out: int, conditioned: bool, **first) -> list:
        """A level's first, conditioned, ResnetBlock and the list of its plain ones (ip.py:1370-1371, 1409-1410; iv.py:1471-1472, 1513-1514)."""
        tcd = self.time_cond_dim
        return [self._Resnet(dim_in, dim_out, cond_dim=self.cond_dim if conditioned else None, time_cond_dim=tcd, **first, **self._attn_kwargs),
                nn.ModuleList([self._Resnet(dim_in, dim_out, time_cond_dim=tcd, use_gca=self._locals['use_global_context_attn'])
                               for _ in range(lvl['num_resnet_blocks'])])]

    def _build_levels(self):
        """`downs`, the middle and `ups` (ip.py:1338-1413; iv.py:1449-1519): where the levels downsample (in front of a level under
        `memory_efficient`, behind it otherwise, the last level then keeping its size) and what each up level concatenates."""
        in_out, mem_eff = self._layer_cfg['in_out'], self._layer_cfg['memory_efficient']
        n = len(in_out)
        self.downs = nn.ModuleList([])
        self.ups = nn.ModuleList([])
        skip_connect_dims = []
        for ind, (dim_in, dim_out) in enumerate(in_out):
            is_last = ind >= (n - 1)
            pre = self._downsample(dim_in, dim_out) if mem_eff else None
            current_dim = dim_out if mem_eff else dim_in
            skip_connect_dims.append(current_dim)
            post = None
            if not mem_eff:
                post = self._downsample(current_dim, dim_out) if not is_last else self._Parallel(dim_in, dim_out)
            self.downs.append(nn.ModuleList(self._down_level(self._level(ind), current_dim, pre, post)))
        self._build_mid(in_out[-1][1])
        for ind, (dim_in, dim_out) in enumerate(reversed(in_out)):
            is_last = ind == (n - 1)
            self.ups.append(nn.ModuleList(self._up_level(self._level(n - 1 - ind), dim_out + skip_connect_dims.pop(), dim_out,
                                                         dim_in if (not is_last or mem_eff) else None)))

    def _down_level(self, lvl: dict, dim: int, pre, post) -> list:
        """The modules of a down level at `dim` channels, `pre` / `post` (its downsample, or None) included."""
        raise NotImplementedError

    def _build_mid(self, dim: int):
        raise NotImplementedError

    def _up_level(self, lvl: dict, dim_cat: int, dim_out: int, upsample_to) -> list:
        """The modules of an up level whose blocks read `dim_cat` channels (x and the skip connection) and write `dim_out`; it upsamples
        to `upsample_to` channels unless that is None."""
        raise NotImplementedError

    def _build_tail(self, final_conv_dim: int):
        """The final resnet block over `final_conv_dim` channels, the zero-initialised final conv and the engine cache."""
        kw = self._locals
        dim, k = kw['dim'], kw['final_conv_kernel_size']
        self.final_res_block = (self._Resnet(final_conv_dim, dim, time_cond_dim=self.time_cond_dim, use_gca=True)
                                if kw['final_resnet_block'] else None)
        final_conv_dim_in = (dim if kw['final_resnet_block'] else final_conv_dim) + (self.channels if self.lowres_cond else 0)
        self.final_conv = self._Conv(final_conv_dim_in, self.channels_out, k, padding=k // 2)
        nn.init.zeros_(self.final_conv.weight)   # ip.py:1438; iv.py:1578 — parity tests must de-zero this
        nn.init.zeros_(self.final_conv.bias)

        self.resize_mode = kw['resize_mode']
        self._engines = {}

    # ---- cascade plumbing (ip.py:1446-1506; iv.py:1586-1634) -----------------------------------------

    def cast_model_parameters(self, *, lowres_cond, text_embed_dim, channels, channels_out, cond_on_text):
        if (lowres_cond == self.lowres_cond and channels == self.channels and cond_on_text == self.cond_on_text
                and text_embed_dim == self._locals['text_embed_dim'] and channels_out == self.channels_out):
            return self
        updated = dict(lowres_cond=lowres_cond, text_embed_dim=text_embed_dim, channels=channels, channels_out=channels_out,
                       cond_on_text=cond_on_text)
        return self.__class__(**{**self._locals, **updated})

    def to_config_and_state_dict(self):
        return self._locals, self.state_dict()

    @classmethod
    def from_config_and_state_dict(klass, config, state_dict):
        unet = klass(**config)
        unet.load_state_dict(state_dict)
        return unet

    def persist_to_file(self, path):
        path = Path(path)
        path.parents[0].mkdir(exist_ok=True, parents=True)
        config, state_dict = self.to_config_and_state_dict()
        torch.save(dict(config=config, state_dict=state_dict), str(path))

    @classmethod
    def hydrate_from_file(klass, path, trust_checkpoint: bool = False):
        path = Path(path)
        assert path.exists()
        from .checkpoint import _load_checkpoint_file
        pkg = _load_checkpoint_file(path, trust_checkpoint)
        assert 'config' in pkg and 'state_dict' in pkg
        return klass.from_config_and_state_dict(pkg['config'], pkg['state_dict'])

    # ---- execution -------------------------------------------------------------------------------------

    def _cached_engine(self, key: tuple, device: torch.device, make):
        """The engine cached under `key`, built by `make()` if there is none or the parameters changed under it."""
        if device.type not in _ENGINE_DEVICE_TYPES:       # (read at call time: the CPU replay tests widen it)
            raise RuntimeError(self._NO_CPU_PATH)
        eng = self._engines.get(key)
        if eng is None or eng.stale():
            eng = self._engines[key] = make()
        return eng

    def release_engines(self):
        self._engines.clear()

    @staticmethod
    def _keep_mask(B: int, cfg: bool, cond_drop_prob: float) -> torch.Tensor:
        """bool [rows], True = conditional row: B conditional + B null rows under guidance, else what prob_mask_like draws (ip.py:201-207) —
        from the caller's generator in the fractional case only."""
        if cfg:
            return torch.cat((torch.ones(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)))
        if cond_drop_prob == 0:
            return torch.ones(B, dtype=torch.bool)
        if cond_drop_prob == 1:
            return torch.zeros(B, dtype=torch.bool)
        return torch.rand(B) < (1 - cond_drop_prob)

    def forward_with_cond_scale(self, *args, cond_scale=1., negative_text_embeds=None, negative_text_masks=None, negative_texts=None, **kwargs):
        """ip.py:1510-1522; iv.py:1636-1648 — the cond and null branches run as ONE 2B-row batch through the kernel plan.

        Extension: negative_text_embeds (+ negative_text_masks, default any(embeds != 0, -1)) puts a second prompt on the null branch — the
        result is neg + (pos - neg) * cond_scale with both branches evaluated at cond_drop_prob = 0.  A batch-1 negative prompt serves the
        whole batch.  (`negative_texts` needs an encoder: Imagen.sample takes it; a bare unet has none.)

        Prompt and negative prompt share one token axis, the longer one's.  One consequence for a call WITHOUT `text_mask` whose prompt is
        the shorter of the two: the positions it is padded by are masked, so they become null_text_embed, where the same call without a
        negative prompt leaves zero tokens from the prompt's end to max_text_len.  It is the result of passing text_mask = all ones over
        the prompt's own tokens; pass a `text_mask` (Imagen.sample always derives one) and the conditional branch does not depend on
        the negative prompt at all."""
        _guided_negative(self, cond_scale, kwargs.get('text_embeds'), negative_texts, negative_text_embeds, negative_text_masks)
        if cond_scale == 1:
            return self.forward(*args, **kwargs)
        kwargs.pop('cond_drop_prob', None)
        both = self._run(*args, cfg=True, negative_text_embeds=negative_text_embeds, negative_text_mask=negative_text_masks, **kwargs)
        b = both.shape[0] // 2
        logits, null_logits = both[:b], both[b:]
        return null_logits + (logits - null_logits) * cond_scale


class Unet(UnetBase):
    _CrossEmbed, _Conv, _Resnet, _Parallel, _downsample = CrossEmbedP, nn.Conv2d, ResnetBlockP, ParallelP, staticmethod(downsample_p)
    _PER_LEVEL = UnetBase._PER_LEVEL + ('use_linear_cross_attn',)
    _CFG_FLAGS = UnetBase._CFG_FLAGS + ('layer_mid_attns_depth',)
    _NO_CPU_PATH = "imagen_pytorch_amd.Unet runs on MI355X through libimagen_hip.so only; there is no CPU path"

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
        cond_images_channels=0,
        channels=3,
        channels_out=None,
        attn_dim_head=64,
        attn_heads=8,
        ff_mult=2.,
        lowres_cond=False,
        layer_attns=True,
        layer_attns_depth=1,
        layer_mid_attns_depth=1,
        layer_attns_add_text_cond=True,
        attend_at_middle=True,
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
        resize_mode='nearest',
        combine_upsample_fmaps=False,
        pixel_shuffle_upsample=True,
    ):
        super().__init__(locals())
        global _printed_dim_hint
        if dim < 128 and not _printed_dim_hint:
            _printed_dim_hint = True
            print('The base dimension of your u-net should ideally be no smaller than 128 (reference hint, ip.py:1168)', file=sys.stderr)

        # ---- scope gate: flags with no kernel plan fail loudly at construction
        if any(_cast_tuple(use_linear_attn)):
            _unsupported('use_linear_attn')
        if cross_embed_downsample:
            # the reference cannot build this either: partial(CrossEmbedLayer, kernel_sizes=...) is called with (dim_in, dim_out)
            # positionally (ip.py:1315, 1357, 1366), so dim_out collides with kernel_sizes and Unet(...) raises TypeError — no
            # checkpoint with this flag exists
            _unsupported('cross_embed_downsample')
        if attn_dim_head not in (32, 64, 128):
            raise NotImplementedError(f"attn_dim_head = {attn_dim_head}: the attention kernels are built for head dims 64 (every README config), "
                                      "32 (the reference's UnetConfig default, configs.py:48-49) and 128 (wide heads)")

        self._build_front()
        self._layer_cfg['use_linear_cross_attn'] = tuple(bool(v) for v in self._layer_cfg['use_linear_cross_attn'])   # ip.py:1306
        self._build_levels()

        # whether to combine the feature maps of all up levels before the final resnet block (ip.py:1415-1422)
        self.upsample_combiner = UpsampleCombinerP(dim, enabled=combine_upsample_fmaps, dim_outs=dim,
                                                   dim_ins=[dim_out for _, dim_out in reversed(self._layer_cfg['in_out'])])
        self.init_conv_to_final_conv_residual = init_conv_to_final_conv_residual          # ip.py:1426-1427
        if init_conv_to_final_conv_residual:
            assert self._layer_cfg['init_dim'] == dim, \
                'init_conv_to_final_conv_residual needs init_dim == dim (the reference concatenates `dim` channels)'
        self._build_tail(self.upsample_combiner.dim_out + (dim if init_conv_to_final_conv_residual else 0))

    def _level_modules(self, lvl: dict, dim_in: int, dim_out: int) -> list:
        """[first block, blocks, transformer]; ip.py:1341, 1395: the linear flag conditions the level's first block even where
        layer_cross_attns is False."""
        kw, linear = self._locals, lvl['use_linear_cross_attn']
        return [*self._level_blocks(lvl, dim_in, dim_out, bool(lvl['layer_cross_attns'] or linear), linear_attn=linear),
                (TransformerBlockP(dim=dim_out, depth=lvl['layer_attns_depth'], ff_mult=kw['ff_mult'], context_dim=self.cond_dim, **self._attn_kwargs)
                 if lvl['layer_attns'] else nn.Identity())]

    def _down_level(self, lvl, dim, pre, post):
        return [pre, *self._level_modules(lvl, dim, dim), post]

    def _build_mid(self, dim):
        """ip.py:1378-1382 — NB: the mid ResnetBlocks are built without the attention kwargs, i.e. always 8 heads x 64."""
        kw, tcd = self._locals, self.time_cond_dim
        self.mid_block1 = ResnetBlockP(dim, dim, cond_dim=self.cond_dim, time_cond_dim=tcd)
        self.mid_attn = TransformerBlockP(dim, depth=kw['layer_mid_attns_depth'], **self._attn_kwargs) if kw['attend_at_middle'] else None
        self.mid_block2 = ResnetBlockP(dim, dim, cond_dim=self.cond_dim, time_cond_dim=tcd)

    def _up_level(self, lvl, dim_cat, dim_out, upsample_to):
        upsample = PixelShuffleUpsampleP if self._locals['pixel_shuffle_upsample'] else upsample_conv_p
        return [*self._level_modules(lvl, dim_cat, dim_out), upsample(dim_out, upsample_to) if upsample_to is not None else nn.Identity()]

    # ---- execution -------------------------------------------------------------------------------------

    @property
    def size_divisor(self) -> int:
        """What both sides of an image must be a multiple of: one halving per level but the last (ip.py:1359-1366), and one in front of
        EVERY level under `memory_efficient` (ip.py:1353-1355: the last level then downsamples too, and its up level upsamples back)."""
        n = len(self._layer_cfg["in_out"])
        return 2 ** (n if self._layer_cfg["memory_efficient"] else n - 1)

    def check_image_size(self, H: int, W: int, what: str = "image"):
        """ValueError for an H x W the down path does not divide: a level's pixel-unshuffle would drop the odd row / column and the
        skip connections of the up path would no longer meet maps of their own size."""
        d = self.size_divisor
        if H <= 0 or W <= 0 or H % d or W % d:
            raise ValueError(f"{what} of {H} x {W}: both sides must be positive multiples of {d} (what the downsamples of this unet divide by)")

    def engine(self, batch_rows: int, src_batch: int, image_size, device, with_text: bool = True) -> "UnetEngine":  # noqa: F821
        """Compiled kernel plan for `batch_rows` denoiser rows (= src_batch, 2*src_batch with CFG, or (K + 1)*src_batch for K composed prompt sets) at image_size^2, or at H x W for
        image_size = (H, W); (S, S) is the engine of S."""
        from .engine import UnetEngine

        if not isinstance(image_size, int):
            H, W = (int(v) for v in image_size)
            image_size = H if H == W else (H, W)

        device = torch.device(device)
        return self._cached_engine((batch_rows, src_batch, image_size, device.index or 0, bool(with_text)), device,
                                   lambda: UnetEngine(self, batch_rows, src_batch, image_size, device, with_text=with_text))

    def forward(self, x, time, *, lowres_cond_img=None, lowres_noise_times=None, text_embeds=None, text_mask=None,
                cond_images=None, self_cond=None, cond_drop_prob=0.):
        """ip.py:1524-1725.  `time` / `lowres_noise_times` are log-SNR conditions.  Returns fp32 NCHW."""
        return self._run(x, time, lowres_cond_img=lowres_cond_img, lowres_noise_times=lowres_noise_times, text_embeds=text_embeds,
                         text_mask=text_mask, cond_images=cond_images, self_cond=self_cond, cond_drop_prob=cond_drop_prob, cfg=False)

    @torch.no_grad()
    def _run(self, x, time, *, lowres_cond_img=None, lowres_noise_times=None, text_embeds=None, text_mask=None, cond_images=None,
             cond_drop_prob=0., cfg=False, self_cond=None, negative_text_embeds=None, negative_text_mask=None):
        assert not (self.lowres_cond and lowres_cond_img is None), 'low resolution conditioning image must be present'
        assert not (self.lowres_cond and lowres_noise_times is None), 'low resolution conditioning noise time must be present'
        assert not (self.has_cond_image ^ (cond_images is not None)), \
            'you either requested to condition on an image on the unet, but the conditioning image is not supplied, or vice versa'
        if self.training:
            raise RuntimeError("the MI355X path implements sampling (eval mode) only; call .eval() first")
        B, _, H, W = x.shape
        self.check_image_size(H, W)
        check_negative_prompt(negative_text_embeds, negative_text_mask, B,       # before an engine is built or anything is launched
                              None if text_embeds is None else text_embeds.shape[-1])
        rows = 2 * B if cfg else B
        with_text = bool(self.cond_on_text and text_embeds is not None)
        eng = self.engine(rows, B, (H, W), x.device, with_text=with_text)
        eng.set_conditioning(text_embeds=text_embeds if with_text else None, text_mask=text_mask, keep=self._keep_mask(B, cfg, cond_drop_prob),
                             lowres_noise_times=lowres_noise_times, negative_text_embeds=negative_text_embeds,
                             negative_text_mask=negative_text_mask)
        if cond_images is not None:
            eng.set_cond_images(cond_images)
        if self.self_cond:
            eng.set_self_cond(self_cond)             # None: zeros (ip.py:1542); a unet built without self_cond ignores the argument, as the reference does
        out = eng.forward(x.float().contiguous(), time.float().contiguous(),
                          lowres_cond_img=None if lowres_cond_img is None else lowres_cond_img.float().contiguous())
        return out.clone()


class NullUnet(nn.Module):
    """ip.py:1729-1739."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.lowres_cond = False
        self.dummy_parameter = nn.Parameter(torch.tensor([0.]))

    def cast_model_parameters(self, *args, **kwargs):
        return self

    def forward(self, x, *args, **kwargs):
        return x


class BaseUnet64(Unet):
    """ip.py:1743-1755."""

    def __init__(self, *args, **kwargs):
        defaults = dict(dim=512, dim_mults=(1, 2, 3, 4), num_resnet_blocks=3, layer_attns=(False, True, True, True),
                        layer_cross_attns=(False, True, True, True), attn_heads=8, ff_mult=2., memory_efficient=False)
        super().__init__(*args, **{**defaults, **kwargs})


class SRUnet256(Unet):
    """ip.py:1757-1769."""

    def __init__(self, *args, **kwargs):
        defaults = dict(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=(2, 4, 8, 8), layer_attns=(False, False, False, True),
                        layer_cross_attns=(False, False, False, True), attn_heads=8, ff_mult=2., memory_efficient=True)
        super().__init__(*args, **{**defaults, **kwargs})


class SRUnet1024(Unet):
    """ip.py:1771-1783."""

    def __init__(self, *args, **kwargs):
        defaults = dict(dim=128, dim_mults=(1, 2, 4, 8), num_resnet_blocks=(2, 4, 8, 8), layer_attns=False,
                        layer_cross_attns=(False, False, False, True), attn_heads=8, ff_mult=2., memory_efficient=True)
        super().__init__(*args, **{**defaults, **kwargs})
