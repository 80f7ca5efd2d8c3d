"""UnetEngine3D — kernel planner of the drop-in `Unet3D` (Imagen-Video denoiser, imagen_pytorch/imagen_video.py:1650-1941 = iv.py).

The two kernels it needs beyond the image path live in csrc/temporal.hip.  Checked on CPU against oracle/unet3d_oracle.py through
tests/plan_interp.py and on MI355X by tests/test_video_gpu.py (DESIGN.md §8 NEXT-2).

Layout: a clip is fp16 [R, F, H, W, C] — F consecutive NHWC frames per row — so the same memory serves three views:
  frames  Act(R*F, H, W, C)     per-frame ops of the image path (3x3 conv, down / up-sampling, CrossEmbed) with batch R*F
  clip    Act(R, F*H, W, C)     per-clip ops: GlobalContext, cross attention and space-time attention over all F*H*W tokens,
                                1x1 convolutions whose gate / affine is per clip
  time    Act(R, F, H*W, C)     ops along the frame axis: "image" rows = frames, columns = pixels

The pseudo-3D convolution (iv.py:397-451) = the image path's fused ChanRMSNorm -> SiLU -> 3x3 conv per frame, followed by the causal
temporal conv1d (k = 3).  The temporal conv is three accumulating 1x1 GEMMs over frame-shifted views of the time layout
(y[f] = W2 x[f] + b;  y[1:] += W1 x[:-1];  y[2:] += W0 x[:-2]): only IGEMM features the image path already uses.  That costs three
launches and ~2x the minimal traffic per temporal conv; a dedicated (3 x 1)-tap staging path is the obvious next optimisation.
Everything input-independent is prepared at plan build: the relative position bias table of every temporal attention
(DynamicPositionBias MLP on the 2F-1 frame distances, iv.py:1182-1223) and the depthwise PEG taps.

Prompt frames (`cond_video_frames` / `post_cond_video_frames`, iv.py:1682-1718, 1933-1939): the network then runs on
F = len(post) + len(pre) + Fx frames per clip — the reference concatenates BOTH prompts in front of the Fx frames being denoised —
while the sampler state `x_in` / `out` keep Fx frames.  The prompt slots of the packed input clip are static (written once by
set_cond_video_frames); per step the Fx packed frames are copied behind them and the final conv's F output frames are cut back to
frames [len(pre), len(pre) + Fx) — two strided row copies around the unchanged plan.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as TF

from . import ops
from .engine import SIM_SCALE, UnetEngine, _pad_vec, _w2d
from .modules3d import TransformerBlock3dP
from .ops import ACT_SILU, OUT_NCHW_F32, Act


def _wb2d(mod):
    """_w2d as the (weight, bias) pair the image planner's init / final conv weight builders take."""
    cw = _w2d(mod)
    return cw.weight, cw.bias


# Split-precision weights (engine.py, SPLIT_*) on the video path's OUTPUT stage: `final_conv` and block1 of `final_res_block` — the two convs
# whose weight rounding reaches the output unattenuated (plan interpreter, BASELINE C5: cond 1.008e-3 -> 0.970e-3, null 0.921e-3 -> 0.901e-3;
# block1 of the two outer down levels on top of them buys nothing).  A video clip puts R * F frames through every conv, so the image path's
# executed-FLOP bound (SPLIT_SMALL_FLOPS) never admits them: the output stage gets its own, wider, bound; two launches per step grow by
# ~20 us each (1 % of the C5 step).
SPLIT_OUTPUT_STAGE = 1
TEMPORAL_CONV_FUSED = 1   # (round 6) the causal temporal Conv1d as one (3 x 1)-tap launch (ABI 10: ImagenIgemmParams.pad_x1) instead of three 1x1 GEMMs
TIME_CHAIN_F32 = 0        # (round 6, call A) 1 = to_time_cond and the batched time MLPs on fp32 rows (IMAGEN_OP_LINEAR_F32) as the image planner runs them: priced in the
                          # plan interpreter at +-0.5 % on C5 (cond 0.970 -> 0.965e-3, null 0.901 -> 0.905e-3) and measured on MI355X at 9.67e-4 / 9.97e-4 against 9.64e-4 /
                          # 9.76e-4 without — no gain on the video denoiser, so its chain stays on the fp16 GEMMs
SPLIT_OUTPUT_MAX_K = 640          # taps * input channels of the unsplit weight (dim 64: 576)
SPLIT_OUTPUT_FLOPS = 4.0e10       # 2 * pixels * Cout * (2 K) of the split launch (C5: 1.9e10)


class UnetEngine3D(UnetEngine):

    def enable_time_table(self, coef, step_ptr):
        """(The per-request time table of the image engine is not built for the video plan: its step keeps the per-step chain.)"""
        return None

    def __init__(self, unet, rows: int, src_batch: int, frames: int, size: int, device, with_text: bool = True, ignore_time: bool = False,
                 dry: bool = False, pre_frames: int = 0, post_frames: int = 0):
        self.Fx, self.Fpre, self.Fpost = frames, pre_frames, post_frames   # frames of the sampler state / of the two prompts
        self.F = frames + pre_frames + post_frames                         # frames the network runs on
        self.ignore_time = ignore_time
        self.temporal = not ignore_time
        assert self.F <= 128, "the temporal attention kernels hold at most 128 frames per pixel"
        div = getattr(unet, 'total_temporal_divisor', 1)
        assert pre_frames % div == 0 and post_frames % div == 0, \
            f'the number of conditioning frames must be divisible by {div}'                     # iv.py:1700, 1713
        if getattr(unet, 'self_cond', False) and (pre_frames or post_frames):
            from .imagen import _out_of_scope
            _out_of_scope("Unet3D(self_cond=True) with cond_video_frames / post_cond_video_frames (the reference cannot concatenate a "
                          "self-conditioning clip of the frames of x with the extended clip either, iv.py:1676, 1703)")
        super().__init__(unet, rows, src_batch, size, device, with_text=with_text, dry=dry)

    # ------------------------------------------------------------------------------------------ views
    def frames(self, a: Act, F: int) -> Act:
        """clip / time view -> per-frame view."""
        n = a.B * a.H * a.W
        RF = self.R * F
        P = n // RF
        S = int(round(math.sqrt(P)))
        assert S * S == P and a.ld == a.C
        return Act(a.t, RF, S, S, a.C, a.C, P * a.C, a.off, ssq=a.ssq)

    def clip(self, a: Act, F: int) -> Act:
        assert a.ld == a.C and a.B == self.R * F
        return Act(a.t, self.R, F * a.H, a.W, a.C, a.C, F * a.H * a.W * a.C, a.off, ssq=a.ssq)

    def _alloc_io(self):
        super()._alloc_io()
        R, S, u, F, Fx = self.R, self.S, self.unet, self.F, self.Fx
        # frame-major fp32 images: (b, f, c, h, w); the sampler's state and the prediction it reads hold the Fx denoised frames only
        self.x_in = self.f32buf(self.src_batch, Fx, u.channels, S, S, zero=True)
        self.lowres_in = self.f32buf(self.src_batch, Fx, u.channels, S, S, zero=True) if self.lowres else None
        self.out = self.f32buf(R, Fx, u.channels_out, S, S)
        self.out_full = self.f32buf(R, F, u.channels_out, S, S) if F != Fx else self.out   # what final_conv writes
        # conditioning image (Unet3D(cond_images_channels=...), iv.py:1722-1731): ONE image per sample, repeated over every frame the
        # network runs on; the init conv reads it as a second, channel-concatenated input like the image Unet does
        cc = getattr(u, 'cond_images_channels', 0)
        # self-conditioning clip (Unet3D(self_cond=True), iv.py:1674-1676): the previous evaluation's thresholded x0 over the frames of x,
        # frame-major like `x_in`, zeros at first.  As on the image path it is the leading part of the init conv's second input
        # `cimg`, packed at the start of every step.  It never meets a conditioning image (Unet3D refuses the two together) nor prompt
        # frames (__init__), so F == Fx here
        sc = u.channels if getattr(u, 'self_cond', False) else 0
        assert not (sc and cc) and not (sc and F != Fx)
        self.self_cond_in = self.f32buf(self.src_batch, Fx, sc, S, S, zero=True) if sc else None
        self.cimg = self.new(R * F, S, S, (sc + cc + 7) // 8 * 8, zero=True) if sc + cc else None

    def set_cond_images(self, cond_images: torch.Tensor):
        """(src_batch, cond_images_channels, h, w), values as given: resized to this engine's resolution with the unet's resize_mode
        (resize_video_to after the repeat over frames, iv.py:1728-1729: the frames are identical, so one 2-D resize), packed to fp16
        NHWC and written to every frame of every row — static over the timesteps."""
        u, R, S, F = self.unet, self.R, self.S, self.F
        cc = u.cond_images_channels
        assert self.cimg is not None, 'this unet was built without cond_images_channels'
        assert cond_images.ndim == 4 and cond_images.shape[0] == self.src_batch and cond_images.shape[1] == cc, \
            'the number of channels on the conditioning image you are passing in does not match what you specified on initialiation of the unet'
        ci = cond_images.to(self.dev).float()
        if tuple(ci.shape[-2:]) != (S, S):
            ci = TF.interpolate(ci, S, mode=getattr(u, 'resize_mode', 'nearest'))
        packed = torch.zeros(self.src_batch, S, S, self.cimg.C, device=self.dev)
        packed[..., :cc] = ci.permute(0, 2, 3, 1)
        packed = packed.to(torch.float16).repeat(R // self.src_batch, 1, 1, 1)                       # rows: [cond..., null...]
        self.cimg.t.view(R, F, S, S, self.cimg.C).copy_(packed[:, None].expand(-1, F, -1, -1, -1))

    # ------------------------------------------------------------------------------------------ step plan
    # The traversal is engine.UnetEngine._build_step_plan; these are the video path's versions of its hooks (iv.py:1751-1941).
    PLAN_NAME = "unet3d-step"
    DOWN = dict(pre=0, init=1, blocks=2, attn=3, peg=4, tattn=5, tdown=6, post=7)
    UP = dict(init=0, blocks=1, attn=2, peg=3, tattn=4, tup=5, up=6)
    FINAL_SKIP_SCALE = None  # (no skip there: the value is inert, but it is a field of the launch record, which is pinned with the levels' scale)

    def _pack_inputs(self, plan):
        u, R, S, F, Fx = self.unet, self.R, self.S, self.F, self.Fx
        self.img = self.new(R * F, S, S, 8, zero=True)
        xin = self.x_in.view(self.src_batch * Fx, u.channels, S, S)
        lin = self.lowres_in.view(self.src_batch * Fx, u.channels, S, S) if self.lowres else None
        self.img_x = self.img if F == Fx else self.new(R * Fx, S, S, 8)       # the packed Fx frames [x | lowres | zero pad]
        self._pack_op = ops.pack_image(plan, xin, lin, self.img_x, brep=R // self.src_batch, label="pack_frames")
        plan.keep += [self.x_in, self.lowres_in] if self.lowres else [self.x_in]
        if self.self_cond_in is not None:            # the second 8-channel image, as engine.UnetEngine packs it (F == Fx: _alloc_io)
            self._self_cond_op = ops.pack_image(plan, self.self_cond_in.view(self.src_batch * Fx, u.channels, S, S), None, self.cimg,
                                                brep=R // self.src_batch, label="pack_self_cond")
            plan.keep += [self.self_cond_in]
        self.fin2 = None
        if F != Fx:
            # prompt frames: clip = [post | pre | x] (iv.py:1703, 1716); the prompt slots are static, the Fx frames land behind them
            fr = S * S * 8
            ops.rows_copy(plan, self.img_x.t, self.img.t, B=R, rows=1, C=Fx * fr, src_bs=Fx * fr, src_rs=0, dst_bs=F * fr, dst_rs=0,
                          dst_off=(self.Fpost + self.Fpre) * fr, label="place_frames")
            if self.lowres and self.Fpost:
                # final_conv reads the low-res clip extended as [pre | lowres | post] (iv.py:1687, 1691) — another frame order than
                # the input clip's once there are succeeding prompt frames: its own buffer, same channel slots as `img`
                self.fin2 = self.new(R * F, S, S, 8, zero=True)
                ops.rows_copy(plan, self.img_x.t, self.fin2.t, B=R, rows=1, C=Fx * fr, src_bs=Fx * fr, src_rs=0, dst_bs=F * fr, dst_rs=0,
                              dst_off=self.Fpre * fr, label="place_lowres_frames")

    def _time_chain_args(self) -> dict:
        """The image Unet's chain (iv.py:1764-1781), one (scale, shift) row per frame, plain fp16 weights."""
        return dict(replicas=self.F, split=False, f32=TIME_CHAIN_F32)

    def _temporal(self, plan, x: Act, peg, tattn, peg_name: str, tattn_name: str, f: int, tap: str = None) -> Act:
        """Temporal PEG, then temporal attention; nothing under `ignore_time`.  `tap`: the prefix of a tap after each."""
        if self.ignore_time:
            return x
        x = self._temporal_peg(plan, x, peg, peg_name, f)
        if tap:
            self.taps[tap + '_peg'] = x
        x = self._temporal_attn(plan, x, tattn, tattn_name, f)
        if tap:
            self.taps[tap + '_tattn'] = x
        return x

    def _stem(self, plan) -> Act:
        u = self.unet
        x = self._temporal(plan, self._init_conv3d(plan), u.init_temporal_peg, u.init_temporal_attn, "init_temporal_peg", "init_temporal_attn", self.F)
        self.taps['init'] = x
        return x

    def _level_attn(self, plan, x: Act, tb, name: str, f: int) -> Act:
        return self._transformer3d(plan, x, tb, name, f)

    def _level_temporal(self, plan, x: Act, lvl, idx: dict, name: str, f: int) -> Act:
        return self._temporal(plan, x, lvl[idx['peg']], lvl[idx['tattn']], f"{name}.{idx['peg']}", f"{name}.{idx['tattn']}", f)

    def _frames_down(self, plan, x: Act, lvl, i: int, f: int) -> tuple:
        tdown = lvl[self.DOWN['tdown']]
        if tdown is None or self.ignore_time:
            return x, f
        return self._temporal_down(plan, x, tdown, f"downs.{i}.{self.DOWN['tdown']}", f), f // self.lc["temporal_strides"][i]

    def _frames_up(self, plan, x: Act, lvl, i: int, f: int) -> tuple:
        tup = lvl[self.UP['tup']]
        if tup is None or self.ignore_time:
            return x, f
        return self._temporal_up(plan, x, tup, f"ups.{i}.{self.UP['tup']}", f), f * self.lc["temporal_strides"][len(self.unet.ups) - 1 - i]

    def _mid(self, plan, x: Act, f: int) -> Act:
        u = self.unet
        self.taps['mid_in'] = x
        x = self._resnet(plan, x, None, u.mid_block1, "mid_block1", with_cond=True, f=f)
        self.taps['mid_block1'] = x
        if u.mid_attn is not None:                    # Residual(Attention) over all f*h*w tokens, no context, no feed-forward
            tok = self.clip(x, f).tokens()
            y, _ = self._self_attn_out(plan, self._self_attn(plan, tok, u.mid_attn.fn, "mid_attn.fn", with_context=False), tok, u.mid_attn.fn, "mid_attn.fn")
            x = Act(y.t, x.B, x.H, x.W, x.C, x.C, x.H * x.W * x.C)
        self.taps['mid_attn'] = x
        x = self._temporal(plan, x, u.mid_temporal_peg, u.mid_temporal_attn, "mid_temporal_peg", "mid_temporal_attn", f, tap='mid')
        return self._resnet(plan, x, None, u.mid_block2, "mid_block2", with_cond=True, f=f)

    def _head(self, plan, x: Act):
        self._final_conv3d(plan, x)

    # ------------------------------------------------------------------------------------------ convolutions
    def _init_conv3d(self, plan) -> Act:
        """CrossEmbedLayer per frame (iv.py:1121-1146) as ONE kmax x kmax conv, or the plain init conv."""
        out = self.new(self.R * self.F, self.S, self.S, self.lc["init_dim"])
        self._igemm_ssq(plan, self.img, self.W.get("init_conv", lambda: self._init_conv_weight(_wb2d)), out, x2=self.cimg, label="init_conv")
        return out

    def _final_conv3d(self, plan, x: Act):
        """final_conv over cat(x, lowres_cond_img) per frame (iv.py:1928-1931) -> fp32 (R, F, C, H, W)."""
        u = self.unet
        extra = (self.fin2 if self.fin2 is not None else self.img) if self.lowres else None
        cw = _w2d(u.final_conv)

        kh_ = cw.weight.shape[-1]
        split = extra is None and self._split_output(x.C, kh_ * kh_, cw.weight.shape[0], x.rows)

        make = lambda: self._final_conv_weight(_wb2d, x.C, extra is not None, split)
        out4 = self.out_full.view(self.R * self.F, u.channels_out, self.S, self.S)
        ops.igemm(plan, x, self.W.get("final_conv|split" if split else "final_conv", make), out4, x2=extra, out_mode=OUT_NCHW_F32, label="final_conv")
        plan.keep.append(self.out_full)
        if self.F != self.Fx:
            # out[:, :, len(pre):][:, :, :-len(post)] (iv.py:1933-1939): frames [Fpre, Fpre + Fx) of every clip; fp32 moved as fp16 pairs
            fr = 2 * u.channels_out * self.S * self.S
            ops.rows_copy(plan, self.out_full, self.out, B=self.R, rows=1, C=self.Fx * fr, src_bs=self.F * fr, src_rs=0,
                          dst_bs=self.Fx * fr, dst_rs=0, src_off=self.Fpre * fr, label="cut_frames")
            plan.keep.append(self.out)

    def set_cond_video_frames(self, cond_video_frames: Optional[torch.Tensor], post_cond_video_frames: Optional[torch.Tensor]):
        """The prompt frames of the following forward / sampling calls, each (src_batch, c, f', h, w) with values as given (the
        reference does not normalise them): nearest-resized to this engine's resolution, frame count unchanged (resize_video_to,
        iv.py:1702, 1715), and written to the static slots of the packed input clip — and of the final conv's low-res clip, where a
        low-res stage sees them as extra low-res frames (iv.py:1686-1692; there the reference needs them at the stage's size)."""
        u, R, S, F = self.unet, self.R, self.S, self.F
        c = u.channels
        img = self.img.t.view(R, F, S, S, 8)
        fin2 = self.fin2.t.view(R, F, S, S, 8) if self.fin2 is not None else None
        for v, n, at_in, at_fin in ((cond_video_frames, self.Fpre, self.Fpost, 0), (post_cond_video_frames, self.Fpost, 0, self.Fpre + self.Fx)):
            assert (v is None) == (n == 0), 'this engine was planned for another number of conditioning frames'
            if v is None:
                continue
            assert v.ndim == 5 and v.shape[0] == self.src_batch and v.shape[1] == c and v.shape[2] == n, \
                f'conditioning frames must be ({self.src_batch}, {c}, {n}, h, w), got {tuple(v.shape)}'
            v = v.to(self.dev).float()
            if self.lowres:
                assert v.shape[-1] == S and v.shape[-2] == S, \
                    'a low-res-conditioned Unet3D concatenates the conditioning frames with its low-res clip: they must have its size'
            elif tuple(v.shape[-2:]) != (S, S):
                v = TF.interpolate(v, (n, S, S), mode='nearest')
            fm = v.permute(0, 2, 3, 4, 1)                                   # (b, f', h, w, c)
            packed = torch.zeros(self.src_batch, n, S, S, 8, device=self.dev)
            packed[..., :c] = fm
            if self.lowres:
                packed[..., c:2 * c] = fm                                   # cat((frames, frames), dim = 1), iv.py:1688, 1692
            packed = packed.to(torch.float16).repeat(R // self.src_batch, 1, 1, 1, 1)
            img[:, at_in:at_in + n] = packed
            if fin2 is not None:
                fin2[:, at_fin:at_fin + n] = packed

    def _split_output(self, Cin: int, taps: int, Cout: int, pixels: int) -> bool:
        """A split-precision weight for a launch of the output stage (SPLIT_OUTPUT_* above)?"""
        return bool(SPLIT_OUTPUT_STAGE and Cin % 8 == 0 and taps * Cin <= SPLIT_OUTPUT_MAX_K
                    and 4.0 * pixels * Cout * taps * Cin <= SPLIT_OUTPUT_FLOPS)

    def _temporal_conv(self, plan, x: Act, conv, name: str, f: int) -> Act:
        """Causal Conv1d(k = 3) over the frames of every pixel (iv.py:436-449).  TEMPORAL_CONV_FUSED: ONE launch — in the (clip, frame, pixel) view it is
        a 3 x 1 window over rows = frames with two zero rows in front (ops.igemm(causal_rows=True), kernel family 0): one fp32 accumulation
        instead of three launches that pass their partial sums through fp16 (rounds 1-5: three accumulating 1x1 GEMMs on frame-shifted views,
        144 of the 320 launches of a C5 step)."""
        R = self.R
        C, P = x.C, x.H * x.W
        w = conv.weight.detach().float()                       # (C_out, C_in, 3): tap k multiplies frame f - 2 + k
        K = w.shape[-1]
        y = self.new(x.B, x.H, x.W, w.shape[0])
        Co = w.shape[0]
        if TEMPORAL_CONV_FUSED and C % 8 == 0:
            pw = self.W.raw(f"{name}.taps", w.unsqueeze(-1), conv.bias.detach().float())       # (C_out, C_in, 3, 1)
            ops.igemm(plan, Act(x.t, R, f, P, C, C, f * P * C, x.off), pw, Act(y.t, R, f, P, Co, Co, f * P * Co, y.off), causal_rows=True,
                      label=f"{name}.taps")
            return y
        for shift in range(min(K, f)):                         # shift 0: the current frame (with the bias), 1: f-1, 2: f-2
            tap = K - 1 - shift
            pw = self.W.raw(f"{name}.tap{tap}", w[:, :, tap], conv.bias.detach().float() if shift == 0 else None)
            n = f - shift
            xin = Act(x.t, R, n, P, C, C, f * P * C, x.off)
            yout = Act(y.t, R, n, P, Co, Co, f * P * Co, y.off + shift * P * Co)
            ops.igemm(plan, xin, pw, yout, res=yout if shift else None, label=f"{name}.tap{tap}")
        return y

    # ------------------------------------------------------------------------------------------ ResnetBlock (iv.py:743-815)
    # engine.UnetEngine._resnet with f frames per clip; what differs from the image path is stated here and in `temporal`, clip / frames above.
    SHORTCUTS = False   # the image path's producer shortcuts (engine.UnetEngine.SHORTCUTS) stay off: the C5 plan is pinned without them

    def _spatial(self, project):
        return project.spatial_conv

    def _split_block1(self, b) -> bool:
        """The output stage's block1 takes a split-precision weight (SPLIT_OUTPUT_* above)."""
        return b.name == "final_res_block" and self._split_output(b.Cin, 9, b.Cout, b.px)

    def _resnet_inputs(self, plan, x: Act, skip: Optional[Act], rb, name: str, skip_scale, f: int):
        self._ssq_of(plan, x, name + ".block1.stat_x")       # (this planner reduces x's statistics ahead of the skip's: the launch order is pinned)
        return super()._resnet_inputs(plan, x, skip, rb, name, skip_scale, f)

    # ------------------------------------------------------------------------------------------ temporal PEG / attention
    def _temporal_peg(self, plan, x: Act, mod, name: str, f: int) -> Act:
        conv = mod.fn[1]
        C = x.C
        out = self.new(x.B, x.H, x.W, C)
        ops.temporal_peg(plan, x, self.W.f32(name + ".w", lambda: conv.weight.reshape(C, 3)), self.W.f32(name + ".b", lambda: conv.bias), out,
                         B=self.R, F=f, causal=self.unet.time_causal_attn, label=name)
        return out

    def _position_bias(self, attn, f: int) -> torch.Tensor:
        """[heads, f, f+1] fp32: column 0 = the learned null-key bias, columns 1.. = DynamicPositionBias(i - j) (iv.py:1208-1223,
        547-552).  Input-independent: evaluated once from the parameters when the plan is built."""
        rp = attn.rel_pos_bias
        with torch.no_grad():
            pos = torch.arange(-f + 1, f, dtype=torch.float32).reshape(-1, 1)
            for layer in list(rp.mlp)[:-1]:
                lin, norm = layer[0], layer[1]
                h = TF.linear(pos, lin.weight.detach().float().cpu(), lin.bias.detach().float().cpu())
                h = (h - h.mean(-1, keepdim=True)) * torch.rsqrt(h.var(-1, unbiased=False, keepdim=True) + 1e-5) * norm.g.detach().float().cpu()
                pos = TF.silu(h)
            last = rp.mlp[-1]
            pos = TF.linear(pos, last.weight.detach().float().cpu(), last.bias.detach().float().cpu())       # (2f-1, heads)
            idx = torch.arange(f).reshape(-1, 1) - torch.arange(f).reshape(1, -1) + (f - 1)
            bias = pos[idx].permute(2, 0, 1)                                                               # (heads, f, f)
            null = attn.null_attn_bias.detach().float().cpu().reshape(-1, 1, 1).expand(-1, f, 1)
            return torch.cat((null, bias), dim=-1).contiguous()

    def _temporal_attn(self, plan, x: Act, mod, name: str, f: int) -> Act:
        """x + Attention(causal, relative position bias) along the frames of every pixel (iv.py:257-270, 1416)."""
        W, R = self.W, self.R
        attn = mod.fn.fn
        nm = name + ".fn.fn"
        C, P = x.C, x.H * x.W
        heads, dh = attn.heads, attn.dim_head
        rows = R * f * P
        tok = Act(x.t, 1, 1, rows, C, C, rows * C, x.off)
        wqkv = W.raw(nm + ".qkv", torch.cat((attn.to_q.weight.detach().float(), attn.to_kv.weight.detach().float())), None)
        bias = W.get(f"{nm}.bias.{f}", lambda: self._position_bias(attn, f).to(self.dev))

        def core(plan, qkv: Act) -> Act:
            o = self.new(1, 1, rows, heads * dh)
            ops.temporal_attention(plan, qkv, W.f32(nm + ".null_kv", lambda: attn.null_kv), W.f32(nm + ".q_scale", lambda: attn.q_scale),
                                   W.f32(nm + ".k_scale", lambda: attn.k_scale), bias, o, B=R, F=f, P=P, heads=heads, causal=attn.causal,
                                   scale=SIM_SCALE, head_dim=dh, label=nm + ".attn")
            return o
        out = self.new(x.B, x.H, x.W, C)
        self._token_attn(plan, tok, nm, wqkv, W.f32(nm + ".norm.g", lambda: _pad_vec(attn.norm.g, wqkv.Cin_pad)), core, W.conv(nm + ".to_out", attn.to_out[0]),
                         W.f32(nm + ".out_g", lambda: attn.to_out[1].g), Act(out.t, 1, 1, rows, C, C, rows * C), in_label=".qkv")
        return out

    # ------------------------------------------------------------------------------------------ TransformerBlock (iv.py:1059-1091)
    def _transformer3d(self, plan, x: Act, tb: TransformerBlock3dP, name: str, f: int) -> Act:
        cur = x
        for d, (attn, ff) in enumerate(tb.layers):
            nm = f"{name}.layers.{d}"
            tok = self.clip(cur, f).tokens()
            y, _ = self._self_attn_out(plan, self._self_attn(plan, tok, attn, nm + ".0", with_context=True), tok, attn, nm + ".0")
            cur = Act(y.t, x.B, x.H, x.W, x.C, x.C, x.H * x.W * x.C)
            cur = self._chan_feed_forward(plan, cur, ff, nm + ".1", f)
        return cur

    def _chan_feed_forward(self, plan, x: Act, ff, name: str, f: int) -> Act:
        """x + ChanFeedForward(x) (iv.py:1048-1057): per-position LayerNorm over C -> 1x1 -> GELU -> [second half of the hidden channels
        taken from the previous frame] -> LayerNorm -> 1x1: the image path's feed-forward on the token view, with the shift in between."""
        R, C, P = self.R, x.C, x.H * x.W
        rows = R * f * P

        def shift(hid: Act) -> Act:
            hidden = hid.C
            half = hidden // 2 + hidden % 2                       # torch.chunk(2): the first chunk takes the ceiling
            assert half % 8 == 0 and (hidden - half) % 8 == 0, "time token shift needs 8-channel aligned halves"
            sh = self.new(1, 1, rows, hidden)
            fr = P * hidden                                       # elements per frame
            ops.rows_copy(plan, hid.t, sh.t, B=R, rows=f * P, C=half, src_bs=f * fr, src_rs=hidden, dst_bs=f * fr, dst_rs=hidden,
                          label=name + ".keep_half")
            if f > 1:
                ops.rows_copy(plan, hid.t, sh.t, B=R, rows=(f - 1) * P, C=hidden - half, src_bs=f * fr, src_rs=hidden, dst_bs=f * fr,
                              dst_rs=hidden, src_off=half, dst_off=fr + half, label=name + ".shift_half")
            zeros = self.W.get(("zeros16", hidden), lambda: torch.zeros(hidden, dtype=torch.float16, device=self.dev))
            ops.rows_copy(plan, zeros, sh.t, B=R, rows=P, C=hidden - half, src_bs=0, src_rs=0, dst_bs=f * fr, dst_rs=hidden, dst_off=half,
                          label=name + ".shift_zero")
            return sh

        tok = Act(x.t, 1, 1, rows, C, C, rows * C, x.off)
        on = getattr(ff, "time_token_shift", True) and x.B == R * f      # 5-D input only (iv.py:1041-1042); here always
        return self._feed_forward(plan, tok, ff, name, labels=(".conv1", ".conv2"), between=shift if on else None, out=self.new(x.B, x.H, x.W, C))

    # ------------------------------------------------------------------------------------------ resampling
    def _temporal_down(self, plan, x: Act, mod, name: str, f: int) -> Act:
        """'b c (f p) h w -> b (c p) f h w' + 1x1 conv (iv.py:681-686), p = 2: a two-input GEMM over the even / odd frames."""
        stride = mod.stride
        assert stride == 2, "temporal stride 2 only (two-input GEMM)"
        cw = _w2d(mod[1])
        C = x.C
        w = cw.weight[:, :, 0, 0]                                           # (o, c*2) with input channel index c*2 + p

        def make():
            return ops.pack_weight(torch.cat((w[:, 0::2], w[:, 1::2]), dim=1), cw.bias, self.dev)
        pw = self.W.get(name, make)
        n = x.B // 2
        fr = x.H * x.W * C
        even = Act(x.t, n, x.H, x.W, C, C, 2 * fr, x.off)
        odd = Act(x.t, n, x.H, x.W, C, C, 2 * fr, x.off + fr)
        out = self.new(n, x.H, x.W, pw.Cout)
        self._igemm_ssq(plan, even, pw, out, x2=odd, label=name)
        return out

    def _temporal_up(self, plan, x: Act, mod, name: str, f: int) -> Act:
        """Conv1d(C -> C*r, 1) + SiLU + 'b (c r) n -> b c (n r)' (iv.py:649-679): one GEMM per phase j < r writing frames j::r."""
        r = mod.stride
        cw = _w2d(mod.net[0])
        w, b = cw.weight[:, :, 0, 0], cw.bias                                # rows c*r + j
        co = w.shape[0] // r
        out = self.new(x.B * r, x.H, x.W, co)
        fr = x.H * x.W * co
        for j in range(r):
            pw = self.W.get(f"{name}.phase{j}", lambda j=j: ops.pack_weight(w[j::r], b[j::r], self.dev))
            dst = Act(out.t, x.B, x.H, x.W, co, co, r * fr, out.off + j * fr)
            ops.igemm(plan, x, pw, dst, act_out=ACT_SILU, label=f"{name}.phase{j}")
        return out
