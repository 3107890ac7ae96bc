"""UNet3D — host-side mirror of the reference denoiser's interface (reference models/unet3d.py).

Only the *module tree* lives here: parameter names, shapes and construction order follow the
reference so that `load_state_dict(strict=True)` of a reference checkpoint works and
`torch.manual_seed(s)` before construction yields the same initial weights.  The arithmetic is not
implemented in Python: `UNet3D.forward` compiles the tree into a libctsi program (engine.UNetProgram)
and runs it on the HIP stream.  Calling it on CPU tensors raises — there is no fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .engine import Ctx, UNetProgram, cached_program, check_attention_mode
from .engine_f32 import check_precision
from .engine_x3 import unet_program
from .lib import CtsiError
from .norm_mod import check_dropout, dropout_threshold  # noqa: F401  (re-exported)
from .spatial_attention import check_spatial_attention_supported

_GROUP_CANDIDATES = (32, 16, 8, 4, 2, 1)


def _largest_group_count(channels: int) -> int:
    """Largest of 32,16,...,1 dividing `channels` (reference unet3d.py:62-68 and twins)."""
    return next((g for g in _GROUP_CANDIDATES if channels % g == 0), 1)


class _EngineOnly(nn.Module):
    """Sub-blocks carry parameters only; they execute as part of the enclosing network's program."""

    def forward(self, *args, **kwargs):  # pragma: no cover - defensive
        raise CtsiError(f"{type(self).__name__} is executed by the HIP engine as part of UNet3D / the VAE; "
                        "call the enclosing network instead")


class SinusoidalPositionEmbeddings(_EngineOnly):
    """Parameter-free placeholder keeping `time_mlp.{1,3}` at the reference's Sequential indices
    (unet3d.py:18-32; evaluated by ctsi_time_embed_fwd)."""

    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim


class TimeEmbedding(_EngineOnly):
    def __init__(self, dim: int, time_dim: int):
        super().__init__()
        self.time_mlp = nn.Sequential(SinusoidalPositionEmbeddings(dim), nn.Linear(dim, time_dim), nn.SiLU(),
                                      nn.Linear(time_dim, time_dim))


class Conv3DBlock(_EngineOnly):
    """conv -> GroupNorm -> SiLU (unet3d.py:51-74): 8 groups when C % 8 == 0, else the largest
    divisor from (32..1)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride, padding)
        groups = min(8, out_channels) if out_channels % 8 == 0 else _largest_group_count(out_channels)
        self.norm = nn.GroupNorm(groups, out_channels)
        self.act = nn.SiLU()


class ResBlock3D(_EngineOnly):
    """unet3d.py:77-133.  `scale_shift`: the time projection emits 2 * out_channels values (scale | shift) that modulate the
    normalised features ahead of the activation, silu(gn(h) * (1 + s) + b), instead of one bias added after it (the owning
    UNet3D's `use_scale_shift_norm`); only the shape of `time_mlp.1.{weight,bias}` differs."""

    def __init__(self, in_channels, out_channels, time_dim, scale_shift=False):
        super().__init__()
        self.scale_shift = bool(scale_shift)
        self.conv1 = Conv3DBlock(in_channels, out_channels)
        self.time_mlp = nn.Sequential(nn.SiLU(), nn.Linear(time_dim, (2 if scale_shift else 1) * out_channels))
        self.conv2 = nn.Sequential(nn.Conv3d(out_channels, out_channels, kernel_size=3, padding=1),
                                   nn.GroupNorm(_largest_group_count(out_channels), out_channels))
        self.residual_conv = (nn.Conv3d(in_channels, out_channels, kernel_size=1)
                              if in_channels != out_channels else nn.Identity())
        self.act = nn.SiLU()


class TemporalAttention(_EngineOnly):
    """unet3d.py:136-194: attention along depth.  How it is evaluated is the owning UNet3D's `attention_mode`: 'fast' /
    'exact' reproduce the reference's einsum 'bhqk,bhvc->bhqc' as written -- every query receives the depth SUM of V, the q
    and k thirds of `qkv` have no effect (csrc/attention.hip) -- and 'softmax' computes softmax(q k^T / sqrt(hd)) v over the
    depth positions of each (b, h, w) location (csrc/attention_core.hip).  Parameters and state dict are the same in all
    three."""

    def __init__(self, channels, num_heads=4):
        super().__init__()
        self.num_heads = num_heads
        self.channels = channels
        self.head_dim = channels // num_heads
        assert channels % num_heads == 0, "channels must be divisible by num_heads"
        self.norm = nn.GroupNorm(_largest_group_count(channels), channels)
        self.qkv = nn.Conv3d(channels, channels * 3, kernel_size=1)
        self.proj_out = nn.Conv3d(channels, channels, kernel_size=1)


class SpatialAttention(_EngineOnly):
    """In-plane attention (ADM's attention block; with TemporalAttention, Video Diffusion Models' factorised space-time
    attention): per sample and depth slice, over the N = h * w positions of the plane,
        y = x + proj_out(A),  [q | k | v] = qkv(gn(x)),  A[i] = sum_j softmax_j(q_i . k_j / sqrt(hd)) v_j,
    heads split inside each third as TemporalAttention does.  `proj_out` is zero-initialised (ADM's zero_module): a freshly
    added block is the identity.  Evaluated by csrc/attention_plane.hip (spatial_attention.py), whatever the
    owning UNet3D's `attention_mode` says."""

    def __init__(self, channels, num_heads=4):
        super().__init__()
        self.num_heads = num_heads
        self.channels = channels
        self.head_dim = channels // num_heads
        assert channels % num_heads == 0, "channels must be divisible by num_heads"
        self.norm = nn.GroupNorm(_largest_group_count(channels), channels)
        self.qkv = nn.Conv3d(channels, channels * 3, kernel_size=1)
        self.proj_out = nn.Conv3d(channels, channels, kernel_size=1)
        nn.init.zeros_(self.proj_out.weight)
        nn.init.zeros_(self.proj_out.bias)


def check_spatial_attention_levels(levels, num_levels: int):
    """A sequence of distinct ints in range(num_levels) -> tuple; anything else (a bool, a float, a string, a repeated level, a
    level out of range) is a ValueError."""
    what = f"spatial_attention_levels must be a sequence of distinct ints in range({num_levels}), got {levels!r}"
    if isinstance(levels, (str, bytes)) or not isinstance(levels, (list, tuple)):
        raise ValueError(what)
    out = []
    for v in levels:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < num_levels or v in out:
            raise ValueError(what)
        out.append(v)
    return tuple(out)


class Downsample3D(_EngineOnly):
    def __init__(self, in_channels, out_channels=None):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, in_channels if out_channels is None else out_channels,
                              kernel_size=(3, 4, 4), stride=(1, 2, 2), padding=(1, 1, 1))


class Upsample3D(_EngineOnly):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.ConvTranspose3d(channels, channels, kernel_size=(3, 4, 4), stride=(1, 2, 2),
                                       padding=(1, 1, 1))


class UNet3D(nn.Module):
    """forward(x, t, c) -> predicted noise, all (B, latent_dim, T, h, w) fp32 NCDHW; t int64 (B,).

    Extra attribute `attention_mode` ('fast' | 'exact' | 'softmax', default 'fast'; anything else is a ValueError).  'fast'
    and 'exact' both reproduce the reference's einsum, in which every query receives the depth sum of V (they differ in how
    the rowsum(softmax) == 1 factor is obtained, see attention.hip).  'softmax' is true attention over depth,
    y = x + proj_out(softmax(q k^T / sqrt(hd)) v): same modules and state dict, so a checkpoint loads in either mode, and
    forward, every sampler, guidance, v-prediction, stitching and training honour it.  It needs the whole
    depth on one device (CtsiError with depth sharding) and the bf16 engine (CtsiError with inference_precision='fp32').

    Extra attribute `inference_precision` ('bf16' | 'fp32' | 'bf16x3', default 'bf16'; 'bf16x3' = the fp32 mode with split-bf16
    MFMA convolutions, engine_x3.py, same restrictions as 'fp32') selects the arithmetic of `forward` (under
    no_grad) and of the samplers: bf16 activations and bf16 MFMA operands, or fp32 activations and fp32 MFMA operands
    (engine_f32.py: the reference's fp32 inference, models/model.py:254-259).  'fp32' supports attention_mode='fast' and
    one device only (CtsiError with 'exact' / 'softmax' or with depth sharding).  Training (`diffusion.training_loss`) always runs
    the bf16 programs, whatever this attribute says.

    Constructor argument `use_scale_shift_norm` (default False) selects the time conditioning of every ResBlock3D: False is the
    reference's bias, conv2's input = silu(gn(h)) + e; True is the ADM / EDM scale-shift form, silu(gn(h) * (1 + s) + b) with
    (s | b) = the block's 2C-wide time projection, scale first.  The state dict differs only in the shape of the blocks'
    `time_mlp.1.{weight,bias}`, so a checkpoint loads into a model built with the same value; forward, every sampler,
    guidance, v-prediction, the x0 form, stitching, fp32 inference and training honour it.  It needs the whole
    depth on one device (CtsiError with depth sharding).  Attribute `dropout` (constructor argument, default 0.0, a float
    in [0, 1); anything else is a ValueError) drops conv2's input in every ResBlock3D during training only -- `training_loss`
    with `unet.training` true; inference programs never drop.  It is read at each training forward, and the mask is a pure
    function of (seed, block, element), regenerated in the backward; the 64-bit seed is drawn from torch's default CPU
    generator once per training forward, or taken from the attribute `dropout_seed` when that is an int (a test hook).

    Constructor argument `learn_sigma` (default False): True makes `conv_out[2]` a Conv3d(ch, 2 * latent_dim, 3,
    padding=1) -- nothing else in the state dict changes, so a checkpoint loads into a model built with the same value -- and
    forward returns (B, 2 * latent_dim, T, h, w): channels [0, L) the prediction (eps or v), channels [L, 2L) the raw variance
    channels v of Improved DDPM, read when the diffusion's attribute `var_type` is 'learned_range'.  Every sampler, guidance, the three
    inference precisions, stitching and training honour it; the deterministic samplers ignore the variance channels.  It needs
    the whole depth on one device (CtsiError with depth sharding).

    Constructor argument `spatial_attention_levels` (default (): none): a SpatialAttention -- in-plane
    attention over the h * w positions of every depth slice -- is appended to every down and up stage of the listed levels, after
    the ResBlock3D and after the TemporalAttention where the stage has one, independently of `attention_levels`, and
    `mid_attn_spatial` runs after `mid_attn` when the deepest level is listed.  Appending leaves every existing state-dict key
    where it is, and the new `proj_out` is zero-initialised: a reference checkpoint loads with strict=False and evaluates exactly
    as before until the new blocks are trained.  forward, every sampler, guidance, v-prediction, the x0 form, learn_sigma,
    stitching, training and every attention_mode honour it; it needs the bf16 engine (CtsiError with inference_precision
    'fp32' / 'bf16x3'), the whole depth on one device (CtsiError with depth sharding) and a head dimension in
    {8, 16, 32, 64, 128}.
    """

    def __init__(self, latent_dim=4, model_channels=128, num_res_blocks=2, attention_levels=[1, 2],
                 channel_mult=(1, 2, 4, 4), num_heads=4, time_embed_dim=512, use_checkpoint=False,
                 use_scale_shift_norm=False, dropout=0.0, learn_sigma=False, spatial_attention_levels=()):
        super().__init__()
        self.spatial_attention_levels = check_spatial_attention_levels(spatial_attention_levels, len(channel_mult))
        if not isinstance(learn_sigma, bool):
            raise ValueError(f"learn_sigma must be True or False, got {learn_sigma!r}")
        self.learn_sigma = learn_sigma
        self.use_scale_shift_norm = bool(use_scale_shift_norm)
        self.dropout = check_dropout(dropout)
        self.dropout_seed = None     # test hook: an int here replaces the seed drawn at each training forward
        self.latent_dim = latent_dim
        self.model_channels = model_channels
        self.num_res_blocks = num_res_blocks
        self.attention_levels = attention_levels
        self.channel_mult = channel_mult
        self.num_levels = len(channel_mult)
        self.use_checkpoint = use_checkpoint
        self.attention_mode = "fast"
        self.inference_precision = "bf16"

        self.time_embed = TimeEmbedding(model_channels, time_embed_dim)
        self.conv_in = nn.Conv3d(latent_dim * 2, model_channels, kernel_size=3, padding=1)

        def stage(cin, cout, with_attn, with_spatial):
            layers = [ResBlock3D(cin, cout, time_embed_dim, self.use_scale_shift_norm)]
            if with_attn:
                layers.append(TemporalAttention(cout, num_heads))
            if with_spatial:
                layers.append(SpatialAttention(cout, num_heads))
            return nn.ModuleList(layers)

        self.down_blocks = nn.ModuleList()
        self.down_samples = nn.ModuleList()
        ch = model_channels
        for level, mult in enumerate(channel_mult):
            width = model_channels * mult
            blocks = nn.ModuleList()
            for _ in range(num_res_blocks):
                blocks.append(stage(ch, width, level in attention_levels, level in self.spatial_attention_levels))
                ch = width
            self.down_blocks.append(blocks)
            self.down_samples.append(Downsample3D(ch, ch) if level < self.num_levels - 1 else nn.Identity())

        self.mid_block1 = ResBlock3D(ch, ch, time_embed_dim, self.use_scale_shift_norm)
        self.mid_attn = TemporalAttention(ch, num_heads)
        if self.num_levels - 1 in self.spatial_attention_levels:
            self.mid_attn_spatial = SpatialAttention(ch, num_heads)
        self.mid_block2 = ResBlock3D(ch, ch, time_embed_dim, self.use_scale_shift_norm)

        self.up_blocks = nn.ModuleList()
        self.up_samples = nn.ModuleList()
        for level, mult in enumerate(reversed(channel_mult)):
            width = model_channels * mult
            src_level = self.num_levels - 1 - level
            blocks = nn.ModuleList()
            for i in range(num_res_blocks + 1):
                cin = ch + model_channels * channel_mult[src_level] if i == 0 else ch
                blocks.append(stage(cin, width, src_level in attention_levels,
                                    src_level in self.spatial_attention_levels))
                ch = width
            self.up_blocks.append(blocks)
            self.up_samples.append(Upsample3D(ch) if level < self.num_levels - 1 else nn.Identity())

        self.conv_out = nn.Sequential(nn.GroupNorm(_largest_group_count(ch), ch), nn.SiLU(),
                                      nn.Conv3d(ch, (2 if learn_sigma else 1) * latent_dim, kernel_size=3, padding=1))

    @staticmethod
    def _get_num_groups(channels):
        return _largest_group_count(channels)

    # ---- engine plumbing ---------------------------------------------------------------------------
    def invalidate_engine_cache(self):
        """Drop the engine's cached programs (packed bf16 weights, captured graphs) -- needed only after weight
        writes torch cannot observe (`p.data[...] = ...`, raw-pointer copies); optimizer steps, `load_state_dict`
        and replaced parameters are detected automatically (engine.Program._fingerprint)."""
        from .engine import invalidate_engine_cache
        invalidate_engine_cache(self)

    def program(self, ctx: Ctx, n: int, d: int, h: int, w: int, max_rows: int) -> UNetProgram:
        precision = check_precision(self.inference_precision)
        check_attention_mode(self.attention_mode)
        check_spatial_attention_supported(self, precision)
        key = ("unet", ctx.device.index, n, d, h, w, max_rows, self.attention_mode, precision)
        cls = unet_program(precision)
        return cached_program(self, key, lambda: cls(ctx, self, n, d, h, w, max_rows, self.attention_mode))

    @torch.no_grad()
    def forward(self, x, t, c):
        check_precision(self.inference_precision)
        check_attention_mode(self.attention_mode)
        check_spatial_attention_supported(self, self.inference_precision)
        if not (x.is_cuda and c.is_cuda):
            raise CtsiError("UNet3D.forward runs on the HIP engine: move the tensors to a ROCm device "
                            "(there is no CPU path; the oracle under oracle/ is test infrastructure only)")
        n, L, d, h, w = x.shape
        if L != self.latent_dim or tuple(c.shape) != tuple(x.shape):
            raise ValueError(f"expected x and c of shape (B, {self.latent_dim}, T, h, w), got {tuple(x.shape)} "
                             f"and {tuple(c.shape)}")
        ctx = Ctx.get(x.device)
        with ctx.scope():
            prog = self.program(ctx, n, d, h, w, max_rows=n)
            prog_plain = prog
            if getattr(prog, "sampler_kind", None) is not None:
                raise CtsiError("internal: plain forward reuses a sampler program")
            prog_plain.load_latents(x, c)
            # an integer-valued t keeps the int32 embedding; a fractional floating t is embedded as is (the reference
            # embeds t as a float, models/unet3d.py:25-32)
            t_vals = torch.as_tensor(t).reshape(-1).tolist()
            prog_plain.set_schedule([int(v) if float(v).is_integer() else float(v) for v in t_vals])
            prog_plain.launch()
            return prog_plain.out_ncdhw()
