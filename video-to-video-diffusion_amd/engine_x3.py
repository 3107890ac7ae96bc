"""bf16x3 inference mode of the engine: the fp32 programs of engine_f32.py with every convolution on the bf16 MFMA.

Tensors stay fp32.  Inside the convolution (csrc/conv_bf16x3.hip) each fp32 operand v is split as hi = bf16(v) (round to
nearest even), lo = bf16(v - float(hi)), and the kernel sums xh wh + xh wl + xl wh in fp32: three bf16 MFMAs where the fp32
mode spends sixteen MFMAs' worth of cycles, about 2^-16 relative error per product in place of bf16's 2^-8.  Only `conv`
differs from engine_f32._F32Ops:

  convolutions  ctsi_conv_bf16x3_fwd, every layer (the VAE's 1-channel stem and 1-channel head included)
  weights       a hi and a lo bf16 image, split once at pack time, cached under a key led by "bf16x3"
  everything else (GroupNorm, attention, guidance, sampler updates, VAE plumbing): the fp32 mode's kernels, unchanged

Not supported (CtsiError, as in the fp32 mode): depth sharding, attention_mode='exact' / 'softmax', training.

PROGRAMS maps an inference precision to its (U-Net, VAE encode, VAE decode) program classes; unet3d.py, vae.py and sampler.py
pick from it.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from .engine import Act, Ctx, UNetProgram, VAEDecodeProgram, VAEEncodeProgram, _ptr, check_attention_mode
from .engine_f32 import UNetProgramF32, VAEDecodeProgramF32, VAEEncodeProgramF32, _F32Ops
from .lib import ConvDesc, ConvOut, CtsiError


def _x3_pack_sig(desc: ConvDesc, cout_pad: int, wbytes: int) -> tuple:
    """The layout half of a bf16x3 packed-image cache key (engine_f32._f32_pack_sig's fields).  The precision leads the key,
    so neither a bf16 nor an fp32 program finds it."""
    return ("bf16x3", int(desc.transposed), (desc.kd, desc.kh, desc.kw), (desc.sh, desc.sw), desc.c1, desc.c2, desc.cout,
            cout_pad, wbytes)


def _unsupported(what: str) -> CtsiError:
    return CtsiError(f"the bf16x3 inference mode {what}")


_FAST_ONLY = ("supports attention_mode='fast' only (the exact mode evaluates the same mathematics, DESIGN section 3.2; the "
              "softmax mode has bf16 kernels only, section 19)")


class _X3Ops(_F32Ops):
    """engine_f32._F32Ops with the convolution on ctsi_conv_bf16x3_fwd."""

    precision = "bf16x3"

    def act(self, n, c, d, h, w, halo: Optional[int] = None) -> Act:
        if halo:
            raise _unsupported("does not support depth sharding")
        return super().act(n, c, d, h, w, halo)

    def attention(self, m, x: Act, mode: str = "fast") -> Act:
        if mode != "fast":
            raise _unsupported(_FAST_ONLY)
        return super().attention(m, x, mode)

    def conv(self, name: str, weight_fn, bias_fn, x1: Act, x2: Optional[Act], *, transposed=False, k=(3, 3, 3), s=(1, 1),
             p=(1, 1, 1), cout: int, cin_w: Optional[int] = None, out: Optional[Act] = None, want_stats=False,
             f32_out=None, f32_strides=None, act: int = 0, fuse_gn=None, ext_out: bool = False, norm_in=None,
             residual: Optional[Act] = None):
        """engine_f32._F32Ops.conv (same parameters, same fp32 operands and outputs) on ctsi_conv_bf16x3_fwd."""
        lib, prog = self.lib, self
        if fuse_gn is not None or ext_out:
            raise CtsiError("internal: the fused GroupNorm tail / halo-extended outputs are bf16-path features")
        c2 = 0 if x2 is None else x2.c
        if cin_w is not None and cin_w != x1.c + c2:
            raise CtsiError(f"internal: fp32 activations carry no padding channels (cin_w={cin_w}, c={x1.c + c2})")
        if x2 is not None and (x2.n, x2.d, x2.h, x2.w) != (x1.n, x1.d, x1.h, x1.w):
            raise CtsiError("internal: concatenated sources of different shapes")
        if norm_in is not None:
            self._norm_in_pass(x1, norm_in)
        desc = ConvDesc(int(transposed), k[0], k[1], k[2], s[0], s[1], p[0], p[1], p[2], x1.n, x1.c, c2, cout, x1.d, x1.h,
                        x1.w, 0)
        if not lib.conv_bf16x3_supported(C.byref(desc)):
            raise CtsiError(f"{name}: {lib.last_error().decode()}")
        self.keep.append(desc)
        do, ho, wo, tps, ncls, cpad = (C.c_int() for _ in range(6))
        lib.conv_bf16x3_geometry(C.byref(desc), C.byref(do), C.byref(ho), C.byref(wo), C.byref(tps), C.byref(ncls),
                                 C.byref(cpad))
        do, ho, wo, tps, ncls, cpad = do.value, ho.value, wo.value, tps.value, ncls.value, cpad.value
        wbytes = lib.conv_bf16x3_weight_bytes(C.byref(desc))
        bias = self._conv_bias(bias_fn)
        sptr = self.ctx.sptr
        holder = self._weight_image(weight_fn, _x3_pack_sig(desc, cpad, wbytes), wbytes,
                                    lambda w, t: lib.conv_bf16x3_pack_weights(C.byref(desc), w, t, sptr))
        fl = lib.conv_bf16x3_flops(C.byref(desc))
        self._count_conv(name, fl)
        stats = self._conv_stats(ncls * x1.n * tps, tps, cpad, ncls) if want_stats else None
        co = ConvOut()
        out_act = self._conv_target(co, x1, cout, (do, ho, wo), out, f32_out, f32_strides)
        if out_act is not None and (out_act.n, out_act.c, out_act.d, out_act.h, out_act.w) != (x1.n, cout, do, ho, wo):
            raise CtsiError("internal: conv output buffer of the wrong shape")
        if residual is not None and (f32_out is not None or residual.t.numel() != out_act.t.numel()):
            raise CtsiError("internal: the residual must have the NDHWC output's shape")
        co.act = act
        self.keep.append(co)
        x1p, x2p = _ptr(x1.t), _ptr(None if x2 is None else x2.t)
        bp, rp = _ptr(bias), _ptr(None if residual is None else residual.t)

        def run():
            co.colsum = prog._colsum.data_ptr() if want_stats else 0
            lib.conv_bf16x3_fwd(C.byref(desc), x1p, x2p, _ptr(holder[0]), bp, rp, C.byref(co), sptr)

        bn = 32 if cout <= 32 else (64 if cout <= 64 else 128)
        kernel = "conv_bf16x3_mfma_128x%d%s" % (bn, "t" if transposed else ("d" if tuple(s) == (2, 2) else ""))
        alg = (4.0 * x1.n * x1.d * x1.h * x1.w * (x1.c + c2) + float(wbytes) + 4.0 * x1.n * do * ho * wo * cout
               * (2 if residual is not None else 1))
        self._emit(run, name, fl, kernel, alg_bytes=alg,
                   audit=dict(kind="conv_fwd_x3", f32=True, x1=x1, x2=x2, weight=weight_fn, bias=bias,
                              transposed=bool(transposed), k=tuple(k), s=tuple(s), p=tuple(p), cout=cout, cin_w=None, act=act,
                              out=out_act, f32_out=f32_out,
                              f32_strides=None if f32_out is None else tuple(int(v) for v in f32_strides), stats=stats,
                              colsum=(lambda: prog._colsum) if want_stats else None, stream_tail=False, fuse_gn=None,
                              residual=residual))
        return out_act, stats


class UNetProgramX3(_X3Ops, UNetProgramF32):
    """engine_f32.UNetProgramF32 with bf16x3 convolutions."""

    def __init__(self, ctx: Ctx, unet, n: int, d: int, h: int, w: int, max_rows: int, attention_mode="fast", shard=None,
                 guided: bool = False, rescale: bool = False, prediction: str = "epsilon"):
        if shard is not None:
            raise _unsupported("does not support depth sharding")
        check_attention_mode(attention_mode)
        if attention_mode != "fast":
            raise _unsupported(_FAST_ONLY)
        super().__init__(ctx, unet, n, d, h, w, max_rows, attention_mode, shard=None, guided=guided, rescale=rescale,
                         prediction=prediction)


class VAEEncodeProgramX3(_X3Ops, VAEEncodeProgramF32):
    """engine_f32.VAEEncodeProgramF32 with bf16x3 convolutions."""


class VAEDecodeProgramX3(_X3Ops, VAEDecodeProgramF32):
    """engine_f32.VAEDecodeProgramF32 with bf16x3 convolutions (one device; the tanh head stores fp32 NCDHW)."""

    def __init__(self, ctx: Ctx, vae, n, d, h, w, shard=None):
        if shard is not None:
            raise _unsupported("does not support depth sharding")
        super().__init__(ctx, vae, n, d, h, w)


# inference precision -> (U-Net program, VAE encode program, VAE decode program)
PROGRAMS = {
    "bf16": (UNetProgram, VAEEncodeProgram, VAEDecodeProgram),
    "fp32": (UNetProgramF32, VAEEncodeProgramF32, VAEDecodeProgramF32),
    "bf16x3": (UNetProgramX3, VAEEncodeProgramX3, VAEDecodeProgramX3),
}
# bytes per activation element, for memory estimates
ACT_BYTES = {"bf16": 2, "fp32": 4, "bf16x3": 4}


def unet_program(precision: str):
    return PROGRAMS[precision][0]


def vae_encode_program(precision: str):
    return PROGRAMS[precision][1]


def vae_decode_program(precision: str):
    return PROGRAMS[precision][2]
