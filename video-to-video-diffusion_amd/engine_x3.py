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

from typing import Optional

from .engine import Act, UNetProgram, VAEDecodeProgram, VAEEncodeProgram
from .engine_f32 import ConvFamily, UNetProgramF32, VAEDecodeProgramF32, VAEEncodeProgramF32, _F32Ops

CONV_X3 = ConvFamily(entry="conv_bf16x3", key_lead="bf16x3", audit_kind="conv_fwd_x3", label="conv_bf16x3_mfma")


class _X3Ops(_F32Ops):
    """engine_f32._F32Ops with the convolution on ctsi_conv_bf16x3_fwd."""

    precision = "bf16x3"

    def conv(self, name: str, weight_fn, bias_fn, x1: Act, x2: Optional[Act], **kw):
        """engine_f32._F32Ops.conv (same parameters, same fp32 operands and outputs) on ctsi_conv_bf16x3_fwd."""
        return self._conv_family(CONV_X3, name, weight_fn, bias_fn, x1, x2, **kw)


class UNetProgramX3(_X3Ops, UNetProgramF32):
    """engine_f32.UNetProgramF32 with bf16x3 convolutions."""


class VAEEncodeProgramX3(_X3Ops, VAEEncodeProgramF32):
    """engine_f32.VAEEncodeProgramF32 with bf16x3 convolutions."""


class VAEDecodeProgramX3(_X3Ops, VAEDecodeProgramF32):
    """engine_f32.VAEDecodeProgramF32 with bf16x3 convolutions (one device; the tanh head stores fp32 NCDHW)."""


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
