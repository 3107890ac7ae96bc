"""fp32 inference mode of the engine: the U-Net and VAE programs with fp32 activations and fp32 MFMA convolutions.

The reference's `generate()` runs the VAE and the whole sampler in fp32 (models/model.py:254-259).  These programs are
built by the SAME module walks as engine.UNetProgram / VAEEncodeProgram / VAEDecodeProgram and use the same emit,
capture and launch machinery (one captured hipGraph per sampler step); only the primitives differ:

  activations   fp32 NDHWC (exact channel counts: no layout padding)
  convolutions  ctsi_conv_f32_fwd: implicit GEMM on v_mfma_f32_32x32x2_f32, fp32 operands, fp32 accumulation
  weights       fp32 image [class][tap * cpad + ci][cout_pad], cached under a key that carries the precision
  GroupNorm     ctsi_gn_colsum_f32 / conv column sums -> ctsi_gn_finalize (fp64) -> ctsi_gn_apply_f32
  attention     fast mode only: ctsi_attn_depthsum_f32 / _normsum_f32, the folded (proj_out . W_v) matrix (fp64 product,
                rounded once) as one fp32 1x1x1 conv, ctsi_attn_broadcast_add_f32
  sampler       the `_f32` entry of every engine.SAMPLER_STEPS row (the U-Net's z input written in fp32): the update
                is engine.UNetProgram.add_sampler_step, only the input slice differs (_sampler_zin)

Not supported here (CtsiError): depth sharding, attention_mode='exact' / 'softmax', training.  There is no torch conv, MIOpen or BLAS
call on this path: torch allocates and copies.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from .engine import Act, Ctx, UNetProgram, VAEDecodeProgram, VAEEncodeProgram, _ptr, check_attention_mode
from .lib import ConvDesc, ConvOut, CtsiError

PRECISIONS = ("bf16", "fp32", "bf16x3")       # "bf16x3": engine_x3.py


class ConvFamily(NamedTuple):
    """One kernel family of the convolution on fp32 tensors (csrc/conv_f32_frame.h has what the families share)."""
    entry: str          # the C entry points are ctsi_<entry>_{supported, geometry, weight_bytes, pack_weights, flops, fwd}
    key_lead: str       # leads the packed-image cache key
    audit_kind: str
    label: str          # kernel label prefix


CONV_F32 = ConvFamily(entry="conv_f32", key_lead="fp32", audit_kind="conv_fwd", label="conv_f32_mfma")


def _f32_pack_sig(desc: ConvDesc, cout_pad: int, wbytes: int, lead: str = "fp32") -> tuple:
    """The layout half of a packed-image cache key of the convolutions on fp32 tensors: ctsi_conv_*_pack_weights reads the
    descriptor's channel / kernel fields only (never the batch or the spatial size; each supported kernel geometry has one
    padding).  The precision leads the key, so a program of another precision never finds it."""
    return (lead, int(desc.transposed), (desc.kd, desc.kh, desc.kw), (desc.sh, desc.sw), desc.c1, desc.c2, desc.cout,
            cout_pad, wbytes)


def check_precision(p) -> str:
    """Validate an inference precision value ('bf16' | 'fp32' | 'bf16x3'); raises ValueError otherwise."""
    if not isinstance(p, str) or p not in PRECISIONS:
        raise ValueError(f"unknown inference precision {p!r}: expected one of {PRECISIONS}")
    return p


class _F32Ops:
    """The primitive emitters of engine.Program on fp32 tensors (mixed in before the bf16 program class)."""

    precision = "fp32"

    def act(self, n, c, d, h, w, halo: Optional[int] = None) -> Act:
        if halo:
            raise CtsiError(f"the {self.precision} inference mode does not support depth sharding")
        return Act(self.pool.get(n * c * d * h * w, torch.float32), n, c, d, h, w, 0)

    def conv(self, name: str, weight_fn, bias_fn, x1: Act, x2: Optional[Act], **kw):
        """engine.Program.conv on ctsi_conv_f32_fwd (_conv_family has the parameters)."""
        return self._conv_family(CONV_F32, name, weight_fn, bias_fn, x1, x2, **kw)

    def _conv_family(self, fam: ConvFamily, name: str, weight_fn, bias_fn, x1: Act, x2: Optional[Act], *, transposed=False,
                     k=(3, 3, 3), s=(1, 1), p=(1, 1, 1), cout: int, cin_w: Optional[int] = None, out: Optional[Act] = None,
                     want_stats=False, f32_out: Optional[torch.Tensor] = None, f32_strides=None, act: int = 0, fuse_gn=None,
                     ext_out: bool = False, norm_in=None, residual: Optional[Act] = None):
        """engine.Program.conv (which documents the parameters) on the kernels of `fam`.  `residual` (fp32 Act of the
        output's shape) is added in the epilogue.  The fused GroupNorm tail has no fp32 form."""
        lib, prog = self.lib, self
        supported, geometry, weight_bytes, pack_weights, flops, fwd = (
            getattr(lib, f"{fam.entry}_{f}") for f in ("supported", "geometry", "weight_bytes", "pack_weights", "flops", "fwd"))
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
        if not supported(C.byref(desc)):
            raise CtsiError(f"{name}: {lib.last_error().decode()}")
        self.keep.append(desc)
        do, ho, wo, tps, ncls, cpad = (C.c_int() for _ in range(6))
        geometry(C.byref(desc), C.byref(do), C.byref(ho), C.byref(wo), C.byref(tps), C.byref(ncls), C.byref(cpad))
        do, ho, wo, tps, ncls, cpad = do.value, ho.value, wo.value, tps.value, ncls.value, cpad.value
        wbytes = weight_bytes(C.byref(desc))
        bias = self._conv_bias(bias_fn)
        sptr = self.ctx.sptr
        holder = self._weight_image(weight_fn, _f32_pack_sig(desc, cpad, wbytes, fam.key_lead), wbytes,
                                    lambda w, t: pack_weights(C.byref(desc), w, t, sptr))
        fl = flops(C.byref(desc))
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
            fwd(C.byref(desc), x1p, x2p, _ptr(holder[0]), bp, rp, C.byref(co), sptr)

        bn = 32 if cout <= 32 else (64 if cout <= 64 else 128)
        kernel = "%s_128x%d%s" % (fam.label, bn, "t" if transposed else ("d" if tuple(s) == (2, 2) else ""))
        alg = (4.0 * x1.n * x1.d * x1.h * x1.w * (x1.c + c2) + float(wbytes) + 4.0 * x1.n * do * ho * wo * cout
               * (2 if residual is not None else 1))
        self._emit(run, name, fl, kernel, alg_bytes=alg,
                   audit=dict(kind=fam.audit_kind, f32=True, x1=x1, x2=x2, weight=weight_fn, bias=bias,
                              transposed=bool(transposed), k=tuple(k), s=tuple(s), p=tuple(p), cout=cout, cin_w=None, act=act,
                              out=out_act, f32_out=f32_out,
                              f32_strides=None if f32_out is None else tuple(int(v) for v in f32_strides), stats=stats,
                              colsum=(lambda: prog._colsum) if want_stats else None, stream_tail=False, fuse_gn=None,
                              residual=residual))
        return out_act, stats

    def gn_colsum(self, x: Act) -> dict:
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        tps = lib.gn_colsum_f32_tiles(x.d, x.h, x.w)
        self._colsum_need = max(self._colsum_need, 2 * x.n * tps * x.c)
        xp = _ptr(x.t)
        n, c, d, h, w = x.n, x.c, x.d, x.h, x.w

        def run():
            lib.gn_colsum_f32(xp, _ptr(prog._colsum), n, c, d, h, w, None, sptr)

        self._emit(run, "gn.colsum", nbytes=4.0 * n * c * d * h * w,
                   audit=dict(kind="gn_colsum", f32=True, x=x, colsum=lambda: prog._colsum, tps=tps, tile_rows=512))
        return dict(tps=tps, cpad=x.c, nclass=1)

    def gn_apply(self, x: Act, slot: int, gn: nn.GroupNorm, *, silu_pre: bool, tbias=None, tbias_off: int = 0,
                 tbias_stride: int = 0, step_ptr: Optional[torch.Tensor] = None, residual: Optional[Act] = None,
                 silu_post: bool = False, out: Optional[Act] = None, synced: bool = False, film: bool = False,
                 drop=None) -> Act:
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        if drop is not None:
            raise CtsiError("internal: inference programs never drop")
        if film and (tbias is None or residual is not None or silu_post or not silu_pre):
            raise CtsiError("internal: the scale-shift pass is the ResBlock's middle pass only")
        gamma = self.dev_f32(lambda: gn.weight)
        beta = self.dev_f32(lambda: gn.bias)
        self.track(gn.weight, gn.bias)
        if out is None:
            out = self.act(x.n, x.c, x.d, x.h, x.w)
        xp, yp, gp, bp = _ptr(x.t), _ptr(out.t), _ptr(gamma), _ptr(beta)
        tbp = C.c_void_p(0 if tbias is None else tbias.data_ptr() + tbias_off * 4)
        stp = _ptr(step_ptr)
        rp = _ptr(None if residual is None else residual.t)
        n, c, d, h, w, groups, eps = x.n, x.c, x.d, x.h, x.w, gn.num_groups, float(gn.eps)

        def run():
            lib.gn_apply_f32(xp, yp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, n, c, d, h, w, d, groups, eps,
                             int(silu_pre), tbp, tbias_stride, stp, rp, int(silu_post), sptr)

        if film:
            from .norm_mod import emit_gn_apply_mod_f32
            emit_gn_apply_mod_f32(self, xp=xp, yp=yp, slot=slot, gp=gp, bp=bp, n=n, c=c, d=d, h=h, w=w, groups=groups, eps=eps,
                                  tbp=tbp, tbias_stride=tbias_stride, stp=stp,
                                  record=dict(x=x, out=out, sums=lambda: prog._gn_sums, slot=slot, gamma=gamma, beta=beta,
                                              groups=groups, eps=eps, d_stat=d, silu_pre=True, tbias=tbias,
                                              tbias_off=tbias_off, tbias_stride=tbias_stride, step_ptr=step_ptr))
            return out
        self._emit(run, "gn.apply", nbytes=(2 + (residual is not None)) * 4.0 * n * c * d * h * w,
                   audit=dict(kind="gn_apply", f32=True, x=x, out=out, sums=lambda: prog._gn_sums, slot=slot, gamma=gamma,
                              beta=beta, groups=groups, eps=eps, d_stat=d, silu_pre=bool(silu_pre), tbias=tbias,
                              tbias_off=tbias_off, tbias_stride=tbias_stride, step_ptr=step_ptr, residual=residual,
                              silu_post=bool(silu_post)))
        return out

    def unet_resblock(self, m, x: Act, skip: Optional[Act], tbias: torch.Tensor, tbias_off: int, tbias_stride: int,
                      step_ptr: Optional[torch.Tensor]) -> Act:
        """ResBlock3D (models/unet3d.py:116-133): conv1 (+column sums) -> GN + SiLU + time bias in place -> conv2 ->
        silu(gn(c2) + residual), the residual being x itself or the 1x1x1 conv of [x | skip]."""
        cout = m.conv1.conv.out_channels
        has_res_conv = not isinstance(m.residual_conv, nn.Identity)
        if not has_res_conv and skip is not None:
            raise CtsiError("identity residual with a concatenated input")
        c1, st = self.conv("rb.conv1", lambda: m.conv1.conv.weight, lambda: m.conv1.conv.bias, x, skip, cout=cout,
                           want_stats=True)
        slot = self.gn_finalize(c1, m.conv1.norm.num_groups, st)
        c2, st = self.conv("rb.conv2", lambda: m.conv2[0].weight, lambda: m.conv2[0].bias, c1, None, cout=cout,
                           want_stats=True, norm_in=(slot, m.conv1.norm, True, (tbias, tbias_off, tbias_stride, step_ptr))
                           + ((True,) if getattr(m, "scale_shift", False) else ()))
        self.release(c1)
        slot = self.gn_finalize(c2, m.conv2[1].num_groups, st)
        if not has_res_conv:
            return self.gn_apply(c2, slot, m.conv2[1], silu_pre=False, residual=x, silu_post=True, out=c2)
        r, _ = self.conv("res1x1", lambda: m.residual_conv.weight, lambda: m.residual_conv.bias, x, skip, k=(1, 1, 1),
                         p=(0, 0, 0), cout=cout)
        out = self.gn_apply(c2, slot, m.conv2[1], silu_pre=False, residual=r, silu_post=True, out=c2)
        self.release(r)
        return out

    def attention(self, m, x: Act, mode: str = "fast") -> Act:
        """TemporalAttention, fast mode (csrc/attention.hip has the identity it rests on)."""
        if mode != "fast":
            raise CtsiError(f"the {self.precision} inference mode supports attention_mode='fast' only (the exact mode "
                            "evaluates the same mathematics, DESIGN section 3.2; the softmax mode has bf16 kernels only, "
                            "section 19)")
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
        tps = lib.attn_depthsum_f32_tiles(h, w)
        self._colsum_need = max(self._colsum_need, 2 * n * tps * c)
        depthsum = self.pool.get(n * h * w * c, torch.float32)
        xp, dsp = _ptr(x.t), _ptr(depthsum)

        def run_ds():
            lib.attn_depthsum_f32(xp, dsp, _ptr(prog._colsum), n, c, d, h, w, sptr)

        self._emit(run_ds, "attn.depthsum", nbytes=4.0 * n * c * d * h * w,
                   audit=dict(kind="attn_depthsum", f32=True, x=x, depthsum=depthsum, colsum=lambda: prog._colsum, tps=tps,
                              tile_pos=64))
        slot = self.gn_finalize(x, m.norm.num_groups, dict(tps=tps, cpad=c, nclass=1))
        gamma = self.dev_f32(lambda: m.norm.weight)
        beta = self.dev_f32(lambda: m.norm.bias)
        groups, eps = m.norm.num_groups, float(m.norm.eps)
        gp, bp = _ptr(gamma), _ptr(beta)
        xs = self.act(n, c, 1, h, w)
        xsp = _ptr(xs.t)

        def run_ns():
            lib.attn_normsum_f32(dsp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, xsp, n, c, d, h, w, groups,
                                 eps, sptr)

        self._emit(run_ns, "attn.normsum",
                   audit=dict(kind="attn_normsum", f32=True, depthsum=depthsum, sums=lambda: prog._gn_sums, slot=slot,
                              gamma=gamma, beta=beta, out=xs, groups=groups, eps=eps, d=d))

        # fold proj_out . V-projection in fp64, round once:  P = (Wp Wv) xs + (D Wp bv + bp)
        def wpv():
            wp = m.proj_out.weight[:, :, 0, 0, 0].double()
            return (wp @ m.qkv.weight[2 * c:3 * c, :, 0, 0, 0].double()).float().reshape(c, c, 1, 1, 1)

        def bpv():
            wp = m.proj_out.weight[:, :, 0, 0, 0].double()
            return (float(d) * (wp @ m.qkv.bias[2 * c:3 * c].double()) + m.proj_out.bias.double()).float()

        pterm, _ = self.conv("attn.pv", wpv, bpv, xs, None, k=(1, 1, 1), p=(0, 0, 0), cout=c)
        self.pool.put(depthsum)
        self.release(xs)
        out = self.act(n, c, d, h, w)
        pp, op_ = _ptr(pterm.t), _ptr(out.t)

        def run_ba():
            lib.attn_broadcast_add_f32(xp, pp, op_, n, c, d, h, w, sptr)

        self._emit(run_ba, "attn.broadcast_add", nbytes=12.0 * n * c * d * h * w,
                   audit=dict(kind="attn_broadcast_add", f32=True, x=x, p=pterm, rowsum=None, heads=m.num_heads, out=out))
        self.release(pterm)
        return out


# ==========================================================================================================
# U-Net
# ==========================================================================================================
class UNetProgramF32(_F32Ops, UNetProgram):
    """engine.UNetProgram in fp32.  The network input is two fp32 NDHWC tensors, z and the conditioning, fed to conv_in as
    a concatenated pair (never materialised)."""

    def __init__(self, ctx: Ctx, unet, n: int, d: int, h: int, w: int, max_rows: int, attention_mode="fast", shard=None,
                 guided: bool = False, rescale: bool = False, prediction: str = "epsilon"):
        if shard is not None:
            raise CtsiError(f"the {self.precision} inference mode does not support depth sharding")
        check_attention_mode(attention_mode)
        if attention_mode != "fast":
            raise CtsiError(f"the {self.precision} inference mode supports attention_mode='fast' only (the exact mode "
                            "evaluates the same mathematics, DESIGN section 3.2; the softmax mode has bf16 kernels only, "
                            "section 19)")
        super().__init__(ctx, unet, n, d, h, w, max_rows, attention_mode, shard=None, guided=guided, rescale=rescale,
                         prediction=prediction)

    def _input_acts(self, n, d, h, w, halo) -> Tuple[Act, Optional[Act]]:
        L = self.L
        zin = Act(self.persistent((n * d * h * w * L,), torch.float32, zero=True), n, L, d, h, w, 0)
        cin = Act(self.persistent((n * d * h * w * L,), torch.float32, zero=True), n, L, d, h, w, 0)
        return zin, cin

    def load_latents(self, z_ncdhw: Optional[torch.Tensor], cond_ncdhw: Optional[torch.Tensor]):
        lib, sptr = self.lib, self.ctx.sptr
        n, L, d, h, w = self.n, self.L, self.d, self.h, self.w
        if z_ncdhw is not None:
            z = z_ncdhw.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
            lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), _ptr(self.z), n, L, d, h, w, sptr)
            lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), _ptr(self.xin.t), n, L, d, h, w, sptr)
            if self.guided:     # both halves of z; rows [n, 2n) of the conditioning stay zero (the null conditioning)
                lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), self._uncond_zin(), n, L, d, h, w, sptr)
            z.record_stream(self.ctx.stream)
        if cond_ncdhw is not None:
            cnd = cond_ncdhw.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
            lib.ncdhw_f32_to_ndhwc_f32(_ptr(cnd), _ptr(self.xin2.t), n, L, d, h, w, sptr)
            cnd.record_stream(self.ctx.stream)

    def _sampler_zin(self):
        return _ptr(self.xin.t), self.L, 4, True


# ==========================================================================================================
# VAE
# ==========================================================================================================
class VAEEncodeProgramF32(_F32Ops, VAEEncodeProgram):
    """engine.VAEEncodeProgram in fp32: the same walk; the input volume keeps its own channel count."""

    def _input_act(self, n, c, d, h, w, halo) -> Tuple[Act, Optional[int]]:
        return Act(self.persistent((n * d * h * w * c,), torch.float32, zero=True), n, c, d, h, w), None

    def _upload(self, src: torch.Tensor, a: Act, c: int):
        self.lib.ncdhw_f32_to_ndhwc_f32(_ptr(src), _ptr(a.t), a.n, c, a.d, a.h, a.w, self.ctx.sptr)


class VAEDecodeProgramF32(VAEEncodeProgramF32, VAEDecodeProgram):
    """engine.VAEDecodeProgram in fp32 (one device; the tanh head stores fp32 NCDHW)."""

    def __init__(self, ctx: Ctx, vae, n, d, h, w, shard=None):
        if shard is not None:
            raise CtsiError(f"the {self.precision} inference mode does not support depth sharding")
        VAEDecodeProgram.__init__(self, ctx, vae, n, d, h, w)
