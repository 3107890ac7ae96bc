"""Training forward/backward of the VAE on the HIP engine: the backward of `SliceInterpolationVAE.forward`.

Reference: `training/train_vae.py` calls `recon, z = vae(x)` (models/vae.py:139-147, 190-204, 235-260), forms an MSE loss
(plus a mid-slice SSIM term that is a Python float) in torch and calls `backward()`.  One `VAETrainProgram` holds

  forward   the launches of engine.VAEEncodeProgram followed by those of engine.VAEDecodeProgram at the same shape (same
            plans, kernels and weight folding, private weight images), with every activation kept: `z` is bit for bit
            `encode(x)` and `recon` bit for bit `decode(z)`;
  backward  a tape of the forward layers replayed in reverse with train_engine.TrainProgram's conv / GroupNorm launches, plus
            ctsi_vae_head_grad (the tanh head, and grad_z at the latent seam) and ctsi_thin_wgrad (the one-channel stem and
            head weight gradients).

Scale folding: the forward packs scaling_factor * W_q into quant_conv and W_p / scaling_factor into post_quant_conv.  The
backward carries sf * dL/dz across the seam: post_quant's data gradient uses W_p as it is (= sf * its true dz), grad_z is
added with factor sf, and quant_conv's weight, bias and data gradients then need no factor at all; post_quant's weight
gradient takes 1 / sf through ctsi_wgrad's scale.

`vae_train_step` wraps both passes in a torch.autograd.Function over the VAE parameters (like train_engine._TrainStep), so
GradScaler, gradient accumulation, clip_grad_norm_ and any torch optimizer work unchanged.  The input gets no gradient.

`VAEDecodeGradProgram` is the opposite cut of the same tape: the decoder alone, differentiated with respect
to its INPUT and nothing else (`SliceInterpolationVAE.decode_with_grad`), for image-space loss terms of the diffusion stage.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch

from .engine import Act, Ctx, _pad8, _ptr
from .lib import CtsiError
from .train_engine import TrainProgram, _clone_grads


def check_trainable_geometry(vae, x: torch.Tensor):
    """Raise CtsiError for inputs the training program cannot differentiate (never a silently wrong backward)."""
    if not x.is_cuda:
        raise CtsiError("VAE training runs on the HIP engine: move the input to a ROCm device (there is no CPU path)")
    if x.dim() != 5:
        raise ValueError(f"forward expects a (B, C, T, H, W) tensor, got shape {tuple(x.shape)}")
    _, c, _, h, w = x.shape
    if c != vae.in_channels:
        raise ValueError(f"forward expects {vae.in_channels} input channels, got {c}")
    if h % 4 or w % 4:
        raise CtsiError(f"VAE training needs H and W that are multiples of 4 (got {h} x {w}): the backward of the stride-2 "
                        "stages assumes planes that they halve exactly.  Crop or pad the patch, or run forward under "
                        "torch.no_grad().")
    if vae.latent_dim % 8:
        raise CtsiError(f"VAE training needs latent_dim a multiple of 8 (got {vae.latent_dim})")
    for p in vae.parameters():
        if not p.is_cuda or p.device != x.device:
            raise CtsiError("VAE training runs on the HIP engine: the VAE's parameters must live on the input's ROCm device")


class VAETrainProgram(TrainProgram):
    stale_msg = ("backward of a VAE training forward whose saved activations were overwritten: another forward of the same "
                 "shape ran on this program in between (tape generation {then}, now {now}).  Call "
                 "backward() before the next training forward of that shape, or run the second batch under torch.no_grad().")

    def __init__(self, ctx: Ctx, vae, n: int, d: int, h: int, w: int):
        super().__init__(ctx, *self._trained(vae), workspaces=("wgrad", "gn", "chsum", "thin"))
        self.vae = vae
        self.n, self.d, self.h, self.w = n, d, h, w
        self.sf = float(vae.scaling_factor)
        self.L = vae.latent_dim
        # A/B: CTSI_VAE_THIN_WGRAD=0 = the MFMA wgrad on padded channels
        self.use_thin = not self.data_only and os.environ.get("CTSI_VAE_THIN_WGRAD", "1") != "0"
        self.zero_gn_op()
        self._emit_front()
        self._emit_decoder()
        self.finish_build()

    def _trained(self, vae):
        """(the module whose parameters take gradients, the floats of its gradient arena)"""
        return vae, sum(p.numel() for p in vae.parameters()) + (4 << 20)

    def _emit_front(self):
        """What precedes the decoder: the encoder (engine.VAEEncodeProgram), quant_conv and the seam into `zin`."""
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        vae, enc, n, d, h, w, L, sf = self.vae, self.vae.encoder, self.n, self.d, self.h, self.w, self.L, self.sf
        cin = vae.in_channels
        self.cin, self.cin_pad = cin, _pad8(cin)
        self.xin = Act(self.persistent((n * d * h * w * self.cin_pad,), torch.bfloat16, zero=True), n, self.cin_pad, d, h, w)
        x = self.conv_gn_act("enc.conv_in", enc.conv_in, self.xin, cin_w=cin, stem=True)
        for stage in (enc.down1, enc.down2):
            for m in stage:
                x = self.block(m, x)
        for m in enc.mid:
            x = self.block(m, x)
        y = self.v_conv("enc.conv_out", enc.conv_out, x)
        hl, wl = y.h, y.w
        self.hl, self.wl = hl, wl
        vox_l = d * hl * wl
        self.z = self.persistent((n, L, d, hl, wl), torch.float32)
        qc = enc.quant_conv
        qb = lambda: qc.bias * sf
        qb.parts, qb.scale = [lambda: qc.bias], sf        # (fast_repack: a scaled parameter view)
        self.conv("enc.quant", lambda: qc.weight * sf, qb, y, None, k=(1, 1, 1), p=(0, 0, 0), cout=L, f32_out=self.z,
                  f32_strides=(L * vox_l, vox_l, hl * wl, wl, 1))
        self.zin = Act(self.persistent((n * vox_l * L,), torch.bfloat16, zero=True), n, L, d, hl, wl)
        self.g_z = self.persistent(tuple(self.z.shape), torch.float32, zero=True)
        self.use_gz = False

        def quant_bwd():      # output gradient: sf * dL/dz, left in zin.grad by the seam (see the module docstring)
            g = prog.zin.grad
            prog._conv_bwd("enc.quant", qc.weight, qc.bias, y, None, g, False, (1, 1, 1), (1, 1), (0, 0, 0), L, True)
            prog.release(g)
            prog.zin.grad = None

        self.tape.append(quant_bwd)

        # ---- seam: z -> bf16 decoder input (engine.VAEDecodeProgram.load) ------------------------------------------------
        zp = self.zin.ip

        def run_seam():
            lib.ncdhw_f32_to_ndhwc_bf16(_ptr(prog.z), zp, n, L, d, hl, wl, L, 0, sptr)

        self._emit(run_seam, "seam.z_to_bf16", audit=dict(kind="seam.z_to_bf16", z=self.z, out=self.zin))

        def seam_bwd():       # runs after post_quant's backward wrote zin.grad = W_p^T du = sf * (its share of dL/dz)
            zg = prog.zin.grad

            def run_gz():
                if prog.use_gz:
                    lib.vae_head_grad(_ptr(prog.g_z), None, n, L, d, hl, wl, sf, 1, zg.ip, zg.c, sptr)

            prog._emit(run_gz, "seam.grad_z", audit=dict(kind="head_grad", mode=1, g=prog.g_z, y=None, scale=sf, out=zg,
                                                        active=lambda: prog.use_gz))

        self.tape.append(seam_bwd)

    def _emit_decoder(self):
        """The decoder (engine.VAEDecodeProgram) from `zin` to the fp32 `recon`, the end of the forward, and the head of the
        backward: ctsi_vae_head_grad from `g_recon` into `d_head`, the output gradient of conv_out.  A `data_only` program
        differentiates post_quant_conv with the folded weight the forward used (the seam's grad_z then is dL/dz itself)."""
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        dec, n, d, sf = self.vae.decoder, self.n, self.d, self.sf
        pq = dec.post_quant_conv
        pq_w = lambda: pq.weight * (1.0 / sf)
        u = self.v_conv("dec.post_quant", pq, self.zin, weight_fn=pq_w, k=(1, 1, 1), cin_w=self.L, w_scale=1.0 / sf,
                        dgrad_weight_fn=pq_w if self.data_only else None)
        x = self.conv_gn_act("dec.conv_in", dec.conv_in, u)
        for m in dec.mid:
            x = self.block(m, x)
        x = self.block(dec.up2_upsample, x)
        for m in dec.up2_res:
            x = self.block(m, x)
        x = self.block(dec.up3_upsample, x)
        for m in dec.up3_res:
            x = self.block(m, x)
        co = self.co = dec.conv_out.out_channels
        ho, wo = self.ho, self.wo = x.h, x.w
        vox = d * ho * wo
        self.recon = self.persistent((n, co, d, ho, wo), torch.float32)
        hp = self.d_head = Act(self.persistent((n * vox * _pad8(co),), torch.bfloat16, zero=True), n, _pad8(co), d, ho, wo)
        self.v_conv("dec.conv_out", dec.conv_out, x, f32_out=self.recon, f32_strides=(co * vox, vox, ho * wo, wo, 1), act=1,
                    gy=hp, thin_head=(co == 1))
        self.end_forward()
        self.g_recon = self.persistent(tuple(self.recon.shape), torch.float32, zero=True)

        def run_head():
            lib.vae_head_grad(_ptr(prog.g_recon), _ptr(prog.recon), n, co, d, ho, wo, 1.0, 0, hp.ip, hp.c, sptr)

        self._emit(run_head, "head.grad", audit=dict(kind="head_grad", mode=0, g=self.g_recon, y=self.recon, scale=1.0, out=hp,
                                                     active=None))

    # ---- layers --------------------------------------------------------------------------------------------------------------
    def v_conv(self, name, m, x1: Act, *, weight_fn=None, bias_fn=None, cin_w=None, k=(3, 3, 3), s=(1, 1),
               transposed=False, want_stats=False, bias_from_gn=False, need_dx=True, f32_out=None, f32_strides=None, act=0,
               gy: Optional[Act] = None, w_scale=1.0, stem=False, thin_head=False, dgrad_weight_fn=None):
        """One forward conv (the call engine.VAE*Program makes for this layer) and its backward on the tape.  In a `data_only`
        program the backward is the data gradient alone (`dgrad_weight_fn`: the weight it uses, when not the layer's own)."""
        p = (1, 1, 1) if k != (1, 1, 1) else (0, 0, 0)
        cout = m.out_channels
        out, st = self.conv(name, weight_fn or (lambda: m.weight), bias_fn or (lambda: m.bias), x1, None,
                            transposed=transposed, k=k, s=s, p=p, cout=cout, cin_w=cin_w, want_stats=want_stats,
                            f32_out=f32_out, f32_strides=f32_strides, act=act)
        # one-channel stem / head: the dedicated weight-gradient kernel (wide operand: output gradient / layer input)
        thin = (self.use_thin and ((stem and m.in_channels == 1) or (thin_head and cout == 1))
                and bool(self.lib.thin_wgrad_supported(cout if stem else x1.c, x1.w, *k)))
        gw_cin = None
        if stem and not thin and m.in_channels != x1.c:
            # the MFMA wgrad writes every (padded) input channel: a padded buffer, cut back to the weight on hand-over
            self.grads[id(m.weight)] = self.grad_alloc((cout, x1.c) + tuple(m.weight.shape[2:]))
            gw_cin = x1.c

        def bwd():
            g = gy if gy is not None else out.grad
            if g is None:
                raise CtsiError(f"internal: no gradient reached the output of {name}")
            self._conv_bwd(name, m.weight, None if (bias_from_gn or self.data_only) else m.bias, x1, None, g, transposed, k, s,
                           p, cout, need_dx and not stem, w_scale=w_scale, gw_cin=gw_cin,
                           emit_wgrad=not thin and not self.data_only, w_src=dgrad_weight_fn)
            if thin:
                self._thin_wgrad(name, m.weight, g, x1, head=not stem)
            if gy is None:
                self.release(out.grad)
                out.grad = None

        self.tape.append(bwd)
        return (out, st) if want_stats else out

    def _thin_wgrad(self, name, wparam, g: Act, x1: Act, head: bool):
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        if head:      # weight (1, C, 3, 3, 3): wide = layer input, thin = output gradient
            wide, thin, c = x1, g, x1.c
            gw = self.grad_buf(wparam, rows_pad=g.c if g.c > wparam.shape[0] else None)
        else:         # weight (C, 1, 3, 3, 3): wide = output gradient, thin = layer input
            wide, thin, c = g, x1, g.c
            gw = self.grad_buf(wparam)
        n, d, h, w = x1.n, x1.d, x1.h, x1.w
        self._need["thin"] = max(self._need["thin"], lib.thin_wgrad_workspace_bytes(n, c, d, h, w))
        wp, tp, tc, wc, dwp = wide.ip, thin.ip, thin.c, wide.c, _ptr(gw)
        fl = 2.0 * n * d * h * w * c * 27

        def run():
            lib.thin_wgrad(wp, c, wc, tp, tc, int(head), n, d, h, w, 3, 3, 3, prog._ws_ptr("thin"), prog._ws["thin"].numel(),
                           dwp, 1.0, sptr)

        self.flops += fl
        # audit: the weight gradient of R = conv3d(G, W) with R = output gradient, G = layer input (one channel of the thin one)
        if head:
            aud = dict(r=g, r_ch=1, g=x1, g_ch=c, out=gw[0:1].reshape(1, c, 27))
        else:
            aud = dict(r=g, r_ch=c, g=x1, g_ch=1, out=gw.reshape(c, 1, 27))
        self._emit(run, name + ".wgrad.thin", fl, "thin_wgrad",
                   audit=dict(aud, kind="wgrad", k=(3, 3, 3), s=(1, 1), p=(1, 1, 1), scale=1.0))

    def conv_gn_act(self, name, m, x: Act, *, cin_w=None, k=(3, 3, 3), s=(1, 1), transposed=False, stem=False) -> Act:
        c, st = self.v_conv(name, m.conv, x, cin_w=cin_w, k=k, s=s, transposed=transposed, want_stats=True,
                            bias_from_gn=True, stem=stem)
        slot = self.gn_finalize(c, m.norm.num_groups, st)
        return self.t_gn(c, slot, m.norm, silu_pre=True, conv_bias=self._gn_bias(m.conv))

    def _gn_bias(self, conv):
        """The conv bias whose gradient the following GroupNorm backward sums (none in a data-gradient-only program)."""
        return None if self.data_only else conv.bias

    def resblock(self, m, x: Act) -> Act:
        c1, st = self.v_conv("rb.conv1", m.conv1.conv, x, want_stats=True, bias_from_gn=True)
        slot = self.gn_finalize(c1, m.conv1.norm.num_groups, st)
        h1 = self.t_gn(c1, slot, m.conv1.norm, silu_pre=True, conv_bias=self._gn_bias(m.conv1.conv))
        c2, st = self.v_conv("rb.conv2", m.conv2[0], h1, want_stats=True, bias_from_gn=True)
        slot = self.gn_finalize(c2, m.conv2[1].num_groups, st)
        return self.t_gn(c2, slot, m.conv2[1], silu_pre=False, residual=x, silu_post=True,
                         conv_bias=self._gn_bias(m.conv2[0]))

    def block(self, m, x: Act) -> Act:
        kind = type(m).__name__
        if kind == "ResBlock3D":
            return self.resblock(m, x)
        if kind == "DownsampleBlock":
            return self.conv_gn_act("down", m, x, k=(3, 4, 4), s=(2, 2))
        if kind == "UpsampleBlock":
            return self.conv_gn_act("up", m, x, k=(3, 4, 4), s=(2, 2), transposed=True)
        raise CtsiError(f"unsupported VAE block {kind}")

    # ---- execution -----------------------------------------------------------------------------------------------------------
    def _load(self, src: torch.Tensor, a: Act, c: int):
        """fp32 NCDHW `src` of `c` channels into the bf16 input tensor `a`."""
        xx = src.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self.lib.ncdhw_f32_to_ndhwc_bf16(_ptr(xx), a.ip, a.n, c, a.d, a.h, a.w, a.c, 0, self.ctx.sptr)
        xx.record_stream(self.ctx.stream)

    def run_forward(self, x: torch.Tensor):
        """Forward launches; overwrites the saved activations (the generation counter makes a backward of an earlier forward
        of this shape fail loudly)."""
        self.forward_ops(lambda: self._load(x, self.xin, self.cin))
        recon, z = self.recon.clone(), self.z.clone()
        self.check_errors()
        return recon, z

    def run_backward(self, grad_recon: Optional[torch.Tensor], grad_z: Optional[torch.Tensor],
                     generation: Optional[int] = None) -> List[torch.Tensor]:
        def load():
            if grad_recon is None:
                self.g_recon.zero_()
            else:
                self.g_recon.copy_(grad_recon.reshape(self.g_recon.shape))
            self.use_gz = grad_z is not None
            if grad_z is not None:
                self.g_z.copy_(grad_z.reshape(self.g_z.shape))

        self.backward_ops(generation, load)
        self.check_errors()
        return self.param_grads()


class _VAETrainStep(torch.autograd.Function):
    """(recon, z) = SliceInterpolationVAE.forward(x); backward runs the engine's backward launches and hands the parameter
    gradients to autograd.  x gets no gradient."""

    @staticmethod
    def forward(fctx, prog: VAETrainProgram, x, *params):
        with prog.ctx.scope():
            recon, z = prog.run_forward(x)
        fctx.prog = prog
        fctx.generation = prog.generation
        fctx.set_materialize_grads(False)
        return recon, z

    @staticmethod
    def backward(fctx, grad_recon, grad_z):
        prog = fctx.prog
        with prog.ctx.scope():
            grads = _clone_grads(prog.run_backward(grad_recon, grad_z, fctx.generation))
        return (None, None) + tuple(grads)


def vae_train_step(prog: VAETrainProgram, x: torch.Tensor):
    return _VAETrainStep.apply(prog, x, *prog.params)


# ==== a differentiable decode of a FROZEN decoder =====================================================
def check_decode_grad_geometry(vae, z: torch.Tensor):
    """Raise CtsiError for latents the data-gradient program cannot differentiate (never a silently wrong backward)."""
    if not z.is_cuda:
        raise CtsiError("decode_with_grad runs on the HIP engine: move the latent to a ROCm device (there is no CPU path)")
    if z.dim() != 5:
        raise ValueError(f"decode expects a (B, C, T, H, W) tensor, got shape {tuple(z.shape)}")
    if z.shape[1] != vae.latent_dim:
        raise ValueError(f"decode expects {vae.latent_dim} latent channels, got {z.shape[1]}")
    if vae.latent_dim % 8:
        raise CtsiError(f"decode_with_grad needs latent_dim a multiple of 8 (got {vae.latent_dim})")
    for p in vae.decoder.parameters():
        if not p.is_cuda or p.device != z.device:
            raise CtsiError("decode_with_grad runs on the HIP engine: the decoder's parameters must live on the latent's ROCm "
                            "device")


class VAEDecodeGradProgram(VAETrainProgram):
    """decode(z) with the gradient for z and for nothing else: the decoder half of VAETrainProgram -- the launches of
    engine.VAEDecodeProgram at that shape, every activation kept, `recon` bit for bit `vae._decode(z, "bf16")` -- and a tape of
    DATA gradients only: ctsi_vae_head_grad mode 0 at the tanh head, the data-gradient conv of every layer (no weight gradient,
    no bias sum), ctsi_gn_bwd for dx (its dgamma / dbeta land in scratch nobody reads), and at the seam one layout pass back to
    fp32 NCDHW.  Scale folding: the forward packs W_p / sf into post_quant_conv; the data gradient uses the same W_p / sf, so
    the seam's grad_z already is dL/dz.  The decoder's parameters get no gradient and their requires_grad flags are not looked
    at.  The weights are frozen as far as this program is concerned, so it shares packed weight images with the inference
    programs (a changed parameter is still picked up: Program.ensure_fresh)."""
    data_only = True
    stale_msg = ("backward of a differentiable decode whose saved activations were overwritten: another decode_with_grad of the "
                 "same shape ran on this program in between (tape generation {then}, now {now}).  Call "
                 "backward() before the next decode_with_grad of that shape, or decode the second latent under torch.no_grad().")

    def _trained(self, vae):
        # (nothing is trained: the arena holds nothing but the dgamma / dbeta rows ctsi_gn_bwd insists on writing)
        norms = [m for m in vae.decoder.modules() if isinstance(m, torch.nn.GroupNorm)]
        return vae.decoder, sum(2 * ((m.num_channels + 63) // 64 * 64) for m in norms)

    def _emit_front(self):
        """The latent input `zin` ((h, w): the LATENT plane) and the seam's backward: one layout pass back to fp32 NCDHW."""
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        n, d, h, w, L = self.n, self.d, self.h, self.w, self.L
        self.hl, self.wl = h, w
        self.zin = Act(self.persistent((n * d * h * w * L,), torch.bfloat16, zero=True), n, L, d, h, w)
        self.g_z = self.persistent((n, L, d, h, w), torch.float32)

        def seam_bwd():       # runs after post_quant's data gradient wrote zin.grad = (W_p / sf)^T du = dL/dz, bf16 NDHWC
            zg = prog.zin.grad

            def run_gz():
                lib.ndhwc_bf16_to_ncdhw_f32(zg.ip, _ptr(prog.g_z), n, L, d, h, w, sptr)

            # a layout turn and a widening cast, checked bit for bit.  (A dict literal: this kind's reference is
            # tests/loss_audit.py's, not one of the two tables that tests/test_host_fwd_audit.py pins to the keyword-form
            # records of this file.)
            prog._emit(run_gz, "seam.grad_z", audit={"kind": "seam.grad_z", "g": zg, "out": prog.g_z})
            prog.release(zg)
            prog.zin.grad = None

        self.tape.append(seam_bwd)

    def run_forward(self, z: torch.Tensor) -> torch.Tensor:
        """Forward launches; overwrites the saved activations (the generation counter makes a backward of an earlier forward
        of this shape fail loudly)."""
        self.forward_ops(lambda: self._load(z, self.zin, self.L))
        recon = self.recon.clone()
        self.check_errors()
        return recon

    def run_backward(self, grad_recon: torch.Tensor, generation: Optional[int] = None) -> torch.Tensor:
        self.backward_ops(generation, lambda: self.g_recon.copy_(grad_recon.reshape(self.g_recon.shape)))
        self.check_errors()
        return self.g_z.clone()


class _VAEDecodeGrad(torch.autograd.Function):
    """recon = decode(z); backward runs the data-gradient launches and returns dL/dz.  No parameter is an input."""

    @staticmethod
    def forward(fctx, prog: VAEDecodeGradProgram, z):
        with prog.ctx.scope():
            recon = prog.run_forward(z)
        fctx.prog = prog
        fctx.generation = prog.generation
        fctx.z_dtype = z.dtype
        return recon

    @staticmethod
    def backward(fctx, grad_recon):
        prog = fctx.prog
        with prog.ctx.scope():
            g_z = prog.run_backward(grad_recon, fctx.generation)
        return None, g_z.to(fctx.z_dtype)


def vae_decode_grad_step(prog: VAEDecodeGradProgram, z: torch.Tensor) -> torch.Tensor:
    return _VAEDecodeGrad.apply(prog, z)
