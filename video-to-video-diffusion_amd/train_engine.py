"""Training forward/backward of the U-Net on the HIP engine.

Reference: `GaussianDiffusion.q_sample / training_loss` (models/diffusion.py:81-247) called from
`VideoToVideoDiffusion.forward` (models/model.py:158-228); the backward is what autograd derives from
models/unet3d.py.  Here one `UNetTrainProgram` holds the forward launches of engine.UNetProgram (without
buffer reuse: 288 GB of HBM keep every activation, so no recomputation / gradient checkpointing is needed) plus
the backward launches, built by replaying a tape of the forward layers in reverse:

  conv            dgrad = one of the *forward* conv kernels on re-laid-out weights (3^3 / 1^3: flipped + transposed;
                  strided Conv3d <-> ConvTranspose3d use each other's plans with the weights as they are),
                  wgrad = ctsi_wgrad (MFMA, transposing LDS reads), bias = ctsi_channel_sum
  GroupNorm chain ctsi_gn_bwd
  attention       the depth-sum form of engine.Program.attention, un-folded into its two 1x1x1 convs so that
                  proj_out / qkv(V) get their own gradients (the q and k thirds get exactly zero: rowsum(softmax) == 1);
                  attention_mode='softmax': the block of attention.py and ctsi_attn_core_bwd (all three thirds get gradients)
  time embedding  ctsi_linear_bwd

`train_step` wraps both passes in a torch.autograd.Function over the U-Net parameters, so `loss.backward()`,
GradScaler, gradient accumulation, clip_grad_norm_ and any torch optimizer work as with the reference.
`train_step_pred` is the same step with the predicted clean latent as a second differentiable output
(ctsi_z0_pred after the forward list; its gradient enters the loss launch through ctsi_loss_bwd_z0).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, Optional

import torch
import torch.nn as nn

from .attention import check_attention_mode, emit_softmax_attention_train
from .spatial_attention import check_spatial_attention_supported, emit_spatial_attention_train
from .engine import Act, Ctx, PhasedProgram, _ptr
from .lib import CtsiError, WgradDesc
from .norm_mod import DropoutState, emit_gn_bwd_mod
from .learned_sigma import emit_hybrid_loss, loss_schedule_rows
from .prediction import check_prediction_type


class TrainProgram(PhasedProgram):
    """Shared machinery of the training programs (U-Net here, VAE in vae_train_engine.py): the gradient arena, the conv and
    GroupNorm forward wrappers that record their backward on a tape, and the backward launches themselves."""
    tbias = None       # time-bias rows of the U-Net (programs without a time embedding leave these unset)
    total_out = 0
    data_only = False  # True: a backward of data gradients only (vae_train_engine.VAEDecodeGradProgram): no parameter buffers

    def __init__(self, ctx: Ctx, module: nn.Module, arena_floats: int, workspaces=("wgrad", "gn", "chsum")):
        """`module`: whose parameters the program differentiates (and watches: needs_rebuild, Program.track_module).  Every
        parameter-gradient buffer is a piece of ONE fp32 arena of `arena_floats`, so that the hand-over to autograd is one copy
        instead of one per parameter (333 launches, 1.6 ms of a config-3 micro-step); size it with slack for the row padding of
        the conv layouts.  `workspaces`: names of the byte workspaces the backward launches share (`_need` -> `_ws`)."""
        super().__init__(ctx)
        self.weight_cache = self.data_only    # trained weights change every optimizer step: private images, repacked in place
        self.tape: List[Callable[[], None]] = []
        self.grads: Dict[int, torch.Tensor] = {}     # id(param) -> fp32 gradient buffer (maybe padded)
        self._need = {key: 16 for key in workspaces}
        self._ws: Dict[str, Optional[torch.Tensor]] = {key: None for key in workspaces}
        self.params = list(module.parameters())
        self.track_module(module)
        self._garena = self.persistent((arena_floats,), torch.float32, zero=True)
        self._garena_used = 0

    def finish_build(self, before_layout: Optional[Callable[[], None]] = None):
        """Close the build after the head of the backward was emitted: the tape in reverse, `before_layout()` for launches that
        follow it, then the statistics buffers and the workspaces at the sizes the launches asked for."""
        for fn in reversed(self.tape):
            fn()
        if before_layout is not None:
            before_layout()
        self.finalize_layout()
        for key, need in self._need.items():
            self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.ctx.device)

    def needs_rebuild(self) -> bool:
        """The autograd bridge hands gradients to the Parameter objects captured at build time: a replaced
        parameter (load_state_dict(assign=True), module.weight = ...) needs a new program, not just a repack."""
        cur = list(self._track_module.parameters())
        return len(cur) != len(self.params) or any(a is not b for a, b in zip(cur, self.params))

    def param_grads(self) -> List[torch.Tensor]:
        """The gradient buffers in `params` order, each cut back from its padded layout to the parameter's own shape."""
        out = []
        for p in self.params:
            g = self.grads.get(id(p))
            if g is None:
                raise CtsiError("internal: a parameter received no gradient buffer")
            out.append(g if g.shape == p.shape else g[tuple(slice(0, s) for s in p.shape)])
        return out

    def _ws_ptr(self, key):
        return C.c_void_p(self._ws[key].data_ptr())

    # ---- helpers ---------------------------------------------------------------------------------------------
    def grad_alloc(self, shape) -> torch.Tensor:
        """A zeroed fp32 gradient buffer: a 256-byte-aligned piece of the arena (a separate allocation once the arena is full)."""
        numel = 1
        for v in shape:
            numel *= int(v)
        if self._garena_used + numel > self._garena.numel():
            return self.persistent(tuple(shape), torch.float32, zero=True)
        g = self._garena[self._garena_used:self._garena_used + numel].view(tuple(shape))
        self._garena_used += (numel + 63) // 64 * 64
        return g

    def grad_buf(self, p: torch.Tensor, rows_pad: Optional[int] = None) -> torch.Tensor:
        g = self.grads.get(id(p))
        if g is None:
            shape = list(p.shape)
            if rows_pad is not None and rows_pad > shape[0]:
                shape[0] = rows_pad
            g = self.grad_alloc(shape)
            self.grads[id(p)] = g
        return g

    def act_like(self, a: Act) -> Act:
        return self.act(a.n, a.c, a.d, a.h, a.w, halo=0)

    def into_grad(self, a: Act, produce: Callable[[Act], None]):
        """Run `produce(dst)` so that it writes a gradient contribution of `a`; the first contribution lands in
        a.grad directly, later ones go through a temporary and ctsi_add_bf16."""
        if a.grad is None:
            a.grad = self.act_like(a)
            produce(a.grad)
            return
        tmp = self.act_like(a)
        produce(tmp)
        lib, sptr = self.lib, self.ctx.sptr
        gp, tp, cnt = a.grad.ip, tmp.ip, a.n * a.vox * a.c

        def run():
            lib.add_bf16(gp, tp, cnt, sptr)

        self._emit(run, "grad.add", audit=dict(kind="add", dst=a.grad, src=tmp))
        self.release(tmp)

    # ---- conv ----------------------------------------------------------------------------------------------------
    def t_conv(self, name, m, x1: Act, x2: Optional[Act], *, transposed=False, k=(3, 3, 3), s=(1, 1), want_stats=False,
               need_dx=True, f32_out=None, f32_strides=None, gy: Optional[Act] = None, ret_stats=False,
               bias_from_gn=False):
        p = (1, 1, 1) if k != (1, 1, 1) else (0, 0, 0)
        cout = m.out_channels
        out, st = self.conv(name, lambda: m.weight, lambda: m.bias, x1, x2, transposed=transposed, k=k, s=s, p=p,
                            cout=cout, want_stats=want_stats, f32_out=f32_out, f32_strides=f32_strides)

        def bwd():
            g = gy if gy is not None else out.grad
            if g is None:
                raise CtsiError(f"internal: no gradient reached the output of {name}")
            self._conv_bwd(name, m.weight, None if bias_from_gn else m.bias, x1, x2, g, transposed, k, s, p, cout,
                           need_dx)
            if gy is None:
                self.release(out.grad)
                out.grad = None

        self.tape.append(bwd)
        return (out, st) if ret_stats else out

    def _conv_bwd(self, name, wparam, bparam, x1, x2, g: Act, transposed, k, s, p, cout, need_dx,
                  w_rows=None, b_scale=1.0, gw: Optional[torch.Tensor] = None, gb: Optional[torch.Tensor] = None,
                  gw_off=0, gb_off=0, w_src: Optional[Callable[[], torch.Tensor]] = None, defer_wb: bool = False,
                  w_scale: float = 1.0, gw_cin: Optional[int] = None, emit_wgrad: bool = True):
        """Emit bias / weight / data gradient launches of one conv whose output gradient is `g`.
        gw/gb (+ element offsets) override the destination (used for the V slice of attention's qkv);
        w_src overrides the weight the data gradient uses (same slice).  w_scale multiplies the weight gradient (a factor
        the forward folded into the weight image); gw_cin: input channels per row of a Conv3d weight-gradient buffer padded
        beyond the weight's own (a thin input whose padded channels the wgrad kernel also writes); emit_wgrad False: the
        caller emits the weight gradient itself."""
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        T = k[0] * k[1] * k[2]
        cin = x1.c + (0 if x2 is None else x2.c)
        cw_out = wparam.shape[1] if transposed else wparam.shape[0]
        if gw is None and not self.data_only:
            pad = g.c if (not transposed and g.c > wparam.shape[0]) else None
            gw = self.grad_buf(wparam, rows_pad=pad)
        if gb is None and bparam is not None:
            gb = self.grad_buf(bparam, rows_pad=g.c if g.c > bparam.shape[0] else None)
        rows = g.n * g.vox
        if defer_wb:
            # a small 1x1x1 layer (rows of a depth-summed tensor): weight and bias gradient join the batched launch at the end of
            # the backward pass (ctsi_linear_wgrad_multi); x1 and g must stay alive until then
            if transposed or T != 1 or x2 is not None:
                raise CtsiError("internal: only plain pointwise layers can defer their weight gradient")
            self._deferred_lin.append((x1, g, gw, gw_off, gb, gb_off, float(b_scale), rows, x1.c, g.c, wparam.shape[1]))
        # bias: channel sums of the output gradient
        if gb is not None and not defer_wb:
            self._need["chsum"] = max(self._need["chsum"], 4 * lib.channel_sum_workspace_floats(rows, g.c))
            gp, gbp, gc = g.ip, C.c_void_p(gb.data_ptr() + 4 * gb_off), g.c

            def run_b():
                lib.channel_sum(gp, rows, gc, gc, prog._ws_ptr("chsum"), gbp, b_scale, sptr)

            self._emit(run_b, name + ".bgrad", audit=dict(kind="chsum", src=g, out=gb[gb_off:gb_off + gc], scale=float(b_scale)))
        # weight
        srcs = [(x1, 0)] + ([(x2, x1.c)] if x2 is not None else [])
        for xa, coff in ([] if (defer_wb or not emit_wgrad) else srcs):
            if transposed:   # weight (cin, cout, T): R = layer input, G = output gradient
                r_act, g_act = xa, g
                sr, sg = cw_out * T, T
                off = gw_off + coff * cw_out * T
            else:            # weight (cout, cin, T): R = output gradient, G = layer input
                r_act, g_act = g, xa
                sr, sg = (gw_cin or wparam.shape[1]) * T, T
                off = gw_off + coff * T
            desc = WgradDesc(k[0], k[1], k[2], s[0], s[1], p[0], p[1], p[2], r_act.n, r_act.d, r_act.h, r_act.w,
                             g_act.d, g_act.h, g_act.w, r_act.c, r_act.c, g_act.c, g_act.c)
            self.keep.append(desc)
            self._need["wgrad"] = max(self._need["wgrad"], lib.wgrad_workspace_bytes(C.byref(desc)))
            fl = lib.wgrad_flops(C.byref(desc))
            self.flops += fl
            rp, gp2, dwp = r_act.ip, g_act.ip, C.c_void_p(gw.data_ptr() + 4 * off)

            def run_w(desc=desc, rp=rp, gp2=gp2, dwp=dwp, sr=sr, sg=sg):
                lib.wgrad(C.byref(desc), rp, gp2, prog._ws_ptr("wgrad"), prog._ws["wgrad"].numel(), dwp, sr, sg, 1, w_scale, sptr)

            # audit: dW[r, g, t] of the conv R = conv3d(G, W) lands at dwp + r * sr + g * sg + t
            dst = gw.as_strided((r_act.c, g_act.c, T), (sr, sg, 1), gw.storage_offset() + off)
            self._emit(run_w, name + ".wgrad", fl, "conv_wgrad",
                       audit=dict(kind="wgrad", r=r_act, r_ch=r_act.c, g=g_act, g_ch=g_act.c, k=k, s=s, p=p, out=dst,
                                  scale=float(w_scale)))
        # data
        if not need_dx:
            return
        if transposed:      # ConvTranspose3d layer: dx = strided Conv3d of g with the same weight tensor
            self.into_grad(x1, lambda dst: self.conv(name + ".dgrad", lambda: wparam, None, g, None, k=k, s=s, p=p,
                                                     cout=x1.c, out=dst,
                                                     audit=dict(kind="dgrad", op="conv", g=g, weight=lambda: wparam,
                                                                w_ci=None, k=k, s=s, p=p)))
        elif s != (1, 1):   # strided Conv3d layer: dx = ConvTranspose3d of g with the same weight tensor
            self.into_grad(x1, lambda dst: self.conv(name + ".dgrad", lambda: wparam, None, g, None, transposed=True,
                                                     k=k, s=s, p=p, cout=x1.c, out=dst,
                                                     audit=dict(kind="dgrad", op="convT", g=g, weight=lambda: wparam,
                                                                w_ci=None, k=k, s=s, p=p)))
        else:               # stride-1 'same' conv: flipped, transposed weights, one launch per concatenated source
            co_w, ci_w = wparam.shape[0], wparam.shape[1]
            if w_src is not None:
                co_w = cout
            for xa, coff in srcs:
                def wfn(coff=coff, cnt=xa.c):
                    src = (w_src() if w_src is not None else wparam).detach().contiguous()
                    outw = torch.empty((cnt, co_w) + tuple(wparam.shape[2:]), dtype=torch.float32,
                                       device=self.ctx.device)
                    lib.weight_dgrad_layout(_ptr(src), _ptr(outw), co_w, ci_w, T, coff, cnt, sptr)
                    src.record_stream(self.ctx.stream)
                    return outw

                # (fast_repack: the same re-layout from a pointer table, into a buffer the program keeps)
                wfn.fast_layout = ((w_src if w_src is not None else (lambda: wparam)), co_w, ci_w, T, coff, xa.c)

                # audit: dx = conv_transpose3d(g, W[:co_w, coff:coff + cnt]) with the layer's own weight
                aud = dict(kind="dgrad", op="convT", g=g, weight=(w_src if w_src is not None else (lambda: wparam)),
                           w_ci=(coff, xa.c), k=k, s=(1, 1), p=p)
                self.into_grad(xa, lambda dst, wfn=wfn, cnt=xa.c, aud=aud: self.conv(
                    name + ".dgrad", wfn, None, g, None, k=k, s=(1, 1), p=p, cout=cnt, out=dst,
                    cin_w=(co_w if co_w != g.c else None), audit=aud))

    # ---- GroupNorm chain ---------------------------------------------------------------------------------------------
    def t_gn(self, x: Act, slot: int, gn: nn.GroupNorm, *, silu_pre: bool, tb_off: Optional[int] = None,
             residual: Optional[Act] = None, silu_post: bool = False, conv_bias: Optional[torch.Tensor] = None,
             film: bool = False, drop=None) -> Act:
        """`conv_bias`: bias parameter of the convolution that produced x; its gradient (sum of dx) then comes out of
        the GroupNorm backward's statistics and that conv's backward skips its own channel-sum pass.
        `film` / `drop` = (norm_mod.DropoutState, layer_id): the ResBlock's middle pass in its scale-shift / dropout forms
        (engine.Program.gn_apply); forward and backward then go to ctsi_gn_apply_mod / ctsi_gn_bwd_mod."""
        mod = dict(film=film, drop=drop) if (film or drop is not None) else {}
        out = self.gn_apply(x, slot, gn, silu_pre=silu_pre, tbias=self.tbias if tb_off is not None else None,
                            tbias_off=tb_off or 0, tbias_stride=self.total_out, residual=residual, silu_post=silu_post,
                            **mod)
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        gamma = self.dev_f32(lambda: gn.weight)
        beta = self.dev_f32(lambda: gn.bias)

        def bwd():
            gy = out.grad
            if gy is None:
                raise CtsiError("internal: no gradient reached a GroupNorm output")
            dxsum = None if conv_bias is None else self.grad_buf(conv_bias)
            if mod:
                emit_gn_bwd_mod(self, x, gy, slot, gn, gamma, beta, tb_off, film, drop, dxsum)
            else:
                self._gn_bwd(x, gy, False, slot, gn, gamma, beta, silu_pre, tb_off, residual, silu_post, None, dxsum=dxsum)
            self.release(gy)
            out.grad = None

        self.tape.append(bwd)
        return out

    def _gn_bwd(self, x: Act, gy: Act, bcast: bool, slot: int, gn, gamma, beta, silu_pre, tb_off, residual, silu_post,
                add: Optional[Act], dxsum: Optional[torch.Tensor] = None):
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
        groups, eps = gn.num_groups, float(gn.eps)
        self._need["gn"] = max(self._need["gn"], 4 * lib.gn_bwd_workspace_floats(n, c, d, h, w, groups))
        if x.grad is not None:
            raise CtsiError("internal: a normalised tensor has a second consumer")
        x.grad = self.act_like(x)
        # g_buf (gradient of the GroupNorm output) is the residual's gradient when no SiLU sits in between
        tmp = None
        if residual is not None and not silu_pre and residual.grad is None:
            residual.grad = self.act_like(residual)
            gbuf = residual.grad
            add_to_res = False
        elif residual is None and not silu_post:
            gbuf = None         # nobody but pass 3 needs the GroupNorm output's gradient: it re-derives it from dy (no buffer, no write)
            add_to_res = False
        else:
            tmp = self.act_like(x)
            gbuf = tmp
            add_to_res = residual is not None
        if residual is not None and silu_pre:
            raise CtsiError("internal: residual after a pre-SiLU is not a combination the U-Net uses")
        dgam, dbet = self.grad_buf(gn.weight), self.grad_buf(gn.bias)
        xp, gyp, gp, bp = x.ip, gy.ip, _ptr(gamma), _ptr(beta)
        rp = C.c_void_p(0) if residual is None else residual.ip
        ap = C.c_void_p(0) if add is None else add.ip
        gbp, dxp, dgp, dbp = (C.c_void_p(0) if gbuf is None else gbuf.ip), x.grad.ip, _ptr(dgam), _ptr(dbet)
        dtp = C.c_void_p(0 if tb_off is None else self.d_tbias.data_ptr() + 4 * tb_off)
        tstride = self.total_out
        dxsp = _ptr(dxsum)

        def run():
            lib.gn_bwd(xp, gyp, int(bcast), C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, n, c, d, h, w,
                       groups, eps, int(silu_pre), rp, int(silu_post), ap, gbp, dxp, prog._ws_ptr("gn"), dgp, dbp, dtp,
                       tstride, dxsp, sptr)

        nsum = n * groups * 2
        self._emit(run, "gn.bwd", audit=dict(
            kind="gn_bwd", x=x, dy=gy, bcast=bool(bcast), sums=lambda: prog._gn_sums[slot:slot + nsum], gamma=gamma, beta=beta,
            groups=groups, eps=eps, silu_pre=bool(silu_pre), residual=residual, silu_post=bool(silu_post), add=add, g_out=gbuf,
            dx=x.grad, dgamma=dgam, dbeta=dbet, dxsum=dxsum,
            dtbias=None if tb_off is None else self.d_tbias[:, tb_off:tb_off + c]))
        if add_to_res:
            rgp, cnt = residual.grad.ip, n * x.vox * c

            def run_add():
                lib.add_bf16(rgp, gbp, cnt, sptr)

            self._emit(run_add, "grad.add", audit=dict(kind="add", dst=residual.grad, src=gbuf))
        if tmp is not None:
            self.release(tmp)


class UNetTrainProgram(TrainProgram):
    stale_msg = ("backward of a training forward whose saved activations were overwritten: another forward of the same "
                 "shape ran on this program in between (tape generation {then}, now {now}).  Call "
                 "backward() before the next forward of that shape, or evaluate the second batch under torch.no_grad() "
                 "through model.generate / unet(x, t, c), which do not touch the training tape.")

    def __init__(self, ctx: Ctx, unet, n: int, d: int, h: int, w: int, prediction: str = "epsilon", dropout: bool = False):
        """`prediction` = 'v_prediction' (DESIGN section 18): the inputs come from ctsi_q_sample_v, which also writes the
        target v into `v_target`, and both loss launches read that buffer where the epsilon program reads the noise.
        `dropout`: the ResBlocks' middle passes are the dropout launches; the probability and the seed
        are set per forward (`set_dropout`).  The scale-shift mode is the module tree's (`unet.use_scale_shift_norm`).
        A `unet.learn_sigma` model: the head, its weight gradient and its data gradient are 2L channels wide
        (`eps` then holds both halves, `d_eps` both gradients), and the loss pair is ctsi_hybrid_loss_fwd / _bwd, which read
        z0, the noise and the per-timestep rows `lv_sched` (set_diffusion) instead of a target buffer."""
        super().__init__(ctx, unet, sum(p.numel() for p in unet.parameters()) + (16 << 20))
        self.learn_sigma = bool(getattr(unet, "learn_sigma", False))
        self.film = bool(getattr(unet, "use_scale_shift_norm", False))
        self.drop_state = DropoutState(self.persistent((1,), torch.int64, zero=True)) if dropout else None
        self.prediction = check_prediction_type(prediction)
        self.attention_mode = check_attention_mode(unet.attention_mode)
        if self.attention_mode == "exact":
            raise CtsiError("training supports attention_mode='fast' and 'softmax' (the exact mode multiplies in a row sum "
                            "that is 1: its gradient is the fast mode's)")
        self.unet = unet
        self.n, self.d, self.h, self.w = n, d, h, w
        L = unet.latent_dim
        self.L = L
        Lo = self.Lo = 2 * L if self.learn_sigma else L        # channels of the head
        if unet.conv_out[2].out_channels != Lo:
            raise CtsiError(f"internal: the head has {unet.conv_out[2].out_channels} channels, expected {Lo}")
        self.Lp = (Lo + 7) // 8 * 8
        vox = d * h * w
        self._deferred_lin: List[tuple] = []     # small pointwise layers whose weight / bias gradients go into ONE launch at the end
        for p in self.params:
            if not p.is_cuda:
                raise CtsiError("training runs on the HIP engine: move the model to a ROCm device first")

        # ---- inputs ------------------------------------------------------------------------------------
        self.xin = Act(self.persistent((n * vox * 2 * L,), torch.bfloat16, zero=True), n, 2 * L, d, h, w, 0)
        self.z0 = self.persistent((n, L, d, h, w), torch.float32, zero=True)
        self.noise = self.persistent((n, L, d, h, w), torch.float32, zero=True)
        v_pred = self.prediction == "v_prediction"
        self.v_target = self.persistent((n, L, d, h, w), torch.float32, zero=True) if v_pred else None
        self.target = self.v_target if v_pred else self.noise      # what the prediction is compared with
        self.cond = self.persistent((n, L, d, h, w), torch.float32, zero=True)
        self.t_rows = self.persistent((n,), torch.int32, zero=True)
        self.norm = self.persistent((n,), torch.float32, zero=True)
        self.mask = self.persistent((n, L, d), torch.float32, zero=True)
        self.use_mask = False
        self.gscale = self.persistent((1,), torch.float32, zero=True)
        self.eps = self.persistent((n, d, h, w, Lo), torch.float32)
        if self.learn_sigma:      # {total, mse, vb, per-sample sums of the two terms}
            self.loss_out = self.persistent((3 + 2 * n,), torch.float32, zero=True)
            self.loss_ws = self.persistent((self.lib.hybrid_loss_workspace_doubles(n),), torch.float64)
            self.norm_vb = self.persistent((n,), torch.float32, zero=True)
            self.lv_sched = self.persistent((1, 8), torch.float32)      # replaced by set_diffusion()
        else:
            self.loss_out = self.persistent((1 + n,), torch.float32, zero=True)
            self.loss_ws = self.persistent((self.lib.mse_loss_workspace_doubles(n),), torch.float64)
        self.sqrt_ac = self.persistent((1,), torch.float32)      # replaced by set_diffusion()
        self.sqrt_1mac = self.persistent((1,), torch.float32)

        # ---- time embedding --------------------------------------------------------------------------------
        te = unet.time_embed.time_mlp
        self.dim = unet.model_channels
        self.time_dim = te[1].out_features
        self.blocks = [m for m in unet.modules() if type(m).__name__ == "ResBlock3D"]
        self.tb_off = {}
        off = 0
        for m in self.blocks:
            self.tb_off[id(m)] = off
            off += m.time_mlp[1].out_features
        self.total_out = off
        # the dropout layer ids: a ResBlock's ordinal in unet.modules() order, the enumeration of tb_off
        names = {id(m): name for name, m in unet.named_modules()}
        self.layer_id = {id(m): i for i, m in enumerate(self.blocks)}
        self.dropout_layers = [(names[id(m)], i, m.conv1.conv.out_channels) for i, m in enumerate(self.blocks)]
        self.w1 = self.dev_f32(lambda: te[1].weight)
        self.b1 = self.dev_f32(lambda: te[1].bias)
        self.w2 = self.dev_f32(lambda: te[3].weight)
        self.b2 = self.dev_f32(lambda: te[3].bias)
        self.w_all = self.dev_f32(lambda: torch.cat([m.time_mlp[1].weight for m in self.blocks], 0),
                                  parts=[(lambda m=m: m.time_mlp[1].weight) for m in self.blocks])
        self.b_all = self.dev_f32(lambda: torch.cat([m.time_mlp[1].bias for m in self.blocks], 0),
                                  parts=[(lambda m=m: m.time_mlp[1].bias) for m in self.blocks])
        self.tbias = self.persistent((n, self.total_out), torch.float32, zero=True)
        self.d_tbias = self.persistent((n, self.total_out), torch.float32, zero=True)
        self.te_scratch = self.persistent((n * (self.dim + 2 * self.time_dim),), torch.float32)
        self.g_w_all = self.grad_alloc((self.total_out, self.time_dim))
        self.g_b_all = self.grad_alloc((self.total_out,))
        self.g_temb = self.persistent((n, self.time_dim), torch.float32, zero=True)
        self.g_lin1 = self.persistent((n, self.time_dim), torch.float32, zero=True)

        lib, sptr = self.lib, ctx.sptr
        prog = self

        def run_inputs():
            if v_pred:
                lib.q_sample_v(_ptr(prog.z0), _ptr(prog.noise), _ptr(prog.sqrt_ac), _ptr(prog.sqrt_1mac),
                               _ptr(prog.t_rows), prog.xin.ip, _ptr(prog.v_target), n, L, d, h, w, 2 * L, 0, sptr)
            else:
                lib.q_sample(_ptr(prog.z0), _ptr(prog.noise), _ptr(prog.sqrt_ac), _ptr(prog.sqrt_1mac),
                             _ptr(prog.t_rows), prog.xin.ip, n, L, d, h, w, 2 * L, 0, sptr)
            lib.ncdhw_f32_to_ndhwc_bf16(_ptr(prog.cond), prog.xin.ip, n, L, d, h, w, 2 * L, L, sptr)
            lib.time_embed_train_fwd(_ptr(prog.t_rows), n, prog.dim, prog.time_dim, _ptr(prog.w1), _ptr(prog.b1),
                                     _ptr(prog.w2), _ptr(prog.b2), _ptr(prog.w_all), _ptr(prog.b_all), prog.total_out,
                                     _ptr(prog.te_scratch), _ptr(prog.tbias), sptr)

        self._emit(run_inputs, "train.inputs", audit=dict(
            kind="train.inputs", z0=self.z0, noise=self.noise, cond=self.cond, t_rows=self.t_rows,
            sqrt_ac=lambda: prog.sqrt_ac, sqrt_1mac=lambda: prog.sqrt_1mac, xin=self.xin, L=L, dim=self.dim,
            time_dim=self.time_dim, w1=self.w1, b1=self.b1, w2=self.w2, b2=self.b2, w_all=self.w_all, b_all=self.b_all,
            te_scratch=self.te_scratch, tbias=self.tbias,
            **(dict(kernel="q_sample_v", v_target=self.v_target) if v_pred else {})))
        self.zero_gn_op()

        # ---- forward network (same wiring as engine.UNetProgram) -------------------------------------------------
        x = self.t_conv("conv_in", unet.conv_in, self.xin, None, need_dx=False)
        skips: List[Act] = []
        for level_blocks, down in zip(unet.down_blocks, unet.down_samples):
            for block_list in level_blocks:
                for layer in block_list:
                    x = self._layer(layer, x, None)
            skips.append(x)
            if not isinstance(down, nn.Identity):
                x = self.t_conv("down", down.conv, x, None, k=(3, 4, 4), s=(2, 2))
        x = self._layer(unet.mid_block1, x, None)
        x = self._layer(unet.mid_attn, x, None)
        if hasattr(unet, "mid_attn_spatial"):
            x = self._layer(unet.mid_attn_spatial, x, None)
        x = self._layer(unet.mid_block2, x, None)
        for level_blocks, up in zip(unet.up_blocks, unet.up_samples):
            for j, block_list in enumerate(level_blocks):
                skip = skips.pop() if j == 0 else None
                for layer in block_list:
                    x = self._layer(layer, x, skip)
                    skip = None
            if not isinstance(up, nn.Identity):
                x = self.t_conv("up", up.conv, x, None, transposed=True, k=(3, 4, 4), s=(2, 2))
        gn, conv = unet.conv_out[0], unet.conv_out[2]
        st = self.gn_colsum(x)
        slot = self.gn_finalize(x, gn.num_groups, st)
        y = self.t_gn(x, slot, gn, silu_pre=True)
        self.d_eps = Act(self.persistent((n * vox * self.Lp,), torch.bfloat16, zero=True), n, self.Lp, d, h, w, 0)
        self.t_conv("conv_out", conv, y, None, f32_out=self.eps, f32_strides=(vox * Lo, 1, h * w * Lo, w * Lo, Lo),
                    gy=self.d_eps)

        def run_loss():
            lib.mse_loss_fwd(_ptr(prog.eps), _ptr(prog.target), _ptr(prog.mask) if prog.use_mask else None,
                             _ptr(prog.norm), n, L, d, h, w, _ptr(prog.loss_ws), _ptr(prog.loss_out), sptr)

        if self.learn_sigma:
            emit_hybrid_loss(self, backward=False)
        else:
            self._emit(run_loss, "loss.fwd", audit=dict(
                kind="loss.fwd", pred=self.eps, noise=self.target, mask=lambda: prog.mask if prog.use_mask else None,
                norm=self.norm, out=self.loss_out))
        self.end_forward()

        # ---- backward: loss, then the tape in reverse, then the time embedding ---------------------------------
        # the predicted clean latent as a second output (train_step_pred): buffers made on first use, the
        # gradient that came back through it enters the loss launch below
        self.z0_hat = self.g_z0 = self.active = self.coef = None
        self.use_gz0 = False

        def run_loss_bwd():
            if prog.use_gz0:      # ctsi_mse_loss_bwd's expression + active coef g_z0, rounded once
                lib.loss_bwd_z0(_ptr(prog.eps), _ptr(prog.target), _ptr(prog.mask) if prog.use_mask else None,
                                _ptr(prog.norm), _ptr(prog.gscale), _ptr(prog.g_z0), _ptr(prog.active), _ptr(prog.coef),
                                n, L, d, h, w, prog.d_eps.ip, prog.Lp, sptr)
                return
            lib.mse_loss_bwd(_ptr(prog.eps), _ptr(prog.target), _ptr(prog.mask) if prog.use_mask else None,
                             _ptr(prog.norm), _ptr(prog.gscale), n, L, d, h, w, prog.d_eps.ip, prog.Lp, sptr)

        if self.learn_sigma:
            emit_hybrid_loss(self, backward=True)
        else:
            self._emit(run_loss_bwd, "loss.bwd", audit=dict(
                kind="loss_bwd", pred=self.eps, noise=self.target, mask=lambda: prog.mask if prog.use_mask else None,
                norm=self.norm, gscale=self.gscale, out=self.d_eps))

        def tail():
            self._emit_deferred_lin()
            self._time_embed_bwd()

        self.finish_build(tail)

    def _emit_deferred_lin(self):
        """ONE launch for the weight and bias gradients of every deferred pointwise layer (the 22 attention projections):
        device tables of layers and of 64 x 64 dW tiles, built once."""
        import struct
        if not self._deferred_lin:
            return
        ents, blks, fl = [], [], 0.0
        for i, (xa, ga, gw, gw_off, gb, gb_off, b_scale, rows, cin, cout, dw_stride) in enumerate(self._deferred_lin):
            dbp = 0 if gb is None else gb.data_ptr() + 4 * gb_off
            ents.append(struct.pack("<QQQQiiiifi", xa.ip.value, ga.ip.value, gw.data_ptr() + 4 * gw_off, dbp, rows, cin, cout,
                                    dw_stride, b_scale, 0))
            for ct in range((cout + 63) // 64):
                for it in range((cin + 63) // 64):
                    blks.append(struct.pack("<iiii", i, ct, it, 0))
            fl += 2.0 * rows * cin * cout
        dev = self.ctx.device
        et = torch.frombuffer(bytearray(b"".join(ents)), dtype=torch.uint8).to(dev)
        bt = torch.frombuffer(bytearray(b"".join(blks)), dtype=torch.uint8).to(dev)
        self._lin_tables = (et, bt)      # host-built tables (uploaded whole): kept alive here; `keep` lists the program's own allocations
        lib, sptr, nb = self.lib, self.ctx.sptr, len(blks)

        def run():
            lib.linear_wgrad_multi(_ptr(et), _ptr(bt), nb, sptr)

        self.flops += fl
        layers = [dict(x=xa, g=ga, dw=gw.as_strided((cout, cin), (dw_stride, 1), gw.storage_offset() + gw_off),
                       db=None if gb is None else gb[gb_off:gb_off + cout], scale=b_scale)
                  for (xa, ga, gw, gw_off, gb, gb_off, b_scale, rows, cin, cout, dw_stride) in self._deferred_lin]
        self._emit(run, "attn.wgrad+bgrad.batched", fl, "linear_wgrad_multi",
                   audit=dict(kind="linear_wgrad_multi", layers=layers))
        for (xa, ga, *_rest) in self._deferred_lin:
            self.release(ga)

    def _layer(self, layer, x: Act, skip: Optional[Act]) -> Act:
        kind = type(layer).__name__
        if kind == "ResBlock3D":
            y = self.t_resblock(layer, x, skip)
        elif kind == "TemporalAttention":
            y = self.t_attention_softmax(layer, x) if self.attention_mode == "softmax" else self.t_attention(layer, x)
        elif kind == "SpatialAttention":
            y = emit_spatial_attention_train(self, layer, x)
        else:
            raise CtsiError(f"unsupported U-Net layer {kind}")
        return y

    # ---- ResBlock3D (models/unet3d.py:116-133) ------------------------------------------------------------------------
    def t_resblock(self, m, x: Act, skip: Optional[Act]) -> Act:
        if isinstance(m.residual_conv, nn.Identity):
            if skip is not None:
                raise CtsiError("identity residual with a concatenated input")
            r = x
        else:
            r = self.t_conv("res1x1", m.residual_conv, x, skip, k=(1, 1, 1))
        c1, st = self.t_conv("rb.conv1", m.conv1.conv, x, skip, want_stats=True, ret_stats=True, bias_from_gn=True)
        slot = self.gn_finalize(c1, m.conv1.norm.num_groups, st)
        h1 = self.t_gn(c1, slot, m.conv1.norm, silu_pre=True, tb_off=self.tb_off[id(m)], conv_bias=m.conv1.conv.bias,
                       film=self.film, drop=None if self.drop_state is None else (self.drop_state, self.layer_id[id(m)]))
        c2, st = self.t_conv("rb.conv2", m.conv2[0], h1, None, want_stats=True, ret_stats=True, bias_from_gn=True)
        slot = self.gn_finalize(c2, m.conv2[1].num_groups, st)
        out = self.t_gn(c2, slot, m.conv2[1], silu_pre=False, residual=r, silu_post=True, conv_bias=m.conv2[0].bias)
        return out

    # ---- TemporalAttention in its depth-sum form (see engine.Program.attention) ---------------------------------------------
    def t_attention(self, m, x: Act) -> Act:
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
        tps = lib.attn_depthsum_tiles(c, h, w)
        self._colsum_need = max(self._colsum_need, 2 * n * tps * c)
        depthsum = self.persistent((n * h * w * c,), torch.float32)
        xp, dsp = x.ip, _ptr(depthsum)

        def run_ds():
            lib.attn_depthsum(xp, dsp, _ptr(prog._colsum), n, c, d, h, w, sptr)

        self._emit(run_ds, "attn.depthsum", audit=dict(kind="attn_depthsum", x=x, depthsum=depthsum,
                                                       colsum=lambda: prog._colsum, tps=tps, tile_pos=256 // (c // 8)))
        slot = self.gn_finalize(x, m.norm.num_groups, dict(tps=tps, cpad=c, nclass=1))
        gamma = self.dev_f32(lambda: m.norm.weight)
        beta = self.dev_f32(lambda: m.norm.bias)
        xs = self.act(n, c, 1, h, w, halo=0)
        groups, eps = m.norm.num_groups, float(m.norm.eps)
        gp, bp, xsp = _ptr(gamma), _ptr(beta), xs.ip

        def run_ns():
            lib.attn_normsum(dsp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, xsp, n, c, d, h, w, groups,
                             eps, sptr)

        self._emit(run_ns, "attn.normsum", audit=dict(kind="attn_normsum", depthsum=depthsum, sums=lambda: prog._gn_sums,
                                                      slot=slot, gamma=gamma, beta=beta, out=xs, groups=groups, eps=eps, d=d))
        wv = lambda: m.qkv.weight[2 * c:3 * c]
        def bv():                      # the V bias is added once per depth slice of the sum
            return float(d) * m.qkv.bias[2 * c:3 * c]

        bv.parts, bv.scale = [lambda: m.qkv.bias[2 * c:3 * c]], float(d)     # (fast_repack: a scaled parameter view)
        u, _ = self.conv("attn.v", wv, bv, xs, None, k=(1, 1, 1), p=(0, 0, 0), cout=c)
        pterm, _ = self.conv("attn.proj", lambda: m.proj_out.weight, lambda: m.proj_out.bias, u, None, k=(1, 1, 1),
                             p=(0, 0, 0), cout=c)
        out = self.act(n, c, d, h, w, halo=0)
        pp, op_ = pterm.ip, out.ip

        def run_ba():
            lib.attn_broadcast_add(xp, pp, None, m.num_heads, op_, n, c, d, h, w, sptr)

        self._emit(run_ba, "attn.broadcast_add", audit=dict(kind="attn_broadcast_add", x=x, p=pterm, rowsum=None,
                                                            heads=m.num_heads, out=out))

        def bwd():
            gy = out.grad
            if gy is None:
                raise CtsiError("internal: no gradient reached an attention output")
            # dP = sum over depth of gy  (fp32 -> bf16 (n,1,h,w,c))
            dsum = self.pool.get(n * h * w * c, torch.float32)
            dP = self.act(n, c, 1, h, w, halo=0)
            gyp, dsp2, dPp = gy.ip, _ptr(dsum), dP.ip

            def run_dsum():
                lib.attn_depthsum(gyp, dsp2, _ptr(prog._colsum), n, c, d, h, w, sptr)
                lib.f32_to_bf16(dsp2, dPp, n * h * w * c, sptr)

            self._emit(run_dsum, "attn.bwd.depthsum", audit=dict(kind="depthsum", src=gy, out=dP))
            # proj_out: dW_p, db_p, du
            defer = not os.environ.get("CTSI_TRAIN_NO_LIN_BATCH")     # (A/B timing, tests: one wgrad + bgrad launch pair per layer)
            self._conv_bwd("attn.proj", m.proj_out.weight, m.proj_out.bias, u, None, dP, False, (1, 1, 1), (1, 1),
                           (0, 0, 0), c, True, defer_wb=defer)
            du = u.grad
            # V third of qkv: dW_v, db_v (x D: the bias is added once per depth slice), d(xs)
            gqkv_w, gqkv_b = self.grad_buf(m.qkv.weight), self.grad_buf(m.qkv.bias)
            self._conv_bwd("attn.v", m.qkv.weight, m.qkv.bias, xs, None, du, False, (1, 1, 1), (1, 1), (0, 0, 0), c,
                           True, b_scale=float(d), gw=gqkv_w, gb=gqkv_b, gw_off=2 * c * c, gb_off=2 * c, w_src=wv, defer_wb=defer)
            dxs = xs.grad
            # GroupNorm under the depth sum: dy is d(xs) broadcast over depth; + gy (the identity path)
            self._gn_bwd(x, dxs, True, slot, m.norm, gamma, beta, False, None, None, False, gy)
            for a in ((dxs, gy) if defer else (dP, du, dxs, gy)):      # (deferred: dP and du are read by the batched launch)
                self.release(a)
            self.pool.put(dsum)
            u.grad = xs.grad = out.grad = None

        self.tape.append(bwd)
        return out

    # ---- TemporalAttention as true attention over depth (attention_mode='softmax', attention.py) ---------------------------
    def t_attention_softmax(self, m, x: Act) -> Act:
        return emit_softmax_attention_train(self, m, x)

    # ---- time embedding backward ------------------------------------------------------------------------------------------
    def _time_embed_bwd(self):
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        te = self.unet.time_embed.time_mlp
        n, dim, td, tot = self.n, self.dim, self.time_dim, self.total_out
        gw1, gb1 = self.grad_buf(te[1].weight), self.grad_buf(te[1].bias)
        gw2, gb2 = self.grad_buf(te[3].weight), self.grad_buf(te[3].bias)
        sincos = self.te_scratch
        lin1 = self.te_scratch[n * dim:]
        temb = self.te_scratch[n * dim + n * td:]

        def run():
            lib.linear_bwd(_ptr(temb), _ptr(prog.w_all), _ptr(prog.d_tbias), n, td, tot, 1, _ptr(prog.g_w_all),
                           _ptr(prog.g_b_all), _ptr(prog.g_temb), sptr)
            lib.linear_bwd(_ptr(lin1), _ptr(prog.w2), _ptr(prog.g_temb), n, td, td, 1, _ptr(gw2), _ptr(gb2),
                           _ptr(prog.g_lin1), sptr)
            lib.linear_bwd(_ptr(sincos), _ptr(prog.w1), _ptr(prog.g_lin1), n, dim, td, 0, _ptr(gw1), _ptr(gb1), None,
                           sptr)

        self._emit(run, "time_embed.bwd", audit=dict(kind="linear_bwd_chain", steps=[
            dict(x=temb, w=self.w_all, dy=self.d_tbias, rows=n, cin=td, cout=tot, silu_in=True, dw=self.g_w_all, db=self.g_b_all,
                 dx=self.g_temb),
            dict(x=lin1, w=self.w2, dy=self.g_temb, rows=n, cin=td, cout=td, silu_in=True, dw=gw2, db=gb2, dx=self.g_lin1),
            dict(x=sincos, w=self.w1, dy=self.g_lin1, rows=n, cin=dim, cout=td, silu_in=False, dw=gw1, db=gb1, dx=None)]))
        # the per-block Linear gradients are row slices of the stacked buffers
        for m in self.blocks:
            off = self.tb_off[id(m)]
            co = m.time_mlp[1].out_features
            self.grads[id(m.time_mlp[1].weight)] = self.g_w_all[off:off + co]
            self.grads[id(m.time_mlp[1].bias)] = self.g_b_all[off:off + co]

    # ---- execution ---------------------------------------------------------------------------------------------------------
    def set_diffusion(self, diffusion):
        self.sqrt_ac = diffusion.sqrt_alphas_cumprod.detach().to(self.ctx.device, torch.float32).contiguous()
        self.sqrt_1mac = diffusion.sqrt_one_minus_alphas_cumprod.detach().to(self.ctx.device, torch.float32).contiguous()
        if self.learn_sigma:
            self.lv_sched = loss_schedule_rows(diffusion).to(self.ctx.device).contiguous()

    def set_dropout(self, p: float, seed: int):
        """Probability and 64-bit seed of the NEXT forward (a program built with dropout=True only); the seed reaches the device
        buffer in run_forward."""
        if self.drop_state is None:
            raise CtsiError("internal: this train program was built without the dropout launches")
        self.drop_state.set(p, seed)
        if self.drop_state.thr <= 0:
            raise CtsiError("internal: a dropout program needs a threshold > 0 (thr == 0 takes the default kernels)")

    def set_vb_norm(self, norm_vb: torch.Tensor):
        """The bound's per-sample factors of the NEXT forward (a learn_sigma program only): learned_sigma.hybrid_norms."""
        if not self.learn_sigma:
            raise CtsiError("internal: this train program has no variational-bound term")
        self.norm_vb.copy_(norm_vb.to(torch.float32))

    def run_forward(self, z0, cond, t, noise, norm, mask=None) -> torch.Tensor:
        """Runs the forward launches and overwrites the tape (saved activations, t, noise) of this program (a new generation:
        engine.PhasedProgram)."""
        def load():
            self.z0.copy_(z0)
            self.cond.copy_(cond)
            self.noise.copy_(noise)
            self.t_rows.copy_(t.to(torch.int32))
            self.norm.copy_(norm.to(torch.float32))
            if self.drop_state is not None:
                self.drop_state.upload()
            self.use_mask = mask is not None
            if mask is not None:
                self.mask.copy_(mask.to(torch.float32))

        self.forward_ops(load)
        return self.loss_out[0].clone()

    def run_z0_pred(self, active: Optional[torch.Tensor]) -> torch.Tensor:
        """After run_forward: the clean latent its prediction stands for (one ctsi_z0_pred launch on the program's own z0, noise,
        t_rows, schedule tables and raw prediction), fp32 NCDHW.  `active` (bool, (n,); None = every row): the other rows come
        back as z0 itself and take no gradient.  Also stores the rows' d z0^ / d pred for the backward.  (Not for learn_sigma
        programs, whose `eps` holds 2L channels: train_step_pred refuses them.)"""
        n, L = self.n, self.L
        if self.z0_hat is None:
            self.z0_hat = self.persistent((n, L, self.d, self.h, self.w), torch.float32)
            self.g_z0 = self.persistent((n, L, self.d, self.h, self.w), torch.float32, zero=True)
            self.active = self.persistent((n,), torch.int32, zero=True)
            self.coef = self.persistent((n,), torch.float32, zero=True)
        dev = self.ctx.device
        act = torch.ones(n, dtype=torch.bool, device=dev) if active is None else active.to(device=dev, dtype=torch.bool)
        if tuple(act.shape) != (n,):
            raise ValueError(f"active must be a bool tensor of shape ({n},), got {tuple(act.shape)}")
        self.active.copy_(act.to(torch.int32))
        # coef[b] = d z0^ / d pred, float64 from the two tables the kernel reads, rounded once: -sqrt(1 / abar - 1) | -sqrt(1 - abar)
        t = self.t_rows.long()
        a, s = self.sqrt_ac.double()[t], self.sqrt_1mac.double()[t]
        coef = -s if self.prediction == "v_prediction" else -s / torch.where(act, a, torch.ones_like(a))
        self.coef.copy_(torch.where(act, coef, torch.zeros_like(coef)).float())
        self.lib.z0_pred(_ptr(self.z0), _ptr(self.noise), _ptr(self.eps), self.Lo, _ptr(self.sqrt_ac), _ptr(self.sqrt_1mac),
                         _ptr(self.t_rows), _ptr(self.active), int(self.prediction == "v_prediction"), n, L, self.d, self.h,
                         self.w, _ptr(self.z0_hat), self.ctx.sptr)
        return self.z0_hat.clone()

    def run_backward(self, grad_out: Optional[torch.Tensor], generation: Optional[int] = None,
                     grad_z0: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """`grad_z0` (train_step_pred): the gradient of run_z0_pred's result; the loss launch then is ctsi_loss_bwd_z0.
        `grad_out` None: the loss itself took no gradient (gscale 0)."""
        def load():
            if grad_out is None:
                self.gscale.zero_()
            else:
                self.gscale.copy_(grad_out.reshape(1).to(torch.float32))
            self.use_gz0 = grad_z0 is not None
            if grad_z0 is not None:
                if self.g_z0 is None:
                    raise CtsiError("internal: a gradient of the predicted latent without a run_z0_pred")
                self.g_z0.copy_(grad_z0.reshape(self.g_z0.shape))

        self.backward_ops(generation, load)
        return self.param_grads()


def _clone_grads(grads: List[torch.Tensor]) -> List[torch.Tensor]:
    """Copies of the program's gradient buffers for autograd to own (the program overwrites its buffers in the next backward).
    Buffers that share a storage -- the program's gradient arena -- are copied as ONE range and returned as views of the copy
    at the same offsets; a storage whose members cover less than half of the range they span is copied tensor by tensor."""
    if os.environ.get("CTSI_TRAIN_NO_GRAD_ARENA"):          # A/B timing: one copy per parameter, as before round 4
        return [g.clone() for g in grads]
    groups: Dict[int, List[int]] = {}
    for i, g in enumerate(grads):
        groups.setdefault(g.untyped_storage().data_ptr(), []).append(i)
    out: List[Optional[torch.Tensor]] = [None] * len(grads)
    for idx in groups.values():
        g0 = grads[idx[0]]
        lo = min(grads[i].storage_offset() for i in idx)
        hi = max(grads[i].storage_offset() + grads[i].numel() for i in idx)
        dense = all(grads[i].is_contiguous() and grads[i].dtype == g0.dtype for i in idx)
        if len(idx) == 1 or not dense or (hi - lo) > 2 * sum(grads[i].numel() for i in idx):
            for i in idx:
                out[i] = grads[i].clone()
            continue
        flat = torch.empty(0, dtype=g0.dtype, device=g0.device).set_(g0.untyped_storage(), lo, (hi - lo,)).clone()
        for i in idx:
            out[i] = flat.as_strided(grads[i].shape, grads[i].stride(), grads[i].storage_offset() - lo)
    return out


class _TrainStep(torch.autograd.Function):
    """loss = training loss of one batch; backward runs the engine's backward launches and hands the parameter
    gradients to autograd (which accumulates them into .grad like any other op)."""

    @staticmethod
    def forward(fctx, prog: UNetTrainProgram, z0, cond, t, noise, norm, mask, *params):
        ectx = prog.ctx
        with ectx.scope():
            loss = prog.run_forward(z0, cond, t, noise, norm, mask)
        fctx.prog = prog
        fctx.generation = prog.generation
        return loss

    @staticmethod
    def backward(fctx, grad_out):
        prog = fctx.prog
        with prog.ctx.scope():
            grads = _clone_grads(prog.run_backward(grad_out, fctx.generation))
        return (None,) * 7 + tuple(grads)


def train_step(prog: UNetTrainProgram, z0, cond, t, noise, norm, mask=None) -> torch.Tensor:
    return _TrainStep.apply(prog, z0, cond, t, noise, norm, mask, *prog.params)


class _TrainStepPred(torch.autograd.Function):
    """(loss, z0_pred) of one batch: _TrainStep with the predicted clean latent as a second differentiable output.  Either
    gradient may be absent in the backward; one generation check covers both outputs."""

    @staticmethod
    def forward(fctx, prog: UNetTrainProgram, z0, cond, t, noise, norm, mask, active, *params):
        with prog.ctx.scope():
            loss = prog.run_forward(z0, cond, t, noise, norm, mask)
            z0_pred = prog.run_z0_pred(active)
        fctx.prog = prog
        fctx.generation = prog.generation
        fctx.set_materialize_grads(False)
        return loss, z0_pred

    @staticmethod
    def backward(fctx, grad_loss, grad_z0):
        prog = fctx.prog
        if grad_loss is None and grad_z0 is None:
            return (None,) * (8 + len(prog.params))
        with prog.ctx.scope():
            grads = _clone_grads(prog.run_backward(grad_loss, fctx.generation, grad_z0))
        return (None,) * 8 + tuple(grads)


def train_step_pred(prog: UNetTrainProgram, z0, cond, t, noise, norm, mask=None, active=None):
    """train_step that also returns the clean latent the prediction stands for (fp32 NCDHW, ctsi_z0_pred), with a gradient:
    `active` (bool, (n,); None = all) names the rows that take part -- the others are returned as z0 and get no gradient.
    learn_sigma programs raise CtsiError."""
    if prog.learn_sigma:
        raise CtsiError("train_step_pred does not support learn_sigma programs: the hybrid loss has its own backward kernel, "
                        "which takes no gradient of the predicted latent")
    return _TrainStepPred.apply(prog, z0, cond, t, noise, norm, mask, active, *prog.params)
