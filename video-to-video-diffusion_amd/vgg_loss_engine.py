"""The VGG-19 perceptual loss on the HIP engine: forward and backward of `losses.VGGPerceptualLoss` (reference
models/losses.py:22-146).

One `VGGLossProgram` serves one (N images, H, W) key of one loss module.  The N sampled slices of `pred` and the N of `target`
go through the VGG-19 `features` stack as ONE batch of 2 N images (half the launches, the weights read once): the images are
the depth axis of a bf16 channels-last tensor and every 3 x 3 convolution is a (1, 3, 3) / pad (0, 1, 1) conv plan, so packed
weight images go through the engine's content-addressed cache like every other layer's.

  forward   ctsi_vgg_prep (twice: pred, target) | per conv: ctsi_conv_fwd with the ReLU epilogue on the planar halo-tile form
            (conv3_planar_k32_kernel), ctsi_conv_fwd + ctsi_relu_bf16 in place where the plan keeps the gather kernel (the
            3 -> 64 stem, planes too small for a tile, deep-K layers on small grids) | ctsi_maxpool2_fwd |
            per compared feature ctsi_feat_loss_fwd (fixed-order partial sums) | ONE ctsi_feat_loss_finalize -> device scalar
  backward  over the pred half only, deepest layer first: ctsi_feat_grad_relu_bwd (loss term + ReLU mask from the stored
            post-ReLU activation, one pass per layer boundary) | the conv's data gradient = the same (1, 3, 3) plan on flipped,
            transposed weights (ctsi_weight_dgrad_layout, as train_engine._conv_bwd does for stride-1 convs) |
            ctsi_maxpool2_bwd | ctsi_vgg_prep_bwd -> fp32 NCDHW grad_pred, zero on unsampled slices

No weight gradient exists: the VGG weights are frozen.  Every reduction has a fixed order and nothing uses float atomics, so loss
and gradient are bit-identical run to run.

In-place ReLU (torchvision's): a feature taken at a conv that another block follows is overwritten by that block's leading
ReLU before the loss reads it, so it is compared POST-ReLU; only a conv that ends the stack is compared pre-ReLU.  Here the
ReLU pass runs right behind every conv but the stack's last module, which gives exactly that.

Every launch carries an audit record (engine.Program._emit): references to what it reads and writes and the scalars of its
formula, from which tests/loss_audit.py recomputes each launch in float64.  The records change nothing about the launches.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from .engine import Act, Ctx, PhasedProgram, _ptr
from .lib import ConvDesc, CtsiError

# torchvision's vgg19().features: module index -> ("conv", cin, cout) | ("relu",) | ("pool",); 37 modules, 16 convs
VGG19_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


# torchvision's vgg16().features without its last pool: 30 modules, 13 convs; lpips' five slices end on the ReLUs 3, 8, 15, 22, 29
VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512]
LPIPS_TAPS = (3, 8, 15, 22, 29)


def feature_modules(cfg) -> List[tuple]:
    mods, cin = [], 3
    for v in cfg:
        if v == "M":
            mods.append(("pool",))
        else:
            mods.extend([("conv", cin, v), ("relu",)])
            cin = v
    return mods


def vgg19_feature_modules() -> List[tuple]:
    return feature_modules(VGG19_CFG)


VGG19_MODULES = vgg19_feature_modules()
VGG16_MODULES = feature_modules(VGG16_CFG)
K, P = (1, 3, 3), (0, 1, 1)


class VGGLossProgram(PhasedProgram):
    """convs: {module index: nn.Conv2d} up to max(feature_layers); n_img: sampled slices per call (B * num).  `modules`: the
    stack's module table (VGG-19 for the feature loss, VGG-16 for LPIPS).  `distance`: "feat" -- the L1 / L2 feature distance
    averaged over the layers into one scalar -- or "lpips" -- the unit-normalised, head-weighted squared distance of
    csrc/lpips.hip, one value PER IMAGE (`heads`: one (C,) weight tensor per layer; every layer a ReLU output).  The conv /
    ReLU / pool / data-gradient launches are the same for both."""

    def __init__(self, ctx: Ctx, convs, feature_layers: Sequence[int], use_l1: bool, n_img: int, h: int, w: int, *,
                 modules: Sequence[tuple] = VGG19_MODULES, distance: str = "feat", heads=None):
        super().__init__(ctx)
        lib, sptr, prog = self.lib, ctx.sptr, self
        self.n_img, self.h, self.w = n_img, h, w
        self.layers = list(feature_layers)
        last = self.layers[-1]
        nl = len(self.layers)
        n2 = 2 * n_img
        if distance not in ("feat", "lpips"):
            raise CtsiError(f"internal: unknown feature distance {distance!r}")
        self.lpips = distance == "lpips"
        self.label = "LPIPS" if self.lpips else "VGG loss"
        self.stale_msg = (f"backward of a{'n' if self.lpips else ''} {self.label} forward whose saved activations were "
                          "overwritten (internal: a program was handed out twice)")
        if self.lpips:
            if heads is None or len(heads) != nl or any(modules[i][0] != "relu" for i in self.layers):
                raise CtsiError("internal: the LPIPS distance needs one head per tap and taps at ReLU outputs")
            self.blocks = lib.lpips_blocks()
            self.partials = self.persistent((nl * n_img * self.blocks,), torch.float64)
            self.out = self.persistent((n_img + nl,), torch.float32)          # per-image values, then the tap means
            self.gl = self.persistent((n_img,), torch.float32)                # the upstream gradient, per image
            self.track(*heads)
            head_bufs = [self.dev_f32(lambda t=t: t.reshape(-1)) for t in heads]
        else:
            self.blocks = lib.feat_loss_blocks()
            self.partials = self.persistent((nl * self.blocks,), torch.float64)
            self.out = self.persistent((1 + nl,), torch.float32)
            self.gl = self.persistent((1,), torch.float32)
        self.xin = Act(self.persistent((n2 * h * w * 8,), torch.bfloat16), 1, 8, n2, h, w)

        # ---- forward --------------------------------------------------------------------------------------------------------
        nodes, x = [], self.xin
        for i, m in enumerate(modules[:last + 1]):
            if m[0] == "conv":
                conv = convs[i]
                self.track(conv.weight, conv.bias)
                relu = i < last
                fused = relu and self._planar(x, m[2])      # the planar halo-tile form applies ReLU in its epilogue
                out, _ = self.conv(f"vgg.{i}", (lambda c=conv: c.weight.unsqueeze(2)), (lambda c=conv: c.bias), x, None, k=K,
                                   p=P, cout=m[2], cin_w=3 if i == 0 else None, act=2 if fused else 0)
                if relu and not fused:
                    self._emit_relu(f"vgg.{i + 1}.relu", out)
                nodes.append(dict(node="conv", i=i, x=x, out=out, relu=relu, conv=conv, feats=[]))
                x = out
            elif m[0] == "pool":
                out = self.act(1, x.c, x.d, x.h // 2, x.w // 2)
                xp, op, xd, xh, xw, xc = x.ip, out.ip, x.d, x.h, x.w, x.c
                nbytes = 2.0 * x.d * x.h * x.w * x.c * 1.25

                def run_pool(xp=xp, op=op, xd=xd, xh=xh, xw=xw, xc=xc):
                    lib.maxpool2_fwd(xp, op, xd, xh, xw, xc, sptr)

                self._emit(run_pool, f"vgg.{i}.pool", 0.0, "maxpool2_fwd", nbytes=nbytes,
                           audit=dict(kind="maxpool2_fwd", x=x, out=out))
                nodes.append(dict(node="pool", i=i, x=x, out=out, relu=False, feats=[]))
                x = out
            if i in self.layers:       # (a ReLU index lands on its conv's node: the same post-ReLU tensor)
                nodes[-1]["feats"].append(self.layers.index(i))
        counts = [0] * nl
        sq = 0 if use_l1 else 1
        taps: List[Optional[Act]] = [None] * nl      # per compared layer: the Act it is taken from (audit records only)
        for node in nodes:
            a = node["out"]
            half = n_img * a.h * a.w * a.c
            for l in node["feats"]:
                pp, tp = a.ip, C.c_void_p(a.ip.value + 2 * half)
                taps[l] = a
                if self.lpips:
                    pos = a.h * a.w
                    counts[l] = pos                    # LPIPS means over positions, per image
                    if a.c != head_bufs[l].numel():
                        raise CtsiError(f"LPIPS head {l} has {head_bufs[l].numel()} weights, its tap has {a.c} channels")
                    hp, dst = _ptr(head_bufs[l]), C.c_void_p(self.partials.data_ptr() + 8 * l * n_img * self.blocks)

                    def run_dist(pp=pp, tp=tp, hp=hp, dst=dst, pos=pos, c=a.c):
                        lib.lpips_dist_fwd(pp, tp, hp, n_img, pos, c, dst, sptr)

                    nb = n_img * self.blocks
                    self._emit(run_dist, f"vgg.{node['i']}.lpips", 0.0, "lpips_dist", nbytes=4.0 * half,
                               audit=dict(kind="lpips_dist", x=a, n_img=n_img, l=l, half=half, pos=pos, head=head_bufs[l],
                                          slab=self.partials[l * nb:(l + 1) * nb], partials=self.partials, blocks=self.blocks))
                    continue
                counts[l] = half
                dst = C.c_void_p(self.partials.data_ptr() + 8 * l * self.blocks)

                def run_loss(pp=pp, tp=tp, dst=dst, half=half):
                    lib.feat_loss_fwd(pp, tp, half, sq, dst, sptr)

                self._emit(run_loss, f"vgg.{node['i']}.loss", 0.0, "feat_loss", nbytes=4.0 * half,
                           audit=dict(kind="feat_loss", x=a, n_img=n_img, l=l, half=half, sq=sq,
                                      slab=self.partials[l * self.blocks:(l + 1) * self.blocks], partials=self.partials,
                                      blocks=self.blocks))
        self.counts = self.persistent((nl,), torch.int64)
        self.counts.copy_(torch.tensor(counts, dtype=torch.int64))
        pa, cn, ob = _ptr(self.partials), _ptr(self.counts), _ptr(self.out)

        if self.lpips:
            tm = C.c_void_p(self.out.data_ptr() + 4 * n_img)

            def run_fin():
                lib.lpips_finalize(pa, cn, nl, n_img, ob, tm, sptr)

            self._emit(run_fin, "vgg.lpips.finalize", 0.0, "lpips_finalize",
                       audit=dict(kind="lpips_finalize", partials=self.partials, counts=self.counts, taps=taps, n_img=n_img,
                                  blocks=self.blocks, out=self.out))
        else:
            def run_fin():
                lib.feat_loss_finalize(pa, cn, nl, ob, sptr)

            self._emit(run_fin, "vgg.loss.finalize", 0.0, "feat_loss_finalize",
                       audit=dict(kind="feat_loss_finalize", partials=self.partials, counts=self.counts, taps=taps, n_img=n_img,
                                  blocks=self.blocks, out=self.out))
        self.end_forward()

        # ---- backward (pred half) ------------------------------------------------------------------------------------------
        glp = _ptr(self.gl)
        kind_loss = 1 if use_l1 else 2
        g: Optional[Act] = None
        for node in reversed(nodes):
            a = node["out"]
            half = n_img * a.h * a.w * a.c
            if self.lpips and node["feats"]:
                l, = node["feats"]
                gout = g if g is not None else self.act(1, a.c, n_img, a.h, a.w)
                gi, yp, tp, go = (g.ip if g is not None else C.c_void_p(0)), a.ip, C.c_void_p(a.ip.value + 2 * half), gout.ip
                hp = _ptr(head_bufs[l])

                def run_lgrad(gi=gi, yp=yp, tp=tp, hp=hp, go=go, pos=a.h * a.w, c=a.c):
                    lib.lpips_grad_relu_bwd(gi, yp, tp, hp, go, n_img, pos, c, glp, sptr)

                self._emit(run_lgrad, f"vgg.{node['i']}.grad", 0.0, "lpips_grad_relu_bwd", nbytes=8.0 * half,
                           audit=dict(kind="lpips_grad_relu", g_in=g, no_g_in=g is None, y=a, n_img=n_img, l=l, half=half,
                                      pos=a.h * a.w, head=head_bufs[l], gl=self.gl, out=gout))
                g = gout
            elif node["feats"] or node["relu"]:
                if g is None and not node["feats"]:
                    raise CtsiError("internal: no gradient reaches the deepest VGG layer")
                kind = kind_loss if node["feats"] else 0
                coef = len(node["feats"]) / (nl * float(half))
                gout = g if g is not None else self.act(1, a.c, n_img, a.h, a.w)
                gi, yp, tp, go = (g.ip if g is not None else C.c_void_p(0)), a.ip, C.c_void_p(a.ip.value + 2 * half), gout.ip
                relu = int(node["relu"])

                def run_grad(gi=gi, yp=yp, tp=tp, go=go, half=half, coef=coef, kind=kind, relu=relu):
                    lib.feat_grad_relu_bwd(gi, yp, tp, go, half, coef, kind, relu, glp, sptr)

                self._emit(run_grad, f"vgg.{node['i']}.grad", 0.0, "feat_grad_relu_bwd", nbytes=(8.0 if kind else 6.0) * half,
                           audit=dict(kind="feat_grad_relu", g_in=g, no_g_in=g is None, y=a, n_img=n_img, l=list(node["feats"]),
                                      nl=nl, half=half, coef=coef, loss_kind=kind, relu=relu, sq=sq, gl=self.gl, out=gout))
                g = gout
            xa = node["x"]
            if node["node"] == "pool":
                gx = self.act(1, xa.c, n_img, xa.h, xa.w)
                xp, gp, gxp, xh, xw, xc = xa.ip, g.ip, gx.ip, xa.h, xa.w, xa.c

                def run_pool_bwd(xp=xp, gp=gp, gxp=gxp, xh=xh, xw=xw, xc=xc):
                    lib.maxpool2_bwd(xp, gp, gxp, n_img, xh, xw, xc, sptr)

                self._emit(run_pool_bwd, f"vgg.{node['i']}.pool.bwd", 0.0, "maxpool2_bwd",
                           nbytes=2.0 * n_img * xa.h * xa.w * xa.c * 2.25,
                           audit=dict(kind="maxpool2_bwd", x=xa, g=g, n_img=n_img, out=gx))
            else:
                conv = node["conv"]
                cout, cin = conv.weight.shape[0], conv.weight.shape[1]
                gx = self.act(1, xa.c, n_img, xa.h, xa.w)

                def wfn(conv=conv, cout=cout, cin=cin, rows=xa.c):
                    # (rows, cout, 1, 3, 3): the layer's weights flipped and transposed; rows past cin (the 8-channel input
                    # image of the 3-channel stem) are zero
                    src = conv.weight.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
                    outw = torch.zeros((rows, cout, 1, 3, 3), dtype=torch.float32, device=ctx.device)
                    lib.weight_dgrad_layout(_ptr(src), _ptr(outw), cout, cin, 9, 0, cin, sptr)
                    src.record_stream(ctx.stream)
                    return outw

                self.conv(f"vgg.{node['i']}.dgrad", wfn, None, g, None, k=K, p=P, cout=xa.c, out=gx,
                          audit=dict(kind="dgrad", op="convT", g=g, weight=lambda c=conv: c.weight.unsqueeze(2), w_ci=None, k=K,
                                     s=(1, 1), p=P))
            self.release(g)
            g = gx
        self.g_in = g
        self.finalize_layout()

    def _planar(self, x: Act, cout: int) -> bool:
        """Whether the (1, 3, 3) conv of `x` to `cout` channels is planned onto the planar halo-tile form (ctsi_conv_plan_form,
        bit 16; CTSI_CONV_PLANAR=0 keeps every layer on the gather kernel) -- the only form with a ReLU epilogue."""
        plan, form = C.c_void_p(), (C.c_int * 8)()
        self.lib.conv_plan_create(C.byref(plan), C.byref(ConvDesc(0, 1, 3, 3, 1, 1, 0, 1, 1, x.n, x.c, 0, cout, x.d, x.h, x.w, 0)))
        try:
            self.lib.conv_plan_form(plan, form)
        finally:
            self.lib.conv_plan_destroy(plan)
        return bool(form[4] & 16)

    def _emit_relu(self, name: str, a: Act):
        lib, sptr = self.lib, self.ctx.sptr
        ap, cnt = a.ip, a.d * a.h * a.w * a.c

        def run():
            lib.relu_bf16(ap, cnt, sptr)

        self._emit(run, name, 0.0, "relu_bf16", nbytes=4.0 * cnt, audit=dict(kind="relu", x=a, out=a))

    # ---- execution -----------------------------------------------------------------------------------------------------------
    # `args`, the per-distance part of a call, the same tuple for the forward and its backward:
    #   feature loss  (slices, norm, b, d, num)   x0, x1: fp32 contiguous (B, 1, D, H, W) device tensors, pred and target
    #   LPIPS         (c, normalize)              x0, x1: fp32 contiguous (N, c = 1 | 3, H, W) device tensors
    def run_forward(self, x0: torch.Tensor, x1: torch.Tensor, args: tuple) -> torch.Tensor:
        """Returns the fp32 device tensor [loss, layer means] (LPIPS: [N per-image values, tap means])."""
        lib, sptr, h, w = self.lib, self.ctx.sptr, self.h, self.w
        if (x0.shape[0] if self.lpips else args[2] * args[4]) != self.n_img:
            raise CtsiError(f"internal: the {self.label} program was built for another number of images")

        def load():
            for src, off in ((x0, 0), (x1, self.n_img * h * w * 8 * 2)):
                dst = C.c_void_p(self.xin.ip.value + off)
                if self.lpips:
                    c, normalize = args
                    lib.lpips_prep(_ptr(src), dst, self.n_img, c, h, w, int(normalize), sptr)
                else:
                    slices, norm, b, d, num = args
                    lib.vgg_prep(_ptr(src), _ptr(slices), _ptr(norm), dst, b, d, num, h, w, sptr)
            x0.record_stream(self.ctx.stream)
            x1.record_stream(self.ctx.stream)

        self.forward_ops(load)
        out = self.out.clone()
        self.check_errors()
        return out

    def run_backward(self, grad_out: torch.Tensor, args: tuple, generation: int) -> torch.Tensor:
        """grad_out: fp32 device, one element (LPIPS: (N,)); returns the gradient of x0, fp32, in x0's shape."""
        lib, sptr, h, w = self.lib, self.ctx.sptr, self.h, self.w
        self.backward_ops(generation, lambda: self.gl.copy_(grad_out.reshape(self.gl.shape)))
        if self.lpips:
            c, normalize = args
            grad = torch.empty((self.n_img, c, h, w), dtype=torch.float32, device=self.ctx.device)
            lib.lpips_prep_bwd(self.g_in.ip, _ptr(grad), self.n_img, c, h, w, int(normalize), sptr)
        else:
            slices, norm, b, d, num = args
            grad = torch.empty((b, 1, d, h, w), dtype=torch.float32, device=self.ctx.device)
            lib.vgg_prep_bwd(self.g_in.ip, _ptr(slices), _ptr(norm), _ptr(grad), b, d, num, h, w, sptr)
        self.check_errors()
        return grad
