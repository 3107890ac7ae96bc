"""Structural losses of the reference's `models/losses.py` on the HIP engine.

`MS_SSIM_Loss` (losses.py:149-276) is a differentiable loss here: forward and backward are HIP launches
(csrc/msssim.hip) behind a `torch.autograd.Function`, 6 launches forward and 5 backward, with no
host read in either direction.  `CombinedLoss` (losses.py:279-361) keeps the reference's bookkeeping around it.
`VGGPerceptualLoss` (losses.py:22-146) runs on the engine too (vgg_loss_engine.py, csrc/vgg_loss.hip),
forward and backward, once it is given VGG-19 `features` weights: `VGGPerceptualLoss(weights=state_dict_or_path)`.  The
reference fetches them with `torchvision.models.vgg19(pretrained=True)`; the engine depends on neither the package nor a
download, and NO weights ship with the project: save `torchvision.models.vgg19(weights="IMAGENET1K_V1").features.state_dict()`
(or the whole model's state dict) on a machine that has torchvision and pass the file.  Without `weights` the constructor
raises `NotImplementedError`, so a `CombinedLoss` needs `c.perceptual_loss = VGGPerceptualLoss(weights=...)` before its
perceptual term is first due, or `lambda_perceptual=0`.

Semantics of `VGGPerceptualLoss(...)(pred, target)`, both (B, 1, D, H, W) in [-1, 1]: `num = max(1, int(D * rate))` slices per
sample at `torch.linspace(0, D - 1, num, dtype=torch.long)` (all of them when num >= D); each slice becomes the 3-channel image
`((x + 1) / 2 - mean_c) / std_c`; the VGG-19 `features` stack is cut into blocks `features[prev : idx + 1]` for idx in
`feature_layers`; the loss is the mean over blocks of `F.l1_loss` (`use_l1=False`: `F.mse_loss`) between the block outputs of
pred and target.  torchvision's ReLUs are in place: a block that ends on a conv and is followed by another block is compared
AFTER the next block's leading ReLU has overwritten it, so with the default list the features of convs 2, 7, 12, 21 are
post-ReLU and that of conv 30 is pre-ReLU.  Deviations from the reference: H and W must be multiples of 16 (`ValueError`; the
training sizes are 192 and 512); the tensors must be ROCm tensors (`CtsiError`, as for `MS_SSIM_Loss`); the gradient is computed
for `pred` only (`target` is detached, as the reference's `no_grad` does); activations are bf16 with fp32 accumulation, like
every engine layer -- the test criterion is the error of the same torch ops under bf16 autocast.

Semantics of `MS_SSIM_Loss()(pred, target)`, both (B, C, D, H, W) in [-1, 1]: every (b, c, d) plane is an H x W image
of `(v + 1) / 2`; five levels of the full SSIM map under the zero-padded 11 x 11 Gaussian window (sigma 1.5), the
level value is the mean over all planes and pixels, a 2 x 2 average pool (floor) between levels,
`loss = 1 - prod_i mean_i ** w_i`.  A negative level mean gives NaN for the loss and every gradient element, as
torch's `pow` does in the reference.  The gradient is computed for `pred` only.

`LPIPS` is the perceptual distance of the `lpips` package (0.1.x, net='vgg', eval mode) that the reference's VAE trainer
uses (training/train_vae.py:42-169), on the same engine program with a VGG-16 module table and the kernels of csrc/lpips.hip
(DESIGN.md section 30).  Semantics of `LPIPS(weights=...)(in0, in1)`, both (N, 3, H, W) in [-1, 1]: the scaling layer
`(x - shift_c) / scale_c`; torchvision's VGG-16 `features` 0..29; at the ReLU outputs 3, 8, 15, 22, 29 both feature maps are
divided, per position, by their 2-norm over the channels plus 1e-10; the tap's value is the mean over positions of
`sum_c w_c (u_c - v_c)^2` with the tap's learned 1x1 head `w`; the result is the sum of the five tap values PER IMAGE, shape
(N, 1, 1, 1).  The same deviations as for `VGGPerceptualLoss` apply (H, W multiples of 16; ROCm tensors; gradient for `in0`
only; bf16 activations), and again no weights ship or are fetched.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .engine import Ctx, _ptr
from .lib import CtsiError
from .vgg_loss_engine import LPIPS_TAPS, VGG16_MODULES, VGG19_MODULES, VGGLossProgram

MIN_SIZE = 16          # four 2 x 2 pools must leave at least one pixel
MAX_WINDOW = 15        # csrc/msssim.hip: odd windows 1 .. 15
LEVEL_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

# free workspaces per (device index, planes, h, w, window, want_grad).  A forward in grad mode owns its workspace (it holds
# the coefficient maps) until its backward has run, so two losses of one shape in one graph never share one.
_WORKSPACES: Dict[Tuple, List[torch.Tensor]] = {}


def _take_workspace(ctx: Ctx, key: Tuple) -> torch.Tensor:
    free = _WORKSPACES.setdefault(key, [])
    if free:
        return free.pop()
    nbytes = ctx.lib.msssim_workspace_bytes(*key[1:])
    if nbytes == 0:
        msg = ctx.lib.last_error()
        raise CtsiError(f"ctsi_msssim_workspace_bytes failed: {msg.decode() if msg else '?'}")
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=ctx.device)


class _MSSSIMFn(torch.autograd.Function):
    """loss = 1 - MS-SSIM(pred, target) on fp32 contiguous device tensors; backward gives pred's gradient."""

    @staticmethod
    def forward(fctx, pred, target, window, want_grad, owner):
        ctx = Ctx.get(pred.device)
        b, c, d, h, w = pred.shape
        planes = b * c * d
        key = (ctx.device.index, planes, h, w, int(window), int(bool(want_grad)))
        out = torch.empty(6, dtype=torch.float32, device=pred.device)
        with ctx.scope():
            ws = _take_workspace(ctx, key)
            ctx.lib.msssim_fwd(_ptr(pred), _ptr(target), planes, h, w, int(window), key[-1], _ptr(ws), _ptr(out), ctx.sptr)
        if owner is not None:
            owner.last_level_means = out[1:6]
        if want_grad:
            fctx.save_for_backward(pred, target)
            fctx.ws, fctx.key = ws, key
        else:
            _WORKSPACES[key].append(ws)      # every use is ordered on the engine stream
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_loss):
        if getattr(fctx, "ws", None) is None:
            raise CtsiError("MS_SSIM_Loss: backward ran twice on one forward (the coefficient maps are released after the "
                            "first backward); run the forward again")
        pred, target = fctx.saved_tensors
        ctx = Ctx.get(pred.device)
        b, c, d, h, w = pred.shape
        g = grad_loss.detach().to(torch.float32).contiguous()
        grad_pred = torch.empty_like(pred)
        with ctx.scope():
            ctx.lib.msssim_bwd(_ptr(pred), _ptr(target), b * c * d, h, w, fctx.key[4], _ptr(fctx.ws), _ptr(g),
                               _ptr(grad_pred), ctx.sptr)
        _WORKSPACES[fctx.key].append(fctx.ws)
        fctx.ws = None
        return grad_pred, None, None, None, None


def _vgg_state_dict(weights) -> Dict[str, torch.Tensor]:
    """A state dict, or a path to one saved with torch.save (loaded with weights_only=True)."""
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    if not isinstance(weights, dict):
        raise ValueError(f"weights must be a state dict or a path to one, got {type(weights).__name__}")
    return weights


def _conv_param(sd: Dict[str, torch.Tensor], idx: int, kind: str, shape: Tuple[int, ...], label: str,
                extra_names: Sequence[str] = ()) -> torch.Tensor:
    """`features.{idx}.{kind}` or `{idx}.{kind}` (torchvision's names for the whole model / its `features`), or one of
    `extra_names` with 1 .. 5 for its '<k>' (lpips' `net.slice<k>.{idx}.{kind}`), shape-checked."""
    names = [f"features.{idx}.{kind}", f"{idx}.{kind}"] + [e.replace("<k>", str(k)) for e in extra_names for k in range(1, 6)]
    name = next((n for n in names if n in sd), None)
    if name is None:
        extra = "".join(f", or '{e}'" for e in extra_names)
        raise ValueError(f"{label} weights: key '{names[0]}' (or '{names[1]}'{extra}) is missing")
    t = sd[name]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{label} weights: key '{name}' has shape {got}, expected {tuple(shape)}")
    return t


def _frozen_convs(sd: Dict[str, torch.Tensor], modules: Sequence[tuple], label: str,
                  extra_names: Sequence[str] = ()) -> Dict[int, nn.Conv2d]:
    """{module index: nn.Conv2d} of the convs of a module table (vgg_loss_engine.feature_modules), filled from `sd`;
    `extra_names` may name {idx} and {kind}."""
    convs = {}
    for i, m in enumerate(modules):
        if m[0] == "conv":
            conv = convs[i] = nn.Conv2d(m[1], m[2], kernel_size=3, padding=1)
            with torch.no_grad():
                for kind, shape in (("weight", (m[2], m[1], 3, 3)), ("bias", (m[2],))):
                    extra = [e.format(idx=i, kind=kind) for e in extra_names]
                    getattr(conv, kind).copy_(_conv_param(sd, i, kind, shape, label, extra))
    return convs


def _rate_slices(depth: int, rate: float) -> torch.Tensor:
    """`max(1, int(depth * rate))` evenly spaced slices of `depth` (host, int64): the reference's own expression."""
    num = max(1, int(depth * rate))
    if num < depth:
        return torch.linspace(0, depth - 1, num, dtype=torch.long)
    return torch.arange(depth, dtype=torch.long)


class _ProgramPool:
    """Free programs of a loss module per (device index, images, h, w), kept where engine.invalidate_engine_cache finds them.
    A forward in grad mode owns its program (it holds the activations) until its backward has run, so two losses of one shape
    in one graph never share one; a program that comes back after the cache was dropped is not kept."""

    def _take_program(self, ctx: Ctx, n_img: int, h: int, w: int) -> VGGLossProgram:
        key = (ctx.device.index, n_img, h, w)
        cache = self.__dict__.setdefault("_ctsi_programs", {})
        free = cache.setdefault(key, [])
        if free:
            return free.pop()
        prog = self._build_program(ctx, n_img, h, w)
        prog.key, prog.home = key, cache
        return prog

    def _give_program(self, prog: VGGLossProgram):
        if self.__dict__.get("_ctsi_programs") is prog.home:
            prog.home.setdefault(prog.key, []).append(prog)


def _owned_program(fctx, name: str) -> VGGLossProgram:
    """The program a forward in grad mode kept for its backward."""
    prog = getattr(fctx, "prog", None)
    if prog is None:
        raise CtsiError(f"{name}: backward ran twice on one forward (the saved activations are released after the first "
                        "backward); run the forward again")
    return prog


def _hand_back(fctx, prog: VGGLossProgram):
    fctx.owner._give_program(prog)
    fctx.prog = None


class _VGGLossFn(torch.autograd.Function):
    """loss = mean over feature blocks of the L1 / L2 feature distance; backward gives pred's gradient (fp32 NCDHW, exactly
    zero on unsampled slices)."""

    @staticmethod
    def forward(fctx, pred, target, owner, want_grad):
        ctx = Ctx.get(pred.device)
        b, _, d, h, w = pred.shape
        idx = owner.slice_indices(d)
        num = idx.numel()
        with ctx.scope():
            slices = idx.to(device=pred.device, dtype=torch.int32)
            norm = torch.cat([owner.mean.reshape(-1), owner.std.reshape(-1)]).to(device=pred.device, dtype=torch.float32)
            prog = owner._take_program(ctx, b * num, h, w)
            out = prog.run_forward(pred, target, (slices, norm, b, d, num))
        owner.last_layer_means = out[1:]
        if want_grad:
            fctx.save_for_backward(slices, norm)
            fctx.prog, fctx.owner, fctx.generation, fctx.dims = prog, owner, prog.generation, (b, d, num)
        else:
            owner._give_program(prog)          # every use is ordered on the engine stream
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_loss):
        prog = _owned_program(fctx, "VGGPerceptualLoss")
        with prog.ctx.scope():
            g = grad_loss.detach().to(torch.float32).contiguous()
            grad_pred = prog.run_backward(g, fctx.saved_tensors + fctx.dims, fctx.generation)
        _hand_back(fctx, prog)
        return grad_pred, None, None, None


class VGGPerceptualLoss(_ProgramPool, nn.Module):
    """The reference's VGG-19 perceptual loss on sampled 2-D slices, forward and backward on the HIP engine.

    Args as the reference's (feature_layers: strictly increasing indices into VGG-19 `features`, 0-36; use_l1; slice_sample_rate)
    plus the keyword `weights`: a state dict of torchvision's VGG-19 (`features.{i}.weight / bias`) or of its `features`
    (`{i}.weight / bias`), or a path to one (`torch.load(..., weights_only=True)`).  Only the convs up to max(feature_layers)
    are read; they are held frozen under the reference's names `vgg_blocks.{block}.{j}`.  `weights=None` raises
    `NotImplementedError`: the engine neither imports torchvision nor downloads, and no weights ship with the project.
    `last_layer_means` holds the per-block distances of the latest forward as a device tensor.  See the module docstring for
    the semantics and the deviations (H, W multiples of 16; ROCm tensors; gradient for `pred` only)."""

    def __init__(self, feature_layers: list = [2, 7, 12, 21, 30], use_l1: bool = True, slice_sample_rate: float = 0.2, *,
                 weights: Optional[Union[Dict[str, torch.Tensor], str, "os.PathLike"]] = None):
        if weights is None:
            raise NotImplementedError(
                "VGGPerceptualLoss needs pre-trained VGG-19 weights, which the reference fetches through torchvision from the "
                "network; the HIP engine does neither.  Pass them: VGGPerceptualLoss(weights=<state dict or path of "
                "torchvision's vgg19 / vgg19().features>) (DESIGN.md section 22), or use CombinedLoss(lambda_perceptual=0, ...) "
                "or MS_SSIM_Loss.")
        super().__init__()
        layers = list(feature_layers)
        if (not layers or any(not isinstance(v, int) or isinstance(v, bool) for v in layers) or layers[0] < 0
                or layers[-1] >= len(VGG19_MODULES) or any(a >= b for a, b in zip(layers, layers[1:]))):
            raise ValueError(f"feature_layers must be strictly increasing indices into VGG-19 features (0-"
                             f"{len(VGG19_MODULES) - 1}), got {feature_layers!r}")
        if not 0.0 <= float(slice_sample_rate):
            raise ValueError(f"slice_sample_rate must not be negative, got {slice_sample_rate!r}")
        sd = _vgg_state_dict(weights)
        self.feature_layers = layers
        self.use_l1 = use_l1
        self.slice_sample_rate = slice_sample_rate
        self.vgg_blocks = nn.ModuleList()
        self._convs = _frozen_convs(sd, VGG19_MODULES[:layers[-1] + 1], "VGG-19")
        prev = 0
        for idx in layers:
            block = []
            for i in range(prev, idx + 1):
                m = VGG19_MODULES[i]
                if m[0] == "conv":
                    block.append(self._convs[i])
                elif m[0] == "relu":
                    block.append(nn.ReLU(inplace=True))
                else:
                    block.append(nn.MaxPool2d(kernel_size=2, stride=2))
            self.vgg_blocks.append(nn.Sequential(*block))
            prev = idx + 1
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self.last_layer_means = None

    def slice_indices(self, depth: int) -> torch.Tensor:
        """The sampled slices of a volume of `depth` slices (host, int64): the reference's own expression."""
        return _rate_slices(depth, self.slice_sample_rate)

    def _build_program(self, ctx: Ctx, n_img: int, h: int, w: int) -> VGGLossProgram:
        return VGGLossProgram(ctx, self._convs, self.feature_layers, bool(self.use_l1), n_img, h, w)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor) or pred.dim() != 5:
            raise ValueError("VGGPerceptualLoss expects two (B, 1, D, H, W) tensors")
        if pred.shape != target.shape:
            raise ValueError(f"shape mismatch: pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
        if pred.shape[1] != 1:
            raise AssertionError("Expected grayscale input (C=1)")
        if pred.numel() == 0:
            raise ValueError("VGGPerceptualLoss got an empty tensor")
        if pred.shape[3] % 16 or pred.shape[4] % 16:
            raise ValueError(f"H and W must be multiples of 16 (the stack halves them four times), got H={pred.shape[3]}, "
                             f"W={pred.shape[4]}")
        if not pred.is_cuda or not target.is_cuda:
            raise CtsiError("VGGPerceptualLoss runs on the HIP engine: pass ROCm tensors (there is no CPU path in the product; "
                            "tests/vgg_restatement.py is test infrastructure)")
        p = pred.to(torch.float32).contiguous()             # outside the Function: autograd carries dtype and layout
        t = target.detach().to(torch.float32).contiguous()
        return _VGGLossFn.apply(p, t, self, torch.is_grad_enabled() and p.requires_grad)


def _lpips_head(src, k: int, channels: int) -> Optional[torch.Tensor]:
    """Head k: element k of a sequence, or `lin{k}.model.1.weight` / `lins.{k}.model.1.weight` of a state dict; None if absent."""
    if isinstance(src, dict):
        t = next((src[n] for n in (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight") if n in src), None)
    else:
        t = src[k] if k < len(src) else None
    if t is None:
        return None
    if not torch.is_tensor(t) or t.numel() != channels:
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"LPIPS head {k} has shape {got}, expected (1, {channels}, 1, 1)")
    return t.detach().to(torch.float32).reshape(1, channels, 1, 1).clone()


class _LPIPSFn(torch.autograd.Function):
    """out[i] = the LPIPS distance of image i, (N, 1, 1, 1); backward gives in0's gradient from the per-image upstream."""

    @staticmethod
    def forward(fctx, in0, in1, owner, normalize, want_grad):
        ctx = Ctx.get(in0.device)
        n, c, h, w = in0.shape
        with ctx.scope():
            prog = owner._take_program(ctx, n, h, w)
            out = prog.run_forward(in0, in1, (c, bool(normalize)))
        owner.last_layer_means = out[n:]
        if want_grad:
            fctx.prog, fctx.owner, fctx.generation, fctx.args = prog, owner, prog.generation, (c, bool(normalize))
        else:
            owner._give_program(prog)          # every use is ordered on the engine stream
        return out[:n].reshape(n, 1, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(fctx, grad_out):
        prog = _owned_program(fctx, "LPIPS")
        with prog.ctx.scope():
            g = grad_out.detach().to(torch.float32).reshape(-1).contiguous()
            grad = prog.run_backward(g, fctx.args, fctx.generation)
        _hand_back(fctx, prog)
        return grad, None, None, None, None


class LPIPS(_ProgramPool, nn.Module):
    """The `lpips` package's distance (0.1.x, net='vgg', spatial=False, eval mode), forward and backward on the HIP engine.

    `weights`: a state dict (or a path to one, `torch.load(..., weights_only=True)`) of torchvision's VGG-16
    (`features.{i}.weight / bias`), of its `features` (`{i}. ...`) or of an `lpips.LPIPS` (`net.slice{k}.{i}. ...`).  The five
    heads come from `lin_weights` -- five tensors of C = 64, 128, 256, 512, 512 weights, or a state dict with
    `lin{k}.model.1.weight` / `lins.{k}.model.1.weight` -- or from `weights` when it carries those keys; `lpips=False` uses
    all-ones heads (the package's baseline mode).  Negative head weights are accepted: the package does not clamp at inference.
    `weights=None` raises `NotImplementedError`: the engine neither imports `lpips` / torchvision nor downloads, and no weights
    ship with the project.

    `forward(in0, in1, normalize=False)`: (N, 1 | 3, H, W) in [-1, 1] ([0, 1] with `normalize`) -> (N, 1, 1, 1), the
    package's contract (a one-channel image is its grey value in all three channels); (B, 1, D, H, W) volumes -> the scalar
    mean over the slices `slices` selects: 'middle' (D // 2, the VAE trainer's rule), 'all', or a float rate with
    `VGGPerceptualLoss.slice_indices`' expression; the gradient is exactly zero on the other slices.  The gradient is computed
    for `in0` only.  `last_layer_means` holds the five tap means over the batch of the latest forward as a device tensor."""

    CHANNELS = (64, 128, 256, 512, 512)

    def __init__(self, net: str = 'vgg', *, weights: Optional[Union[Dict[str, torch.Tensor], str, "os.PathLike"]] = None,
                 lin_weights=None, lpips: bool = True, slices: Union[str, float] = 'middle', spatial: bool = False):
        if net != 'vgg':
            raise ValueError(f"LPIPS: only net='vgg' runs on the HIP engine (the strided 11x11 and fire-module stacks of 'alex' "
                             f"and 'squeeze' are out of scope), got {net!r}")
        if spatial:
            raise ValueError("LPIPS: spatial=True (a distance map per image) is not implemented; the distance is one value per image")
        if weights is None:
            raise NotImplementedError(
                "LPIPS needs pre-trained VGG-16 weights and linear heads, which the lpips package fetches through torchvision "
                "from the network; the HIP engine does neither.  Pass them: LPIPS(weights=<state dict or path of an "
                "lpips.LPIPS(net='vgg'), or of torchvision's vgg16 / vgg16().features plus lin_weights=...>) (DESIGN.md section "
                "30), or use MS_SSIM_Loss.")
        if not (slices in ('middle', 'all') or (isinstance(slices, (int, float)) and not isinstance(slices, bool) and slices >= 0)):
            raise ValueError(f"slices must be 'middle', 'all' or a non-negative sampling rate, got {slices!r}")
        super().__init__()
        sd = _vgg_state_dict(weights)
        self.slices = slices
        self.lpips = bool(lpips)
        self._convs = _frozen_convs(sd, VGG16_MODULES, "VGG-16", ("net.slice<k>.{idx}.{kind}",))
        self.net = nn.ModuleList(self._convs.values())
        heads = []
        for k, c in enumerate(self.CHANNELS):
            if not self.lpips:
                t = torch.ones(1, c, 1, 1)
            else:
                src = _vgg_state_dict(lin_weights) if isinstance(lin_weights, (str, os.PathLike)) else lin_weights
                t = _lpips_head(src, k, c) if src is not None else _lpips_head(sd, k, c)
                if t is None:
                    raise ValueError(f"LPIPS head {k} is missing: pass lin_weights (five tensors, or a state dict with "
                                     f"'lin{k}.model.1.weight'), weights that carry those keys, or lpips=False")
            heads.append(nn.Parameter(t, requires_grad=False))
        self.lins = nn.ParameterList(heads)
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self.register_buffer('shift', torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1))
        self.register_buffer('scale', torch.tensor([.458, .448, .450]).view(1, 3, 1, 1))
        self.last_layer_means = None

    def slice_indices(self, depth: int) -> torch.Tensor:
        """The selected slices of a volume of `depth` slices (host, int64)."""
        if self.slices == 'middle':
            return torch.tensor([depth // 2], dtype=torch.long)
        if self.slices == 'all':
            return torch.arange(depth, dtype=torch.long)
        return _rate_slices(depth, self.slices)

    def _build_program(self, ctx: Ctx, n_img: int, h: int, w: int) -> VGGLossProgram:
        return VGGLossProgram(ctx, self._convs, list(LPIPS_TAPS), False, n_img, h, w, modules=VGG16_MODULES, distance="lpips",
                              heads=list(self.lins))

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        if not isinstance(in0, torch.Tensor) or not isinstance(in1, torch.Tensor) or in0.dim() not in (4, 5):
            raise ValueError("LPIPS expects two (N, 1 | 3, H, W) images or two (B, 1, D, H, W) volumes")
        if in0.shape != in1.shape:
            raise ValueError(f"shape mismatch: in0 {tuple(in0.shape)} vs in1 {tuple(in1.shape)}")
        if in0.shape[1] not in ((1, 3) if in0.dim() == 4 else (1,)):
            raise ValueError(f"LPIPS expects 1 or 3 channels (volumes: 1), got C={in0.shape[1]}")
        if in0.numel() == 0:
            raise ValueError("LPIPS got an empty tensor")
        if in0.shape[-2] % 16 or in0.shape[-1] % 16:
            raise ValueError(f"H and W must be multiples of 16 (the stack halves them four times), got H={in0.shape[-2]}, "
                             f"W={in0.shape[-1]}")
        if not in0.is_cuda or not in1.is_cuda:
            raise CtsiError("LPIPS runs on the HIP engine: pass ROCm tensors (there is no CPU path in the product; "
                            "tests/lpips_restatement.py is test infrastructure)")
        grad = torch.is_grad_enabled()
        if grad and in1.requires_grad:
            raise CtsiError("LPIPS computes the gradient for `in0` only; `in1` requires grad -- detach it")
        in1 = in1.detach()
        volume = in0.dim() == 5
        if volume:
            # the selected slices as images, sample-major; autograd's scatter leaves exact zeros on the other slices
            b, _, d, h, w = in0.shape
            idx = self.slice_indices(d).to(in0.device)
            in0 = in0.index_select(2, idx).permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
            in1 = in1.index_select(2, idx).permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
        p = in0.to(torch.float32).contiguous()              # outside the Function: autograd carries dtype and layout
        t = in1.to(torch.float32).contiguous()
        out = _LPIPSFn.apply(p, t, self, bool(normalize), grad and p.requires_grad)
        return out.mean() if volume else out


class MS_SSIM_Loss(nn.Module):
    """1 - MS-SSIM of two (B, C, D, H, W) volumes in [-1, 1], slice by slice, differentiable in `pred`.

    Args as the reference's: window_size (odd, at most 15), size_average (only True is defined: the reference's per-image
    form fails unless B * D is 1 or 5), channel (must equal the tensors' C).  `last_level_means` holds the five level
    means of the latest forward as a device tensor.
    """

    def __init__(self, window_size: int = 11, size_average: bool = True, channel: int = 1):
        super().__init__()
        if not isinstance(window_size, int) or window_size < 1 or window_size % 2 == 0 or window_size > MAX_WINDOW:
            raise ValueError(f"window_size must be an odd integer in [1, {MAX_WINDOW}], got {window_size!r}")
        if not isinstance(channel, int) or channel < 1:
            raise ValueError(f"channel must be a positive integer, got {channel!r}")
        self.window_size = window_size
        self.size_average = size_average
        self.channel = channel
        self.window = self._create_window(window_size, channel)
        self.last_level_means = None

    def _gaussian_window(self, window_size: int, sigma: float = 1.5) -> torch.Tensor:
        gauss = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / (2.0 * sigma ** 2)) for x in range(window_size)],
                             dtype=torch.float32)
        # the normaliser is the correctly rounded fp32 sum, as csrc/msssim.hip forms it: torch's own `gauss.sum()` gives the
        # same bits for every odd size up to 13 (so the default window is the reference's, bit for bit) and one ulp more at 15
        return gauss / gauss.double().sum().float()

    def _create_window(self, window_size: int, channel: int) -> torch.Tensor:
        """(channel, 1, window_size, window_size) fp32: the outer product of the normalised 1-D Gaussian.  The kernels
        apply the same 1-D window separably; this attribute is the reference's, kept for callers that read it."""
        g = self._gaussian_window(window_size).unsqueeze(1)
        return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, window_size, window_size).contiguous()

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor) or pred.dim() != 5:
            raise ValueError("MS_SSIM_Loss expects two (B, C, D, H, W) tensors")
        if pred.shape != target.shape:
            raise ValueError(f"shape mismatch: pred {tuple(pred.shape)} vs target {tuple(target.shape)}")
        if pred.shape[1] != self.channel:
            raise ValueError(f"the loss was built for channel={self.channel}, got C={pred.shape[1]}")
        if min(pred.shape[3], pred.shape[4]) < MIN_SIZE:
            raise ValueError(f"five levels need min(H, W) >= {MIN_SIZE}, got H={pred.shape[3]}, W={pred.shape[4]}")
        if pred.numel() == 0:
            raise ValueError("MS_SSIM_Loss got an empty tensor")
        if not self.size_average:
            raise NotImplementedError("size_average=False is not defined: the reference's per-image form raises a shape error "
                                      "in `mssim ** weights` unless B * D is 1 or 5; use size_average=True")
        if not pred.is_cuda or not target.is_cuda:
            raise CtsiError("MS_SSIM_Loss runs on the HIP engine: pass ROCm tensors (there is no CPU path in the product; "
                            "tests/msssim_restatement.py is test infrastructure)")
        grad = torch.is_grad_enabled()
        if grad and target.requires_grad:
            raise CtsiError("MS_SSIM_Loss computes the gradient for `pred` only; `target` requires grad -- detach it")
        p = pred.to(torch.float32).contiguous()             # outside the Function: autograd carries dtype and layout
        t = target.detach().to(torch.float32).contiguous()
        return _MSSSIMFn.apply(p, t, self.window_size, grad and p.requires_grad, self)


class CombinedLoss(nn.Module):
    """diffusion loss + lambda_perceptual * VGG perceptual + lambda_ssim * MS-SSIM, the auxiliary terms every N steps
    (reference losses.py:279-361).  Both auxiliary terms are the device losses above.  The perceptual term needs VGG-19
    weights the constructor has no argument for (its signature is the reference's): assign
    `c.perceptual_loss = VGGPerceptualLoss(weights=...)` before the term is first due.  Otherwise it is built when first due
    and raises `NotImplementedError` then, which leaves `lambda_perceptual=0` as the setting that needs no weights."""

    def __init__(self, lambda_perceptual: float = 0.1, lambda_ssim: float = 0.1, perceptual_every_n_steps: int = 10,
                 ssim_every_n_steps: int = 10):
        super().__init__()
        self.lambda_perceptual = lambda_perceptual
        self.lambda_ssim = lambda_ssim
        self.perceptual_every_n_steps = perceptual_every_n_steps
        self.ssim_every_n_steps = ssim_every_n_steps
        self.perceptual_loss = None
        self.ssim_loss = MS_SSIM_Loss()
        self.register_buffer('step', torch.tensor(0, dtype=torch.long))

    def forward(self, pred: torch.Tensor, target: torch.Tensor, diffusion_loss: torch.Tensor,
                compute_auxiliary: bool = True) -> Tuple[torch.Tensor, dict]:
        loss_dict = {'diffusion': diffusion_loss.item()}
        total_loss = diffusion_loss
        if compute_auxiliary:
            step = int(self.step)
            if step % self.perceptual_every_n_steps == 0 and self.lambda_perceptual > 0:
                if self.perceptual_loss is None:
                    self.perceptual_loss = VGGPerceptualLoss()
                perceptual = self.perceptual_loss(pred, target)
                total_loss = total_loss + self.lambda_perceptual * perceptual
                loss_dict['perceptual'] = perceptual.item()
            if step % self.ssim_every_n_steps == 0 and self.lambda_ssim > 0:
                ssim = self.ssim_loss(pred, target)
                total_loss = total_loss + self.lambda_ssim * ssim
                loss_dict['ssim'] = ssim.item()
        self.step += 1
        loss_dict['total'] = total_loss.item()
        return total_loss, loss_dict


def auxiliary_due(c) -> bool:
    """Whether `c(pred, target, diffusion_loss)` would evaluate an auxiliary term at its current `step`: CombinedLoss.forward's
    own two conditions, read without advancing the step.  The diffusion stage (VideoToVideoDiffusion.image_loss, DESIGN section
    27) asks before it builds `pred`: a decode with its backward tape is not worth building for a step that drops it.  Any
    other callable is always due."""
    if not isinstance(c, CombinedLoss):
        return True
    step = int(c.step)
    return bool((c.lambda_perceptual > 0 and step % c.perceptual_every_n_steps == 0) or
                (c.lambda_ssim > 0 and step % c.ssim_every_n_steps == 0))
