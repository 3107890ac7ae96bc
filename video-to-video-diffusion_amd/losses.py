"""Structural losses of the reference's `models/losses.py` on the HIP engine.

`MS_SSIM_Loss` (losses.py:149-276) is a differentiable loss here: forward and backward are HIP launches
(csrc/msssim.hip) behind a `torch.autograd.Function`, 6 launches forward and 5 backward, with no
host read in either direction.  `CombinedLoss` (losses.py:279-361) keeps the reference's bookkeeping around it.
`VGGPerceptualLoss` needs torchvision and downloaded VGG-19 weights and stays out of scope: it
raises `NotImplementedError`, so `CombinedLoss(lambda_perceptual=0, ...)` is the usable setting.

Semantics of `MS_SSIM_Loss()(pred, target)`, both (B, C, D, H, W) in [-1, 1]: every (b, c, d) plane is an H x W image
of `(v + 1) / 2`; five levels of the full SSIM map under the zero-padded 11 x 11 Gaussian window (sigma 1.5), the
level value is the mean over all planes and pixels, a 2 x 2 average pool (floor) between levels,
`loss = 1 - prod_i mean_i ** w_i`.  A negative level mean gives NaN for the loss and every gradient element, as
torch's `pow` does in the reference.  The gradient is computed for `pred` only.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .engine import Ctx, _ptr
from .lib import CtsiError

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


class VGGPerceptualLoss(nn.Module):
    """Not available: the reference's perceptual loss needs torchvision and downloaded VGG-19 weights."""

    def __init__(self, feature_layers: list = [2, 7, 12, 21, 30], use_l1: bool = True, slice_sample_rate: float = 0.2):
        raise NotImplementedError(
            "VGGPerceptualLoss needs torchvision and pre-trained VGG-19 weights fetched from the network; it is out of "
            "scope for the HIP engine (DESIGN.md section 7).  Use CombinedLoss(lambda_perceptual=0, ...) or MS_SSIM_Loss.")


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
    (reference losses.py:279-361).  The SSIM term is the device loss above.  The perceptual term is built when it is first
    due and raises `NotImplementedError` then: `lambda_perceptual=0` is the usable setting on this engine."""

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
