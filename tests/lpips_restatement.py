"""Test infrastructure: the LPIPS distance (lpips 0.1.x, net='vgg', lpips=True, spatial=False, eval mode) as plain torch ops,
written from its five steps and not from the package, which the engine must not depend on:

  1. scaling layer      x_c = (in_c - shift_c) / scale_c
  2. VGG-16 `features`  modules 0..29 as torchvision numbers them; taps = the ReLU outputs 3, 8, 15, 22, 29
  3. unit normalisation a = sqrt(sum_c y_c^2), u = y / (a + 1e-10), per tap and per position, for both inputs
  4. tap value          d_tap[i] = mean over positions of sum_c w_c (u_c - v_c)^2, w the tap's (1, C, 1, 1) head
  5. result             out[i] = sum over the taps of d_tap[i], shape (N, 1, 1, 1)

float64 gives the truth of the GPU tests; the same code under bf16 autocast is their yardstick.  `widths` shrinks the stack
(the same module order, fewer channels) for gradcheck.  Weights are He-normal from a fixed seed, heads random and non-negative;
nothing is loaded from outside.
"""
import math

import torch
import torch.nn as nn

CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512]
TAPS = (3, 8, 15, 22, 29)
CHANNELS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
EPS = 1e-10


def make_cfg(widths=None):
    """CFG with the five stage widths replaced (64, 128, 256, 512, 512 by default)."""
    if widths is None:
        return list(CFG)
    out, stage = [], 0
    for v in CFG:
        if v == "M":
            out.append("M")
            stage += 1
        else:
            out.append(widths[stage])
    return out


def make_features(widths=None) -> nn.Sequential:
    mods, cin = [], 3
    for v in make_cfg(widths):
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods.extend([nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)])
            cin = v
    assert len(mods) == 30
    return nn.Sequential(*mods)


def he_state_dict(seed: int, prefix: str = "", widths=None) -> dict:
    """He-normal conv weights (std = sqrt(2 / fan_in)) and 0.05 * randn biases under `{prefix}{i}.weight / bias`."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for i, m in enumerate(make_features(widths)):
        if isinstance(m, nn.Conv2d):
            cout = m.out_channels
            sd[f"{prefix}{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
            sd[f"{prefix}{i}.bias"] = 0.05 * torch.randn(cout, generator=g)
            cin = cout
    return sd


def random_heads(seed: int, widths=None) -> list:
    """Five non-negative (1, C, 1, 1) heads, of the size the trained ones have (a few of them exactly zero)."""
    g = torch.Generator().manual_seed(seed)
    heads = []
    for c in (widths or CHANNELS):
        w = torch.rand(1, c, 1, 1, generator=g) * (64.0 / c)
        w[:, ::7] = 0.0
        heads.append(w)
    return heads


def lpips_state_dict(sd: dict, heads: list) -> dict:
    """The same weights under an lpips.LPIPS state dict's names: net.slice{k}.{i}.*, lin{k}.model.1.weight."""
    out, k = {}, 1
    for i in sorted({int(n.split(".")[0]) for n in sd}):
        while i > TAPS[k - 1]:
            k += 1
        for kind in ("weight", "bias"):
            out[f"net.slice{k}.{i}.{kind}"] = sd[f"{i}.{kind}"]
    for j, w in enumerate(heads):
        out[f"lin{j}.model.1.weight"] = w
    return out


def tap_distance(y: torch.Tensor, t: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """steps 3 and 4 for one tap: (N, C, H, W) features and a (1, C, 1, 1) head -> (N,)"""
    u = y / (torch.sqrt(torch.sum(y ** 2, dim=1, keepdim=True)) + EPS)
    v = t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + EPS)
    return (w * (u - v) ** 2).sum(dim=1).mean(dim=(1, 2))


class Restatement:
    """out = Restatement(sd, heads)(in0, in1): (N, 3 | 1, H, W) in [-1, 1] -> (N, 1, 1, 1); the gradient reaches in0 only."""

    def __init__(self, sd: dict, heads, dtype=torch.float64, device="cpu", widths=None):
        feats = make_features(widths)
        feats.load_state_dict({k: sd.get(k, sd.get("features." + k)).clone() for k in feats.state_dict()})
        self.feats = feats.to(device=device, dtype=dtype).eval()
        for p in self.feats.parameters():
            p.requires_grad = False
        self.heads = [w.to(device=device, dtype=dtype).reshape(1, -1, 1, 1) for w in heads]
        self.dtype, self.device = dtype, device
        self.shift = torch.tensor(SHIFT, dtype=dtype, device=device).view(1, 3, 1, 1)
        self.scale = torch.tensor(SCALE, dtype=dtype, device=device).view(1, 3, 1, 1)

    def taps(self, x: torch.Tensor) -> list:
        out = []
        for i, m in enumerate(self.feats):
            x = m(x)
            if i in TAPS:
                out.append(x)
        return out

    def tap_values(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False, autocast: bool = False) -> list:
        """the five (N,) tensors d_tap"""
        a, b = in0.to(self.dtype), in1.to(self.dtype)
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        if a.shape[1] == 1:
            a, b = a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1)
        a, b = (a - self.shift) / self.scale, (b - self.shift) / self.scale
        with torch.autocast(in0.device.type, dtype=torch.bfloat16, enabled=autocast):
            with torch.no_grad():
                tf = self.taps(b)
            pf = self.taps(a)
            vals = []
            for y, t, w in zip(pf, tf, self.heads):
                vals.append(tap_distance(y, t, w))
        return vals

    def __call__(self, in0, in1, normalize: bool = False, autocast: bool = False) -> torch.Tensor:
        vals = self.tap_values(in0, in1, normalize, autocast)
        return sum(v.to(self.dtype) if not autocast else v.float() for v in vals).reshape(-1, 1, 1, 1)


def volume_loss(r: Restatement, pred: torch.Tensor, target: torch.Tensor, idx, autocast: bool = False) -> torch.Tensor:
    """The module's 5-D contract: the mean of the per-image values over the slices `idx` of (B, 1, D, H, W) volumes."""
    b, _, d, h, w = pred.shape
    idx = torch.as_tensor(idx, dtype=torch.long, device=pred.device)
    p = pred.index_select(2, idx).permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    t = target.index_select(2, idx).permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    return r(p, t, autocast=autocast).mean()


def make_pair(shape, seed: int):
    """target in [-1, 1] and pred = target + 0.3 * noise"""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, generator=g) * 2 - 1
    return target + 0.3 * torch.randn(shape, generator=g), target
