"""Test infrastructure: a torch-ops restatement of the reference's VGGPerceptualLoss (models/losses.py:22-146), written from
its description because the reference module itself imports torchvision, which the engine must not depend on.

VGG-19 `features` is built from its configuration list as an nn.Sequential of Conv2d(3 x 3, pad 1), ReLU(inplace=True) and
MaxPool2d(2, 2) -- module indices 0-36 as torchvision numbers them, convs at 0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30,
32, 34 -- and cut into blocks `features[prev : idx + 1]`.  The in-place ReLUs are kept in place and the loss is taken after all
blocks have run, so a block output that the next block's leading ReLU overwrites is compared post-ReLU, as in the reference.
float64 gives the truth of the GPU tests; the same code under bf16 autocast is their yardstick.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34)
DEFAULT_LAYERS = (2, 7, 12, 21, 30)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_features() -> nn.Sequential:
    mods, cin = [], 3
    for v in CFG:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods.extend([nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)])
            cin = v
    return nn.Sequential(*mods)


def he_state_dict(seed: int, upto: int = 36, prefix: str = "") -> dict:
    """He-normal weights (std = sqrt(2 / fan_in)) and 0.05 * randn biases for the convs up to module `upto`, under
    `{prefix}{i}.weight / bias`: activations stay O(1) through the whole stack."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for i, m in enumerate(make_features()):
        if i > upto:
            break
        if isinstance(m, nn.Conv2d):
            cout = m.out_channels
            sd[f"{prefix}{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cin * 9))
            sd[f"{prefix}{i}.bias"] = 0.05 * torch.randn(cout, generator=g)
            cin = cout
    return sd


def slice_indices(depth: int, rate: float) -> torch.Tensor:
    num = max(1, int(depth * rate))
    return torch.linspace(0, depth - 1, num, dtype=torch.long) if num < depth else torch.arange(depth)


def to_rgb(x: torch.Tensor, rate: float) -> torch.Tensor:
    """(B, 1, D, H, W) in [-1, 1] -> (B * num, 3, H, W) normalised for VGG; the slices of sample b are images b num .. b num + num - 1."""
    b, c, d, h, w = x.shape
    assert c == 1, "Expected grayscale input (C=1)"
    num = max(1, int(d * rate))
    if num < d:
        x = x[:, :, torch.linspace(0, d - 1, num, dtype=torch.long, device=x.device)]
    x = x.permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    x = ((x + 1.0) / 2.0).repeat(1, 3, 1, 1)
    mean = torch.tensor(MEAN, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


class Restatement:
    """The loss for one set of weights: `sd` holds `{i}.weight / bias` (or `features.{i}. ...`) for the convs the layers need."""

    def __init__(self, sd: dict, feature_layers=DEFAULT_LAYERS, use_l1: bool = True, rate: float = 0.2,
                 dtype=torch.float64, device="cpu"):
        feats = make_features()
        own = feats.state_dict()
        for k in own:
            src = sd.get(k, sd.get("features." + k))
            if src is not None:
                own[k] = src.clone()
            elif int(k.split(".")[0]) <= max(feature_layers):
                raise KeyError(k)
        feats.load_state_dict(own)
        feats = feats.to(device=device, dtype=dtype).eval()
        for p in feats.parameters():
            p.requires_grad = False
        self.blocks, prev = [], 0
        for idx in feature_layers:
            self.blocks.append(feats[prev:idx + 1])
            prev = idx + 1
        self.use_l1, self.rate, self.dtype = use_l1, rate, dtype

    def features(self, rgb: torch.Tensor) -> list:
        out, x = [], rgb
        for block in self.blocks:
            x = block(x)
            out.append(x)
        return out

    def __call__(self, pred: torch.Tensor, target: torch.Tensor, autocast: bool = False) -> torch.Tensor:
        p, t = to_rgb(pred.to(self.dtype), self.rate), to_rgb(target.to(self.dtype), self.rate)
        with torch.autocast(pred.device.type, dtype=torch.bfloat16, enabled=autocast):
            with torch.no_grad():
                tf = self.features(t)
            pf = self.features(p)
            loss = 0.0
            for a, b in zip(pf, tf):
                loss = loss + (F.l1_loss(a, b) if self.use_l1 else F.mse_loss(a, b))
        return loss / len(self.blocks)


def smooth_volume(shape, seed: int) -> torch.Tensor:
    """A smooth random volume in [-1, 1]: a coarse random field (one node per 6 pixels, per 2 slices) upsampled trilinearly."""
    g = torch.Generator().manual_seed(seed)
    b, c, d, h, w = shape
    coarse = torch.randn(b, c, max(d // 2, 2), max(h // 6, 2), max(w // 6, 2), generator=g)
    return (F.interpolate(coarse, size=(d, h, w), mode="trilinear", align_corners=False) * 1.2).clamp(-1, 1)
