"""Test infrastructure: the MS-SSIM loss of the reference (models/losses.py:149-276) restated in plain torch ops, dtype a
parameter, usable on any device.  Written from the formulas, pinned to the reference by
tests/test_oracle_msssim_golden.py; the yardstick (fp32) and the truth (fp64) of tests/test_gpu_msssim.py."""
import math

import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window_2d(window_size=11, sigma=1.5):
    """The fp32 window: 1-D Gaussian divided in fp32 by the correctly rounded fp32 sum of its values (torch's own fp32 sum
    has the same bits for every odd size up to 13; the default 11 is pinned to the reference by the goldens), outer product
    in fp32."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / (2.0 * sigma ** 2)) for x in range(window_size)],
                     dtype=torch.float32)
    g = (g / g.double().sum().float()).unsqueeze(1)
    return g.mm(g.t())


def msssim_loss(pred, target, dtype=torch.float32, window_size=11, return_means=False):
    """1 - prod_i mean_i ** w_i over five levels; pred, target (B, C, D, H, W) in [-1, 1]."""
    h, w = pred.shape[-2:]
    a = (pred.to(dtype).reshape(-1, 1, h, w) + 1.0) / 2.0
    b = (target.to(dtype).reshape(-1, 1, h, w) + 1.0) / 2.0
    win = window_2d(window_size).to(device=pred.device, dtype=dtype)[None, None]
    pad, c1, c2 = window_size // 2, 0.01 ** 2, 0.03 ** 2
    means = []
    for level in range(len(WEIGHTS)):
        mu1, mu2 = F.conv2d(a, win, padding=pad), F.conv2d(b, win, padding=pad)
        s1 = F.conv2d(a * a, win, padding=pad) - mu1 * mu1
        s2 = F.conv2d(b * b, win, padding=pad) - mu2 * mu2
        s12 = F.conv2d(a * b, win, padding=pad) - mu1 * mu2
        ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
        means.append(ssim.mean())
        if level + 1 < len(WEIGHTS):
            a, b = F.avg_pool2d(a, 2, 2), F.avg_pool2d(b, 2, 2)
    means = torch.stack(means)
    weights = torch.tensor(WEIGHTS, dtype=torch.float32, device=pred.device).to(dtype)
    loss = 1.0 - (means ** weights).prod()
    return (loss, means) if return_means else loss


def smooth_pair(shape, noise, seed, device="cpu"):
    """The goldens' input recipe: target = a trilinearly upsampled coarse random field (one node per 6 pixels, per 2 slices)
    x 1.2 clamped to [-1, 1], pred = clamp(target + noise * randn).  With noise 0.1 the fp32 restatement gives level means
    >= 0.89 at every shape the tests use (level 0: 0.89 - 0.91), far from the pole of mean ** w."""
    g = torch.Generator().manual_seed(seed)
    b, c, d, h, w = shape
    coarse = torch.randn(b, c, max(d // 2, 2), max(h // 6, 2), max(w // 6, 2), generator=g)
    target = (F.interpolate(coarse, size=(d, h, w), mode="trilinear", align_corners=False) * 1.2).clamp(-1, 1)
    pred = (target + noise * torch.randn(shape, generator=g)).clamp(-1, 1)
    return pred.to(device), target.to(device)
