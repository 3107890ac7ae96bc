"""A torch restatement of ctsi_volume_metrics (csrc/volume_metrics.hip) for the tests: the zero-padded separable window applied
with F.conv3d -- w, then h, then d -- to the five moment fields a, b, a^2, b^2, ab, then slice_metrics_kernel's SSIM formula,
then the means over every axis but the table's.  In float64 it is the reference; the same code in float32 is the noise
yardstick of the tolerance (tests/test_gpu_volume_metrics_ops.py)."""
import numpy as np
import torch
import torch.nn.functional as F

# The kernel's per-slice SSIM may be TOL_FACTOR times as far from float64 as this restatement run in float32 is on the same
# input (another, equally valid summation order differs by a small multiple), and never needs to be nearer than TOL_FLOOR, the
# bound tests/test_gpu_network.py holds ctsi_slice_metrics to.  Measured ratios: profiles/volume_metrics_tests.log
TOL_FACTOR = 4.0
TOL_FLOOR = 2e-6
MSE_RTOL = 1e-12        # fp64 sums of exact fp32 differences


def tolerance(err32: float) -> float:
    return max(TOL_FLOOR, TOL_FACTOR * err32)


AXIS = {"axial": 0, "coronal": 1, "sagittal": 2, "volumetric": 0}


def radii_of(mode: str, window_size: int, window_depth=None):
    R = window_size // 2
    if mode == "volumetric":
        return ((window_size if window_depth is None else window_depth) // 2, R, R)
    return tuple(0 if i == AXIS[mode] else R for i in range(3))


def window_weights(size: int, window: str, sigma: float = 1.5) -> np.ndarray:
    """float64 weights of one axis: box 1 / size, gaussian exp(-(i - R)^2 / (2 sigma^2)) normalised to sum 1."""
    if window == "box":
        return np.full(size, 1.0 / size, dtype=np.float64)
    x = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def ssim_map(a: torch.Tensor, b: torch.Tensor, radii, window: str = "box", sigma: float = 1.5, max_val: float = 1.0,
             dtype=torch.float64) -> torch.Tensor:
    """(n, c, d, h, w) tensors -> the SSIM map of the same shape, every operation in `dtype`."""
    a, b = a.to(dtype), b.to(dtype)
    n, c, d, h, w = a.shape
    m = torch.stack([a, b, a * a, b * b, a * b]).reshape(5 * n * c, 1, d, h, w)
    for axis in (2, 1, 0):                                     # w, h, d
        r = radii[axis]
        if r == 0:
            continue
        shape, pad = [1, 1, 1, 1, 1], [0, 0, 0]
        shape[2 + axis], pad[axis] = 2 * r + 1, r
        g = torch.from_numpy(window_weights(2 * r + 1, window, sigma)).to(device=a.device, dtype=dtype).reshape(shape)
        m = F.conv3d(m, g, padding=pad)
    mu1, mu2, e11, e22, e12 = m.reshape(5, n, c, d, h, w)
    v1, v2, v12 = (e11 - mu1 * mu1).clamp(min=0), (e22 - mu2 * mu2).clamp(min=0), e12 - mu1 * mu2
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    s = ((2 * mu1 * mu2 + c1) * (2 * v12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (v1 + v2 + c2) + 1e-8)
    return s.clamp(0, 1)


def volume_metrics(a, b, radii, axis: int, window: str = "box", sigma: float = 1.5, max_val: float = 1.0,
                   dtype=torch.float64, ssim: bool = True):
    """-> (mse per index of `axis`, SSIM per index of `axis` or None), float64 CPU arrays; the squared differences are
    always summed in float64."""
    dims = [i for i in range(5) if i != 2 + axis]
    mse = (a.double() - b.double()).pow(2).mean(dim=dims).cpu().numpy()
    if not ssim:
        return mse, None
    s = ssim_map(a, b, radii, window, sigma, max_val, dtype)
    return mse, s.double().mean(dim=dims).cpu().numpy()


def smooth_pair(shape, seed: int, device="cpu"):
    """A smooth random field in [0, 1] (low-pass filtered randn, rescaled) plus noise, and b = a + 0.05 noise, clamped."""
    g = torch.Generator().manual_seed(seed)
    n, c, d, h, w = shape
    x = torch.randn((n * c, 1, d, h, w), generator=g, dtype=torch.float64)
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64) / 16.0
    for _ in range(2):
        for axis in range(3):
            ks, pad = [1, 1, 1, 1, 1], [0, 0, 0]
            ks[2 + axis], pad[axis] = 5, 2
            x = F.conv3d(F.pad(x, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]), mode="replicate"), k.reshape(ks))
    x = (x - x.amin()) / (x.amax() - x.amin()).clamp(min=1e-12)
    a = (0.9 * x + 0.1 * torch.rand(x.shape, generator=g, dtype=torch.float64)).clamp(0, 1).reshape(shape).float()
    b = (a + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    return a.to(device), b.to(device)
