"""Validation metrics on device (mirror of reference utils/metrics.py:14-193).

`Trainer.validate*` and the evaluation scripts call these right after `generate`; here the per-slice squared error
and the 11x11 box-window SSIM map are reduced by one HIP launch over the whole volume (ctsi_slice_metrics), and only
the per-slice scalars come back to the host, where the reference's clamps / dB conversion are applied.
Return types and edge cases follow the reference: python floats, PSNR clamped to [0, 100] with the MSE floored at
1e-8, SSIM 0.0 when NaNs are present, `calculate_video_metrics` returning zeros + empty lists on NaN inputs.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List

import numpy as np
import torch

from .engine import Ctx, _ptr
from .lib import CtsiError


def _as_device_f32(t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise CtsiError("metrics run on the HIP engine: pass ROCm tensors (there is no CPU path in the product; "
                        "the oracle under oracle/ is test infrastructure)")
    return t.detach().to(torch.float32).contiguous()


def _slice_stats(a5: torch.Tensor, b5: torch.Tensor, window: int, max_val: float) -> np.ndarray:
    """(n,c,d,h,w) fp32 device tensors -> float64 array (d, 4): mse, mean ssim, nan count a, nan count b."""
    n, c, d, h, w = a5.shape
    ctx = Ctx.get(a5.device)
    out = torch.empty((d, 4), dtype=torch.float64, device=a5.device)
    with ctx.scope():
        ws = torch.empty(max(ctx.lib.slice_metrics_workspace_doubles(n, c, d, h, w), 1), dtype=torch.float64,
                         device=a5.device)
        ctx.lib.slice_metrics(_ptr(a5), _ptr(b5), n, c, d, h, w, int(window), float(max_val), _ptr(ws), _ptr(out),
                              ctx.sptr)
    return out.cpu().numpy()


def _psnr_from_mse(mse: float, max_val: float) -> float:
    mse = max(float(np.float32(mse)), 1e-8)
    return float(min(max(20.0 * math.log10(max_val / math.sqrt(mse)), 0.0), 100.0))


def calculate_psnr(img1, img2, max_val=1.0) -> float:
    """PSNR in dB over all elements of two equally shaped tensors (metrics.py:14-45)."""
    a, b = _as_device_f32(img1), _as_device_f32(img2)
    if a.shape != b.shape:
        raise ValueError(f"shape mismatch: {tuple(a.shape)} vs {tuple(b.shape)}")
    cols = a.shape[-1] if a.dim() else 1
    rows = a.numel() // max(cols, 1)
    st = _slice_stats(a.reshape(1, 1, 1, rows, cols), b.reshape(1, 1, 1, rows, cols), 1, max_val)
    if st[0, 2] > 0 or st[0, 3] > 0:
        return float("nan")
    return _psnr_from_mse(st[0, 0], max_val)


def calculate_ssim(img1, img2, window_size=11, max_val=1.0) -> float:
    """Mean box-window SSIM of (B,C,H,W) images or, slice by slice, of (B,C,D,H,W) volumes (metrics.py:48-121)."""
    a, b = _as_device_f32(img1), _as_device_f32(img2)
    if a.shape != b.shape or a.dim() not in (4, 5):
        raise ValueError(f"expected two (B,C,H,W) or (B,C,D,H,W) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dim() == 4:
        a, b = a.unsqueeze(2), b.unsqueeze(2)
    st = _slice_stats(a, b, window_size, max_val)
    vals = [0.0 if (r[2] > 0 or r[3] > 0) else float(r[1]) for r in st]
    return sum(vals) / len(vals) if vals else 0.0


def calculate_video_metrics(video1, video2, max_val=1.0) -> Dict[str, object]:
    """Per-frame and mean PSNR / SSIM of (B,C,T,H,W) or (C,T,H,W) volumes (metrics.py:124-193)."""
    a, b = _as_device_f32(video1), _as_device_f32(video2)
    if a.dim() == 4:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.shape != b.shape or a.dim() != 5:
        raise ValueError(f"expected two (B,C,T,H,W) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
    st = _slice_stats(a, b, 11, max_val)
    if st[:, 2].sum() > 0 or st[:, 3].sum() > 0:      # NaN anywhere in either volume
        return {'psnr': 0.0, 'ssim': 0.0, 'psnr_per_frame': [], 'ssim_per_frame': []}
    psnr_values: List[float] = [_psnr_from_mse(r[0], max_val) for r in st]
    ssim_values: List[float] = [float(r[1]) for r in st]
    return {'psnr': float(np.mean(psnr_values)) if psnr_values else 0.0,
            'ssim': float(np.mean(ssim_values)) if ssim_values else 0.0,
            'psnr_per_frame': psnr_values, 'ssim_per_frame': ssim_values}


VOLUME_PLANES = {'axial': 0, 'coronal': 1, 'sagittal': 2}     # plane -> the axis its slices are indexed by (d, h, w)
VOLUME_WINDOW_MAX = 15                                        # 2 * 7 + 1: the kernel's largest radius


def gaussian_window(size: int, sigma: float) -> np.ndarray:
    """exp(-(i - R)^2 / (2 sigma^2)), i = 0 .. size - 1, R = size // 2, normalised to sum 1 in float64."""
    x = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return g / g.sum()


def calculate_volume_metrics(video1, video2, max_val=1.0, planes=('axial', 'coronal', 'sagittal'), window_size=11,
                             window='box', sigma=1.5, volumetric=True, window_depth=None) -> Dict[str, object]:
    """PSNR / SSIM of (B,C,D,H,W) or (C,D,H,W) volumes in the three reformats and under a 3-D window
    (ctsi_volume_metrics: the volumes are read in place, no permuted copy).  'axial' slices are (h, w) planes indexed by d,
    'coronal' (d, w) planes indexed by h, 'sagittal' (d, h) planes indexed by w; the window of a plane is window_size x
    window_size inside it.  Each requested plane gives {'psnr', 'ssim', 'psnr_per_slice', 'ssim_per_slice'} (means over the
    plane's slices and the per-slice lists, a slice taken over B and C as calculate_video_metrics does); `volumetric` adds
    'ssim3d' and 'ssim3d_per_slice' (D floats): the same SSIM under a window_depth x window_size x window_size window
    (window_depth defaults to window_size).  window: 'box' (the reference's avg_pool weights) or 'gaussian' (sigma); zero
    padding counts in the window, and a window wider than an axis is legal.  Any NaN in either input gives zeros and empty
    lists in every entry."""
    planes = tuple(planes)
    for name in planes:
        if name not in VOLUME_PLANES:
            raise ValueError(f"unknown plane {name!r}: expected some of {sorted(VOLUME_PLANES)}")
    if window not in ('box', 'gaussian'):
        raise ValueError(f"unknown window {window!r}: expected 'box' or 'gaussian'")
    window_depth = window_size if window_depth is None else window_depth
    for key, val in (('window_size', window_size), ('window_depth', window_depth)):
        if not isinstance(val, int) or val < 1 or val % 2 == 0 or val > VOLUME_WINDOW_MAX:
            raise ValueError(f"{key} must be an odd integer in [1, {VOLUME_WINDOW_MAX}], got {val!r}")
    if window == 'gaussian' and not sigma > 0:
        raise ValueError(f"sigma must be positive, got {sigma!r}")
    if not isinstance(video1, torch.Tensor) or not isinstance(video2, torch.Tensor) or video1.shape != video2.shape \
            or video1.dim() not in (4, 5) or video1.numel() == 0:
        raise ValueError(f"expected two equal (B,C,D,H,W) or (C,D,H,W) tensors, got {tuple(getattr(video1, 'shape', ()))} "
                         f"and {tuple(getattr(video2, 'shape', ()))}")
    a, b = _as_device_f32(video1), _as_device_f32(video2)
    if a.dim() == 4:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    n, c, d, h, w = a.shape
    R, Rd = window_size // 2, window_depth // 2
    # (key, radii, axis) of every launch; all tables land in one device tensor
    jobs = [(name, tuple(0 if i == VOLUME_PLANES[name] else R for i in range(3)), VOLUME_PLANES[name]) for name in planes]
    if volumetric:
        jobs.append(('ssim3d', (Rd, R, R), 0))
    lens = [(d, h, w)[axis] for _, _, axis in jobs]
    if not jobs:
        return {}
    ctx = Ctx.get(a.device)
    table = torch.empty((sum(lens), 4), dtype=torch.float64, device=a.device)
    with ctx.scope():
        gauss = None
        if window == 'gaussian':          # one upload: the weights of both window lengths
            gs, gdp = gaussian_window(window_size, sigma), gaussian_window(window_depth, sigma)
            gauss = torch.from_numpy(np.concatenate([gs, gdp, np.ones(1)]).astype(np.float32)).to(a.device)
            p_s = gauss.data_ptr()                                  # window_size weights | window_depth weights | 1.0 (radius 0)
            p_d, p_1 = p_s + 4 * window_size, p_s + 4 * (window_size + window_depth)
        ws_n = max(ctx.lib.volume_metrics_workspace_doubles(n, c, d, h, w, *radii) for _, radii, _ in jobs)
        ws = torch.empty(max(ws_n, 1), dtype=torch.float64, device=a.device)
        row = 0
        for (key, radii, axis), ln in zip(jobs, lens):
            if gauss is None:
                g = (None, None, None)
            else:
                g = tuple(ctypes.c_void_p(p_1 if r == 0 else (p_d if (i == 0 and key == 'ssim3d') else p_s))
                          for i, r in enumerate(radii))
            ctx.lib.volume_metrics(_ptr(a), _ptr(b), n, c, d, h, w, radii[0], radii[1], radii[2], g[0], g[1], g[2], axis,
                                   float(max_val), _ptr(ws), ctypes.c_void_p(table.data_ptr() + row * 32), ctx.sptr)
            row += ln
    for x in (a, b):
        x.record_stream(ctx.stream)
    st = table.cpu().numpy()
    nan = bool(st[:, 2].sum() > 0 or st[:, 3].sum() > 0)
    out: Dict[str, object] = {}
    row = 0
    for (key, radii, axis), ln in zip(jobs, lens):
        rows, count = st[row:row + ln], float(a.numel() // ln)
        row += ln
        ssim_values: List[float] = [] if nan else [float(r[1] / count) for r in rows]
        ssim_mean = float(np.mean(ssim_values)) if ssim_values else 0.0
        if key == 'ssim3d':
            out['ssim3d'], out['ssim3d_per_slice'] = ssim_mean, ssim_values
            continue
        psnr_values: List[float] = [] if nan else [_psnr_from_mse(r[0] / count, max_val) for r in rows]
        out[key] = {'psnr': float(np.mean(psnr_values)) if psnr_values else 0.0, 'ssim': ssim_mean,
                    'psnr_per_slice': psnr_values, 'ssim_per_slice': ssim_values}
    return out


def measurement_residual(volume, thick, profile) -> Dict[str, List[float]]:
    """How far a thin volume is from reproducing the thick acquisition: W volume (consistency.SliceProfile.measure, on the
    device) against `thick`, per thick slice over (B, C, H, W).  {'rmse': [d_in floats], 'psnr': [d_in floats]}, PSNR in dB at
    data range 2.0 (volumes in [-1, 1]), inf for a slice that is reproduced exactly."""
    v, y = _as_device_f32(volume), _as_device_f32(thick)
    if v.dim() != 5 or y.dim() != 5 or v.shape[2] != profile.d_out or y.shape[2] != profile.d_in \
            or v.shape[:2] != y.shape[:2] or v.shape[3:] != y.shape[3:]:
        raise ValueError(f"expected (B,C,{profile.d_out},H,W) and (B,C,{profile.d_in},H,W) tensors, got {tuple(v.shape)} "
                         f"and {tuple(y.shape)}")
    st = _slice_stats(profile.measure(v).detach(), y, 1, 2.0)
    rmse = [math.sqrt(max(float(r[0]), 0.0)) for r in st]
    return {'rmse': rmse, 'psnr': [20.0 * math.log10(2.0 / e) if e > 0.0 else float("inf") for e in rmse]}


def ensemble_calibration(mean, std, target) -> Dict[str, object]:
    """Can the std map of an ensemble (ensemble.EnsembleResult) be trusted?  (N, C, D, H, W) tensors `mean`, `std` and the
    ground truth `target`; one HIP pass (ctsi_ensemble_calibration) gives per output slice the squared error, the predicted
    variance and how many voxels lie within one and two std of the truth.  Returns, overall and per slice over (N, C, H, W),
    {'rmse', 'rms_std', 'spread_skill' (rms_std / rmse; inf when the error is 0 and the spread is not, nan when both are 0),
    'coverage_1sigma', 'coverage_2sigma'} and the same five as lists of D floats under 'per_slice'.  A calibrated Gaussian
    ensemble gives about 1, 0.68 and 0.95."""
    for name, t in (("mean", mean), ("std", std), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.dim() != 5:
            raise ValueError(f"ensemble_calibration: {name} must be a (N, C, D, H, W) tensor")
    if not (tuple(mean.shape) == tuple(std.shape) == tuple(target.shape)) or mean.numel() == 0:
        raise ValueError(f"ensemble_calibration: shapes differ or are empty: mean {tuple(mean.shape)}, std {tuple(std.shape)}, "
                         f"target {tuple(target.shape)}")
    m, s, t = _as_device_f32(mean), _as_device_f32(std), _as_device_f32(target)
    n, c, d, h, w = m.shape
    planes, plane = n * c * d, h * w
    ctx = Ctx.get(m.device)
    with ctx.scope():
        partials = torch.empty(ctx.lib.ensemble_blocks(planes, plane) * 4, dtype=torch.float64, device=m.device)
        table = torch.empty((planes, 4), dtype=torch.float64, device=m.device)
        ctx.lib.ensemble_calibration(_ptr(m), _ptr(s), _ptr(t), planes, plane, _ptr(partials), _ptr(table), ctx.sptr)
    for x in (m, s, t):
        x.record_stream(ctx.stream)
    per = table.cpu().numpy().reshape(n * c, d, 4).sum(axis=0)        # (d, 4), float64

    def summary(row, voxels):
        rmse, rms_std = math.sqrt(row[0] / voxels), math.sqrt(row[1] / voxels)
        skill = rms_std / rmse if rmse > 0.0 else (float("inf") if rms_std > 0.0 else float("nan"))
        return rmse, rms_std, skill, float(row[2] / voxels), float(row[3] / voxels)

    keys = ('rmse', 'rms_std', 'spread_skill', 'coverage_1sigma', 'coverage_2sigma')
    out = dict(zip(keys, summary(per.sum(axis=0), float(n * c * d * plane))))
    rows = [summary(per[j], float(n * c * plane)) for j in range(d)]
    out['per_slice'] = {k: [r[i] for r in rows] for i, k in enumerate(keys)}
    return out


LPIPS_GROUP = 8        # images per engine call of calculate_lpips: one program, whatever the depth


def calculate_lpips(video1, video2, lpips, max_val=1.0, group: int = LPIPS_GROUP) -> Dict[str, object]:
    """LPIPS (losses.LPIPS, the caller's weights) of every slice of two (B, 1, D, H, W) or (D, H, W) volumes in [0, max_val],
    forward only.  The slices go through the engine in groups of `group` images -- the last group is filled up with repeats of
    the last slice, whose values are dropped -- so one program serves every depth and memory does not grow with D.
    {'lpips': mean over all slices, 'per_slice': [B * D floats, sample-major]}."""
    a, b = _as_device_f32(video1), _as_device_f32(video2)
    if a.dim() == 3:
        a, b = a[None, None], b[None, None]
    if a.shape != b.shape or a.dim() != 5 or a.shape[1] != 1 or a.numel() == 0:
        raise ValueError(f"expected two (B,1,D,H,W) or (D,H,W) volumes, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not (isinstance(group, int) and group > 0) or not max_val > 0:
        raise ValueError(f"group must be a positive integer and max_val positive, got {group!r}, {max_val!r}")
    h, w = a.shape[-2:]
    a, b = (a / max_val).transpose(1, 2).reshape(-1, 1, h, w), (b / max_val).transpose(1, 2).reshape(-1, 1, h, w)
    total = a.shape[0]
    vals = []
    with torch.no_grad():
        for s in range(0, total, group):
            idx = torch.arange(s, s + group, device=a.device).clamp_(max=total - 1)
            vals.append(lpips(a[idx], b[idx], normalize=True).reshape(-1)[:total - s])
    per = torch.cat(vals).double().cpu().tolist()
    return {'lpips': float(np.mean(per)), 'per_slice': per}
