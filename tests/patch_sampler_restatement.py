"""The definition of the device patch sampler, in torch on the CPU.

  * `replay_draw`: the `random.Random` calls of the reference's extract_random_patch + augment_patch, in their order;
  * `item`: data_contract.aligned_patch at the drawn position, then torch.flip / torch.flip / torch.rot90 -- the reference's
    own composition, on the reference's own F.interpolate;
  * `depth_resample_f64`: the thick resample with PyTorch's source-index formula evaluated in fp32 (the weights are then the
    very fp32 numbers the kernel uses) and the blend w0 a + w1 b in float64;
  * `batch`: what DevicePatchSampler.sample must return for the rows of DevicePatchSampler.draw.

Bounds the tests hold the kernel to: the thin patch is a gather, so it is bit-identical (for fp16 storage: float(half(x)));
the thick patch differs from the float64 blend only by the roundings of w0 a + w1 b in fp32 -- at most two roundings of
values below 1 for inputs in [-1, 1] -- so |error| <= THICK_TOL = 2^-22.
"""
import importlib
import random

import numpy as np
import torch

DC = importlib.import_module("video-to-video-diffusion_amd.data_contract")
DD = importlib.import_module("video-to-video-diffusion_amd.device_data")

THICK_TOL = 2.0 ** -22


def replay_draw(rng: random.Random, d_thin, h, w, depth_thin, ph, pw, augment):
    """(z, y0, x0, flip_w, flip_h, k) drawn from `rng` exactly as the reference's dataset draws them from `random`."""
    y0 = rng.randint(0, h - ph)
    x0 = rng.randint(0, w - pw)
    z = rng.randint(0, d_thin - depth_thin) if d_thin >= depth_thin else 0
    fw = fh = False
    k = 0
    if augment:
        fw = rng.random() > 0.5
        fh = rng.random() > 0.5
        k = rng.randint(0, 3)
    return z, y0, x0, fw, fh, k


def augment(t: torch.Tensor, fw, fh, k) -> torch.Tensor:
    """augment_patch on a (1, D, H, W) patch."""
    if fw:
        t = torch.flip(t, dims=[3])
    if fh:
        t = torch.flip(t, dims=[2])
    if k > 0:
        t = torch.rot90(t, k=k, dims=[2, 3])
    return t


def item(thick, thin, z, y0, x0, fw, fh, k, depth_thin, depth_thick, ph, pw):
    """(thick patch, thin patch) fp32, the reference's item at these draws."""
    tk, tn = DC.aligned_patch(thick, thin, z, y0, x0, depth_thin, depth_thick, (ph, pw))
    return augment(tk, fw, fh, k).contiguous(), augment(tn, fw, fh, k).contiguous()


def depth_weights(n_sub: int, depth_thick: int):
    """(i0, i1, w0, w1) per output slice: PyTorch's align_corners=False source index, every step in fp32."""
    scale = np.float32(n_sub) / np.float32(depth_thick)
    out = []
    for j in range(depth_thick):
        s = scale * (np.float32(j) + np.float32(0.5)) - np.float32(0.5)
        s = max(s, np.float32(0.0))
        i0 = min(int(s), n_sub - 1)
        i1 = min(i0 + 1, n_sub - 1)
        w1 = np.float32(s - np.float32(i0))
        out.append((i0, i1, float(np.float32(1.0) - w1), float(w1)))
    return out


def depth_resample_f64(sub: torch.Tensor, depth_thick: int) -> torch.Tensor:
    """(1, n_sub, H, W) -> (1, depth_thick, H, W) float64: fp32 weights, float64 blend."""
    sub = sub.double()
    return torch.stack([w0 * sub[:, i0] + w1 * sub[:, i1] for i0, i1, w0, w1 in depth_weights(sub.shape[1], depth_thick)], 1)


def stored(v: torch.Tensor, dtype) -> torch.Tensor:
    """The values a DeviceVolumeStore of `dtype` holds, as fp32."""
    return v.to(dtype).float()


def batch(volumes, rows: torch.Tensor, depth_thin, depth_thick, ph, pw, dtype=torch.float32, with_thick=True):
    """(thick float64 (n, 1, Dk, ph, pw) or None, thin fp32 (n, 1, Dt, ph, pw)) for rows of DevicePatchSampler.draw;
    `volumes`: [(thick (1, D, H, W) or None, thin)] on the CPU, as they were added to the store."""
    thicks, thins = [], []
    for r in rows.tolist():
        thick, thin = volumes[r[DD.C_VOL]]
        z, y0, x0, k0, k1, fl = r[DD.C_Z], r[DD.C_Y0], r[DD.C_X0], r[DD.C_K0], r[DD.C_K1], r[DD.C_FLAGS]
        fw, fh, k = bool(fl & 1), bool(fl & 2), fl >> 2
        z1 = min(z + depth_thin, thin.shape[1])
        tn = stored(thin[:, z:z1, y0:y0 + ph, x0:x0 + pw], dtype)
        if tn.shape[1] < depth_thin:
            tn = torch.nn.functional.pad(tn, (0, 0, 0, 0, 0, depth_thin - tn.shape[1]), value=-1.0)
        thins.append(augment(tn, fw, fh, k))
        if with_thick:
            sub = stored(thick[:, k0:k1, y0:y0 + ph, x0:x0 + pw], dtype)
            thicks.append(augment(depth_resample_f64(sub, depth_thick), fw, fh, k))
    return (torch.stack(thicks).contiguous() if with_thick else None), torch.stack(thins).contiguous()


class HostStore:
    """The host half of a DeviceVolumeStore -- shapes, categories, ids -- over CPU volumes: what `draw` and the loader need.
    Test infrastructure only (tests/test_host_patch_sampler.py); the product has no CPU path."""

    def __init__(self, volumes, dtype=torch.float32):
        self.volumes, self.dtype = list(volumes), dtype
        self.categories = [f"cat{i % 2}" for i in range(len(self.volumes))]
        self.patient_ids = [f"p{i}" for i in range(len(self.volumes))]

    def __len__(self):
        return len(self.volumes)

    def shape(self, i):
        thick, thin = self.volumes[i]
        return int(thin.shape[1]), 0 if thick is None else int(thick.shape[1]), int(thin.shape[2]), int(thin.shape[3])


def host_sampler(volumes, **kw):
    """A DevicePatchSampler over a HostStore whose `sample` is the restatement (fp32 on the CPU)."""
    s = DD.DevicePatchSampler.__new__(DD.DevicePatchSampler)
    real_store = DD.DeviceVolumeStore.__new__(DD.DeviceVolumeStore)      # passes the constructor's type check; never used
    DD.DevicePatchSampler.__init__(s, real_store, **kw)
    s.store = HostStore(volumes)

    def sample(rows):
        thick, thin = batch(volumes, rows, s.depth_thin, s.depth_thick, s.ph, s.pw)
        return thick.float(), thin

    s.sample = sample
    return s
