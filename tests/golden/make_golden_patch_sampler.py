"""Writes tests/golden/patch_sampler_v1.npz: items of the reference's PatchSliceInterpolationDataset on tiny volumes.

    python tests/golden/make_golden_patch_sampler.py /path/to/video-to-video-diffusion

The reference's dataset module is loaded by file path (its `data/__init__` pulls in the DICOM loader).  A few tiny patient
files are written to a temporary directory; for fixed `random.seed` values the items `ds[idx]` are recorded with augment on
and off.  The fixture holds the volumes, the seeds and the outputs, nothing else:

    vol{v}_thick, vol{v}_thin     fp32 (1, D, H, W)
    cases                         int64 (n, 3): volume, seed, augment
    thick, thin                   fp32 (n, 1, 2, 8, 8) and (n, 1, 12, 8, 8): ds[idx]['input'], ds[idx]['target']
    config                        int64: patch_depth_thin, patch_depth_thick, ph, pw

The volumes: 0 is shallower than the patch (D_thin 9 < 12: padding); 1 has 2 thick slices for 40 thin ones (the thick range
collapses to one slice, n_sub = 1); 2 has D_thin == 12 and 3 thick slices (the range ends at D_thick); 3 has H != W and W odd.
"""
import importlib.util
import os
import random
import sys
import tempfile

import numpy as np
import torch

DEPTH_THIN, DEPTH_THICK, PH, PW = 12, 2, 8, 8
SHAPES = [(2, 9, 12, 12), (2, 40, 11, 12), (3, 12, 8, 8), (4, 20, 10, 13)]       # (D_thick, D_thin, H, W)
SEEDS = (0, 1, 2, 3, 5, 8)


def main(reference_root):
    path = os.path.join(reference_root, "data", "patch_slice_interpolation_dataset.py")
    spec = importlib.util.spec_from_file_location("ref_patch_dataset", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(1234)
    vols = [(torch.rand((1, dk, h, w), generator=g) * 2 - 1, torch.rand((1, dt, h, w), generator=g) * 2 - 1)
            for dk, dt, h, w in SHAPES]
    out = {"config": np.array([DEPTH_THIN, DEPTH_THICK, PH, PW], dtype=np.int64)}
    cases, thick, thin = [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        for v, (tk, tn) in enumerate(vols):
            out[f"vol{v}_thick"], out[f"vol{v}_thin"] = tk.numpy(), tn.numpy()
            torch.save({"input": tk, "target": tn, "category": "c", "patient_id": str(v)}, os.path.join(tmp, f"case_{v:03d}.pt"))
        for aug in (0, 1):
            ds = mod.PatchSliceInterpolationDataset(tmp, DEPTH_THIN, DEPTH_THICK, (PH, PW), split="train", val_ratio=0.0,
                                                    test_ratio=0.0, augment=bool(aug))
            for idx in range(len(ds)):
                for seed in SEEDS:
                    random.seed(seed)
                    it = ds[idx]
                    cases.append((int(it["patient_id"]), seed, aug))
                    thick.append(it["input"].contiguous().numpy())
                    thin.append(it["target"].contiguous().numpy())
    out["cases"] = np.array(cases, dtype=np.int64)
    out["thick"], out["thin"] = np.stack(thick), np.stack(thin)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "patch_sampler_v1.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(cases)} items, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
