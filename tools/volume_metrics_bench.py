"""What the volume metrics cost, variants ALTERNATED in one process on random volumes in [0, 1]:

  at (1,1,48,512,512): ctsi_nan_to_num_f32 on one volume (the one-read-one-write streaming pass the README uses as its
  yardstick), ctsi_slice_metrics (the old axial kernel, window 11), ctsi_volume_metrics in every mode at window 11, box and
  gaussian, the axial mode also at windows 3 and 15 (does the time follow the taps or the bytes?), the float32 restatement of
  each mode as torch ops on the device (tests/volume_metrics_restatement.py), and calculate_volume_metrics with its defaults
  (four launches pairs and the host's read of the tables);
  at (1,1,300,512,512): the axial mode and the old kernel.

Each timing spans --reps back-to-back calls.  us per call, useful bytes (2 x 4 B per voxel read) per second, the ratio to the
nan_to_num pass per byte, and the peak device memory above the inputs of one call.

    python tools/volume_metrics_bench.py >> profiles/volume_metrics_bench.log"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import volume_metrics_restatement as VR     # noqa: E402


def alternate(variants, rounds, warmup, reps):
    """variants: [(name, fn, reps or None)] -> {name: ms per call in round order}, {name: peak bytes above what was held}."""
    times, peaks = {name: [] for name, _, _ in variants}, {}
    for rnd in range(warmup + rounds):
        for name, fn, own in variants:
            r = own or reps
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(r):
                fn()
            e1.record()
            torch.cuda.synchronize()
            peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated() - base)
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) / r)
    return times, peaks


def report(title, variants, times, peaks, voxels, floor_name):
    print(title)
    floor = None
    for name, _, _ in variants:
        s = sorted(times[name])
        med = s[len(s) // 2]
        nbytes = 8 * voxels
        if name == floor_name:
            floor = med
        rel = "" if floor is None else f"   {med / floor:7.2f} x the nan_to_num pass"
        print(f"  ({name:50s}) min {1e3 * s[0]:9.1f} us  median {1e3 * med:9.1f} us  max {1e3 * s[-1]:9.1f} us   spread "
              f"{100 * (s[-1] - s[0]) / s[0]:5.1f} %   {nbytes / (med * 1e-3) / 1e12:6.3f} TB/s useful{rel}   peak memory "
              f"{peaks[name] / 2 ** 20:9.1f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-deep", action="store_true", help="skip the 300-slice volume")
    a = ap.parse_args()
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    MT = importlib.import_module("video-to-video-diffusion_amd.metrics")
    lib = pkg.get_lib()
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"device {torch.cuda.get_device_name(0)}; HIP events, host launch included; {a.rounds} alternated rounds after "
          f"{a.warmup} warm-up; {a.reps} back-to-back calls per timing (torch restatement and public function: 1)")
    for shape in ((1, 1, 48, 512, 512),) + (() if a.no_deep else ((1, 1, 300, 512, 512),)):
        deep = shape[2] > 48
        n, c, d, h, w = shape
        voxels = n * c * d * h * w
        gen = torch.Generator().manual_seed(11)
        va = torch.rand(shape, generator=gen).to(DEV)
        vb = (va + 0.05 * torch.randn(shape, generator=gen).to(DEV)).clamp_(0, 1)
        scratch = va.clone()
        gw = {k: torch.from_numpy(MT.gaussian_window(k, 1.5).astype(np.float32)).to(DEV) for k in (1, 3, 11, 15)}
        ws_old = torch.empty(lib.slice_metrics_workspace_doubles(n, c, d, h, w), dtype=torch.float64, device=DEV)
        out_old = torch.empty((d, 4), dtype=torch.float64, device=DEV)

        def vm(mode, window, size):
            radii, axis = VR.radii_of(mode, size), VR.AXIS[mode]
            ws = torch.empty(lib.volume_metrics_workspace_doubles(n, c, d, h, w, *radii), dtype=torch.float64, device=DEV)
            out = torch.empty((shape[2 + axis], 4), dtype=torch.float64, device=DEV)
            g = [gw[2 * r + 1] if window == "gaussian" else None for r in radii]
            return lambda: lib.volume_metrics(p(va), p(vb), n, c, d, h, w, radii[0], radii[1], radii[2], p(g[0]), p(g[1]), p(g[2]),
                                              axis, 1.0, p(ws), p(out), sp)

        def restate(mode, window):
            radii, axis = VR.radii_of(mode, 11), VR.AXIS[mode]
            dims = [i for i in range(5) if i != 2 + axis]
            return lambda: (VR.ssim_map(va, vb, radii, window, dtype=torch.float32).mean(dim=dims), (va - vb).pow(2).mean(dim=dims))

        variants = [("ctsi_nan_to_num_f32 (one volume: 8 B/voxel)", lambda: lib.nan_to_num_f32(p(scratch), voxels, sp), None)]
        if d * n * c <= 65535:
            variants.append(("ctsi_slice_metrics window 11 (old axial kernel)",
                             lambda: lib.slice_metrics(p(va), p(vb), n, c, d, h, w, 11, 1.0, p(ws_old), p(out_old), sp), None))
        variants.append(("ctsi_volume_metrics axial box 11", vm("axial", "box", 11), None))
        if not deep:
            variants += [("ctsi_volume_metrics axial box 3", vm("axial", "box", 3), None),
                         ("ctsi_volume_metrics axial box 15", vm("axial", "box", 15), None),
                         ("ctsi_volume_metrics axial gaussian 11", vm("axial", "gaussian", 11), None)]
            for mode in ("coronal", "sagittal", "volumetric"):
                variants += [(f"ctsi_volume_metrics {mode} box 11", vm(mode, "box", 11), None),
                             (f"ctsi_volume_metrics {mode} gaussian 11", vm(mode, "gaussian", 11), None)]
            variants.append(("ctsi_volume_metrics sagittal box 3", vm("sagittal", "box", 3), None))
            variants.append(("ctsi_volume_metrics volumetric box 3", vm("volumetric", "box", 3), None))
            for mode in ("axial", "coronal", "sagittal", "volumetric"):
                variants.append((f"float32 restatement as torch ops, {mode} box 11", restate(mode, "box"), 1))
            variants.append(("calculate_volume_metrics(a, b): 4 modes + host read", lambda: MT.calculate_volume_metrics(va, vb), 1))
        else:
            variants.append(("float32 restatement as torch ops, axial box 11", restate("axial", "box"), 1))
        times, peaks = alternate(variants, a.rounds, a.warmup, a.reps)
        report(f"[volume {shape} = {voxels / 1e6:.1f} M voxels, useful bytes = 8 B/voxel = {8 * voxels / 1e6:.1f} MB]", variants,
               times, peaks, voxels, variants[0][0])
        del va, vb, scratch, ws_old, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
