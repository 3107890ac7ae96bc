"""What ensemble sampling costs, variants ALTERNATED in one process:

  --mode kernels   on the config-2 volume (1,1,48,512,512): ctsi_ensemble_accumulate for rows 1 and 4 (first call and a later
                   one), ctsi_ensemble_finalize and ctsi_ensemble_calibration, each beside ctsi_nan_to_num_f32 on the same
                   buffer, the existing one-read-one-write pass (the streaming floor DESIGN section 28 compares against).  Each
                   timing spans --reps back-to-back calls.  us per call, the bytes of the traffic formula ((rows + 4) * 4 per
                   element, (rows + 2) * 4 on the first call; 8 for finalize; 12 for calibration), TB/s and the ratio to the
                   floor per byte.
  --mode ensemble  BASELINE config 1 ((1,1,8,192,192) -> 48 slices, DDIM-10) and config 2 ((1,1,8,512,512) -> 48 slices,
                   DDIM-50), the production model with random weights: generate_ensemble(K = 4 and 8) against the hand-written
                   loop -- K generate() calls, torch.stack, .mean(0) / .std(0) -- time and peak device memory of each.
                   `--configs 1` / `--configs 2` restricts it; `--variant ensemble` / `--variant loop` with `--members 8` runs one
                   variant alone, so that its peak memory does not count the other's cached programs.
  --mode default   generate() of config 2 only; `--root DIR` imports the package from another checkout (a build of the parent
                   commit), so that parent / this / parent runs bracket the default path.

    python tools/ensemble_bench.py --mode kernels >> profiles/ensemble_bench.log"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402

DEV = "cuda:0"


def _root(argv):
    for i, a in enumerate(argv):
        if a == "--root" and i + 1 < len(argv):
            return os.path.abspath(argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ROOT = _root(sys.argv)
sys.path.insert(0, ROOT)
from tests.helpers import FULL_CFG, formula_input     # noqa: E402


def alternate(variants, rounds, warmup, reps=1, after=None):
    """variants: [(name, fn)] -> {name: times in ms per call, in round order}; `reps` back-to-back calls per event pair;
    `after(name)` runs once per timed call after the synchronisation (peak-memory bookkeeping)."""
    times = {name: [] for name, _ in variants}
    for rnd in range(warmup + rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if after is not None:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if after is not None:
                after(name)
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) / reps)
    return times


def kernels_mode(a, pkg):
    lib = pkg.get_lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(5)
    shape = (1, 1, 48, 512, 512)
    n = 48 * 512 * 512
    x = (torch.rand((4,) + shape, generator=gen) * 2 - 1).to(DEV)
    mean, m2, std = (torch.empty(shape, device=DEV) for _ in range(3))
    target = (torch.rand(shape, generator=gen) * 2 - 1).to(DEV)
    lib.ensemble_accumulate(p(x), 4, n, 0, p(mean), p(m2), sp)            # a valid state for the later calls
    planes, plane = 48, 512 * 512
    partials = torch.empty(lib.ensemble_blocks(planes, plane) * 4, dtype=torch.float64, device=DEV)
    table = torch.empty((planes, 4), dtype=torch.float64, device=DEV)
    variants = [
        ("ctsi_nan_to_num_f32", lambda: lib.nan_to_num_f32(p(mean), n, sp), 8),
        ("ctsi_ensemble_accumulate rows 1, first call", lambda: lib.ensemble_accumulate(p(x), 1, n, 0, p(mean), p(m2), sp), 12),
        ("ctsi_ensemble_accumulate rows 1, seen 4", lambda: lib.ensemble_accumulate(p(x), 1, n, 4, p(mean), p(m2), sp), 20),
        ("ctsi_ensemble_accumulate rows 4, first call", lambda: lib.ensemble_accumulate(p(x), 4, n, 0, p(mean), p(m2), sp), 24),
        ("ctsi_ensemble_accumulate rows 4, seen 4", lambda: lib.ensemble_accumulate(p(x), 4, n, 4, p(mean), p(m2), sp), 32),
        ("ctsi_ensemble_finalize (two launches)", lambda: lib.ensemble_finalize(p(m2), p(std), 8, 1, planes, plane, p(partials),
                                                                                p(table), sp), 8),
        ("ctsi_ensemble_calibration (two launches)", lambda: lib.ensemble_calibration(p(mean), p(std), p(target), planes, plane,
                                                                                      p(partials), p(table), sp), 12),
    ]
    times = alternate([(k, f) for k, f, _ in variants], a.rounds, a.warmup, a.reps)
    print(f"[kernels, volume {shape} = {n / 1e6:.1f} M voxels] {a.rounds} alternated rounds after {a.warmup} warm-up; {a.reps} "
          f"back-to-back calls per timing, time per call; bytes from the traffic formula")
    floor = None
    for k, _, bpe in variants:
        s = sorted(times[k])
        med, nbytes = s[len(s) // 2], bpe * n
        per_byte = med / nbytes
        floor = per_byte if floor is None else floor
        print(f"  ({k:46s}) min {1e3 * s[0]:8.1f} us  median {1e3 * med:8.1f} us  max {1e3 * s[-1]:8.1f} us   {bpe:2d} B/voxel = "
              f"{nbytes / 1e6:7.1f} MB -> {nbytes / (med * 1e-3) / 1e12:5.2f} TB/s at the median   {per_byte / floor:5.2f} x the "
              f"nan_to_num pass per byte ({100 * floor / per_byte:5.1f} % of its per-byte rate)")


def _model(pkg):
    torch.manual_seed(0)
    return pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)


def _noise_fn():
    gen = torch.Generator(device=DEV).manual_seed(3)
    return lambda i, shape: torch.randn(shape, generator=gen, device=DEV)


def show(name, ts, peak=None):
    s = sorted(ts)
    mem = "" if peak is None else f"   peak memory {peak / 2 ** 30:7.2f} GiB"
    print(f"  ({name:44s}) median {s[len(s) // 2]:9.2f} ms   min {s[0]:9.2f}  max {s[-1]:9.2f}   spread "
          f"{100 * (s[-1] - s[0]) / s[0]:.2f} %{mem}")
    return s[len(s) // 2]


def ensemble_mode(a, pkg):
    model = _model(pkg)
    members = [int(k) for k in a.members.split(",")]
    for cfg, hw, steps in ((1, 192, 10), (2, 512, 50)):
        if str(cfg) not in a.configs.split(","):
            continue
        v_in = formula_input((1, 1, 8, hw, hw), 18).clamp(-1, 1).to(DEV)
        kw = dict(num_inference_steps=steps, target_depth=48)
        peaks, variants = {}, []
        for K in members:
            def ens(K=K):
                gen = torch.Generator(device=DEV).manual_seed(3)
                model.generate_ensemble(v_in, "ddim", num_members=K,
                                        member_noise_fn=lambda k, i, s: torch.randn(s, generator=gen, device=DEV), **kw)

            def loop(K=K):
                outs = [model.generate(v_in, "ddim", noise_fn=_noise_fn(), **kw) for _ in range(K)]
                st = torch.stack(outs)
                return st.mean(0), st.std(0)

            if a.variant in ("both", "ensemble"):
                variants.append((f"generate_ensemble K={K}", ens))
            if a.variant in ("both", "loop"):
                variants.append((f"loop of generate() + stack/mean/std K={K}", loop))
        base = torch.cuda.memory_allocated()

        def after(name):
            peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated() - base)

        times = alternate(variants, a.rounds, a.warmup, after=after)
        print(f"[config {cfg}: (1,1,8,{hw},{hw}) -> 48 slices, DDIM-{steps}, production model, random weights] {a.rounds} alternated "
              f"rounds after {a.warmup} warm-up; peak memory above the {base / 2 ** 30:.2f} GiB held before (weights; cached programs "
              f"are built in the warm-up and counted)")
        med = {k: show(k, ts, peaks[k]) for k, ts in times.items()}
        for K in members if a.variant == "both" else ():
            e, l = med[f"generate_ensemble K={K}"], med[f"loop of generate() + stack/mean/std K={K}"]
            print(f"  K={K}: generate_ensemble takes {100 * e / l:.1f} % of the loop's time ({e / K:.2f} ms against {l / K:.2f} ms per member)")
        model.invalidate_engine_cache()
        torch.cuda.empty_cache()


def default_mode(a, pkg):
    model = _model(pkg)
    v_in = formula_input((1, 1, 8, 512, 512), 18).clamp(-1, 1).to(DEV)
    times = alternate([("generate()", lambda: model.generate(v_in, "ddim", num_inference_steps=50, target_depth=48,
                                                             noise_fn=_noise_fn()))], a.rounds, a.warmup)
    print(f"[default path, package from {os.path.relpath(ROOT)}] config-2 generate(), DDIM-50, {a.rounds} rounds after {a.warmup} warm-up")
    show("generate()", times["generate()"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "ensemble", "default"), default="kernels")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="--mode kernels: back-to-back calls per event pair")
    ap.add_argument("--configs", default="1,2", help="--mode ensemble: which BASELINE configs")
    ap.add_argument("--members", default="4,8", help="--mode ensemble: the ensemble sizes K")
    ap.add_argument("--variant", choices=("both", "ensemble", "loop"), default="both",
                    help="--mode ensemble: one variant alone gives its peak memory without the other's cached programs")
    ap.add_argument("--root", default=None, help="import the package from this checkout instead of the tool's own")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench.py measures on a ROCm device; none is available")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print(f"device {torch.cuda.get_device_name(0)}; mode {a.mode}; HIP events, host launch included")
    {"kernels": kernels_mode, "ensemble": ensemble_mode, "default": default_mode}[a.mode](a, pkg)


if __name__ == "__main__":
    main()
