"""Latent window fusion on the README's stitching case: an 8 x 512 x 512 thick volume, (8,192,192) ->
(48,192,192) patches at stride (4,96,96) = 25 windows, DDIM-10, bf16.

  1. wall time per volume of fusion='pixel', fusion='latent' decode='full' and decode='windows', alternated in one process
     (host clock around a call that ends in a device synchronise; the first round is the warm-up and is not counted);
  2. the captured step (hipGraph replay, device events) of the fused program next to the plain 25-window step program;
  3. ctsi_window_blend and ctsi_window_gather at that shape: in place inside an eager step (an event pair per launch, the
     caches holding the network's last activations) and back to back (cache-warm); algorithmic bytes / time;
  4. torch.cuda.max_memory_allocated around the fused run, and the U-Net activation pool per window it implies;
  5. with --parent-tree DIR (a checkout of the parent commit with its library built): the DEFAULT path timed in fresh child
     processes parent / this / parent, the check that the default path costs what it did.

Usage: python tools/fused_stitch_bench.py [--reps 3] [--steps 10] [--parent-tree DIR] [--out profiles/fused_stitch_bench.log]
"""
import argparse
import ctypes as C
import importlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = dict(patch_size=(8, 192, 192), target_patch_size=(48, 192, 192), stride=(4, 96, 96))

# the default path of whichever tree is the working directory: one warm-up call, then `reps` timed calls
DEFAULT_SNIPPET = r"""
import importlib, os, sys, time
sys.path.insert(0, os.getcwd())
os.environ.setdefault("CTSI_PROGRAM_CACHE", "8")
import torch
import bench
pkg = importlib.import_module("video-to-video-diffusion_amd")
reps, steps = int(sys.argv[1]), int(sys.argv[2])
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = pkg.VideoToVideoDiffusion(bench.EFFECTIVE_CFG).eval().to(dev)
sampler = pkg.DDIMSampler(model.diffusion, model.unet)
v = (torch.rand(1, 1, 8, 512, 512) * 2 - 1).to(dev)
times = []
for rep in range(reps + 1):
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sampler.sample_with_stitching(v, model.vae, steps, patch_size=(8, 192, 192), target_patch_size=(48, 192, 192),
                                        stride=(4, 96, 96), device=dev, progress=False)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
print("DEFAULT", " ".join(f"{t:.4f}" for t in times[1:]), "checksum", float(out.double().sum()))
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_stitch_bench.log"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def child(tree):
        p = subprocess.run([sys.executable, "-c", DEFAULT_SNIPPET, str(args.reps), str(args.steps)], cwd=tree,
                           capture_output=True, text=True, timeout=600)
        row = [ln for ln in p.stdout.splitlines() if ln.startswith("DEFAULT")]
        if p.returncode != 0 or not row:
            raise SystemExit(f"default-path child in {tree} failed:\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
        return row[0]

    say(f"# fused_stitch_bench: 8x512x512 thick volume, 25 windows, DDIM-{args.steps}, bf16, {args.reps} timed rounds")
    if args.parent_tree:
        say("## default path (no new arguments), fresh child processes, seconds per volume per round")
        for label, tree in (("parent", args.parent_tree), ("this", ROOT), ("parent", args.parent_tree)):
            say(f"{label:7s} {child(tree)}")

    # the three modes keep six VAE programs alive between rounds (two window batches of encoder and decoder, the whole-volume
    # decoder): more than the default of four cached programs per module, which would rebuild one in every timed call
    os.environ.setdefault("CTSI_PROGRAM_CACHE", "8")
    say("(CTSI_PROGRAM_CACHE=%s programs cached per module, in the child processes too)" % os.environ["CTSI_PROGRAM_CACHE"])
    sys.path.insert(0, ROOT)
    import torch
    import bench
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(bench.EFFECTIVE_CFG).eval().to(dev)
    sampler = pkg.DDIMSampler(model.diffusion, model.unet)
    v = (torch.rand(1, 1, 8, 512, 512) * 2 - 1).to(dev)
    modes = [("pixel", {}), ("latent/full", dict(fusion="latent")), ("latent/windows", dict(fusion="latent", decode="windows"))]
    wall = {m: [] for m, _ in modes}
    peak = {}
    for rep in range(args.reps + 1):
        for mode, kw in modes:
            torch.manual_seed(1)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = sampler.sample_with_stitching(v, model.vae, args.steps, device=dev, progress=False, **GEO, **kw)
            torch.cuda.synchronize()
            if rep:
                wall[mode].append(time.perf_counter() - t0)
            peak[mode] = torch.cuda.max_memory_allocated()
            assert tuple(out.shape) == (1, 1, 48, 512, 512) and bool(torch.isfinite(out).all()), mode
            del out
    say("## wall time per volume, alternated in one process (seconds per round; min)")
    for mode, _ in modes:
        say(f"{mode:15s} {' '.join(f'{t:.4f}' for t in wall[mode])}   min {min(wall[mode]):.4f}   "
            f"peak allocated during the call {peak[mode] / 2 ** 30:.2f} GiB")

    # ---- the captured steps ------------------------------------------------------------------------------------------
    fused = next(p for k, p in model.unet._ctsi_programs.items() if k[0] == "sampler-fused")
    lib, ctx = fused.lib, fused.ctx

    def events(n):
        evs = []
        for _ in range(n):
            e = C.c_void_p()
            lib.event_create(C.byref(e))
            evs.append(e)
        return evs

    def timed(fn, n, reset=None):
        """Mean milliseconds of `n` calls of fn on the engine stream between two events (3 untimed calls first)."""
        a, b = events(2)
        best = None
        for _ in range(3):
            with ctx.scope():
                if reset is not None:
                    reset()
                for _ in range(3):
                    fn()
                lib.event_record(a, ctx.sptr)
                for _ in range(n):
                    fn()
                lib.event_record(b, ctx.sptr)
            torch.cuda.synchronize()
            ms = C.c_float()
            lib.event_elapsed_ms(a, b, C.byref(ms))
            best = ms.value / n if best is None else min(best, ms.value / n)
        lib.event_destroy(a)
        lib.event_destroy(b)
        return best

    n_ev = args.steps
    t_fused = timed(fused.launch, n_ev, reset=lambda: fused.step_ptr.zero_())
    say("## captured step (one hipGraph replay = one U-Net evaluation of all 25 windows + update), device events, best of 3")
    say(f"fused step        {t_fused:8.3f} ms   ({len(fused.ops)} launches: {fused.unet_op_count} network + "
        f"{len(fused.ops) - fused.unet_op_count} behind it)")
    torch.manual_seed(1)
    sampler.sample_with_stitching(v, model.vae, args.steps, device=dev, progress=False, window_batch=25, **GEO)
    plain = next(p for k, p in model.unet._ctsi_programs.items() if k[0] == "sampler" and k[2] == 25)
    t_plain = timed(plain.launch, n_ev, reset=lambda: plain.step_ptr.zero_())
    say(f"plain 25-window   {t_plain:8.3f} ms   ({len(plain.ops)} launches)")
    say(f"fused - plain     {t_fused - t_plain:+8.3f} ms   ({(t_fused / t_plain - 1) * 100:+.2f} % of the plain step)")

    # ---- the two kernels alone ---------------------------------------------------------------------------------------
    # in place: an event pair around every launch of 5 eager steps (Program.profile_ops, what bench.py's per-op table uses), so
    # each of the two runs right after a whole U-Net evaluation has streamed through the caches.  Back to back: 200 launches
    # between two events; their 114 / 88 MB may stay in the last-level cache, so that rate is NOT an HBM rate.
    say("## the new kernels at this shape: in place inside an eager step (event pair per launch, mean of 5 steps), and 200")
    say("## launches back to back (best of 3; buffers may stay in the last-level cache: not an HBM rate); algorithmic bytes / time")
    with ctx.scope():
        fused.step_ptr.zero_()
        per_op = fused.profile_ops(repeats=5)
    torch.cuda.synchronize()
    for name in ("window.blend", "window.gather"):
        i = [m[0] for m in fused.op_meta].index(name)
        ms_in = per_op[i][3]
        ms = timed(fused.ops[i], 200)
        nbytes = fused.op_bytes[i]
        say(f"{name:14s} in place {ms_in * 1e3:7.1f} us = {nbytes / (ms_in * 1e-3) / 1e12:5.2f} TB/s ({ms_in / t_fused * 100:.2f} % of "
            f"the fused step)   back to back {ms * 1e3:7.1f} us = {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s   {nbytes / 1e6:6.1f} MB")

    # ---- memory ------------------------------------------------------------------------------------------------------
    nw = fused.nw
    keep = sum(t.numel() * t.element_size() for t in fused.keep if torch.is_tensor(t))
    say("## memory of the fused U-Net step program (25 windows of 48 x 48 x 48 latent, one network batch)")
    say(f"activation pool   {fused.pool.total_bytes / 2 ** 30:6.2f} GiB = {fused.pool.total_bytes / nw / 2 ** 20:7.1f} MiB per window")
    say(f"persistent        {keep / 2 ** 30:6.2f} GiB (inputs, state, timestep tables for {fused.max_rows} rows, workspaces)")
    say(f"peak allocated    pixel {peak['pixel'] / 2 ** 30:.2f} GiB, latent/full {peak['latent/full'] / 2 ** 30:.2f} GiB, "
        f"latent/windows {peak['latent/windows'] / 2 ** 30:.2f} GiB (torch.cuda.max_memory_allocated over one call, programs cached)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
