"""What measurement guidance costs, variants ALTERNATED in one process, on the production model with random
weights (no statement about image quality):

  --mode kernels     the three kernels of csrc/measure_guide.hip at config 1 (8 -> 48 slices of 192 x 192) and config 2 (512 x 512):
                     ctsi_guide_z0 and ctsi_guide_apply per byte beside ctsi_nan_to_num_f32 on the same latent buffers;
                     ctsi_depth_residual_adj beside ctsi_nan_to_num_f32 on the decoded volume and beside the passes it replaces,
                     ctsi_depth_measure -> subtract -> ctsi_depth_measure_adj.  Each timing spans --reps back-to-back calls.
  --mode evaluation  what one guided evaluation adds at both configs, piece by piece -- z0 kernel, decode forward, residual
                     kernel, decode backward, apply -- beside the replay of the unguided captured step of the same process, and
                     the peak device memory while the decoder's gradient program is built and run.
  --mode generate    config 1, DDIM-50: generate() unguided, with MeasurementGuidance() (the defaults: the later half of the
                     evaluations) and with every = 5; ||y - W D(z)|| of each result (reported, not judged).
  --mode default     generate() of config 2 without the attribute only; `--root DIR` imports the package from another checkout (a
                     build of the parent commit), so that parent / this / parent runs bracket the default path.

    python tools/measure_guide_bench.py --mode kernels >> profiles/measure_guide_bench.log"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402

DEV = "cuda:0"
CONFIGS = {"config 1": 192, "config 2": 512}


def _root(argv):
    for i, a in enumerate(argv):
        if a == "--root" and i + 1 < len(argv):
            return os.path.abspath(argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ROOT = _root(sys.argv)
sys.path.insert(0, ROOT)
from tests.helpers import FULL_CFG, formula_input     # noqa: E402


def alternate(variants, rounds, warmup, reps=1, before=None):
    """variants: [(name, fn)] -> {name: times in ms per call, in round order}; `reps` back-to-back calls per event pair;
    `before(name)` runs ahead of a variant, outside its event pair"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in variants]
    times = {name: [] for name, _ in variants}
    for rnd in range(warmup + rounds):
        for i, (name, fn) in enumerate(variants):
            if before is not None:
                before(name)
            ev[i][0].record()
            for _ in range(reps):
                fn()
            ev[i][1].record()
        torch.cuda.synchronize()
        if rnd >= warmup:
            for i, (name, _) in enumerate(variants):
                times[name].append(ev[i][0].elapsed_time(ev[i][1]) / reps)
    return times


def med(ts):
    s = sorted(ts)
    return s[len(s) // 2]


def show(name, ts, extra=""):
    s = sorted(ts)
    print(f"  ({name:52s}) median {med(ts):9.3f} ms   min {s[0]:9.3f}  max {s[-1]:9.3f}   spread {100 * (s[-1] - s[0]) / s[0]:5.2f} %{extra}")
    return med(ts)


def kernels_mode(a, pkg):
    CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
    lib = pkg.get_lib()
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(5)
    rnd = lambda shape: (torch.rand(shape, generator=gen) * 2 - 1).to(DEV)
    for cfg, side in CONFIGS.items():
        n, L, d, h, w = 1, 8, 48, side // 4, side // 4
        z, eps, hist = rnd((n, d, h, w, L)), rnd((n, d, h, w, L)), rnd((n, d, h, w, L))
        g, z0 = rnd((n, L, d, h, w)), torch.empty((n, L, d, h, w), device=DEV)
        zin = torch.zeros((n, d, h, w, 2 * L), dtype=torch.bfloat16, device=DEV)
        sumsq = torch.full((n,), 1e6, dtype=torch.float64, device=DEV)
        x, y = rnd((n, 1, d, side, side)), rnd((n, 1, 8, side, side))
        gx, m = torch.empty_like(x), torch.empty_like(y)
        prof = CS.SliceProfile(8, d)
        W32, _, bw, _ = prof.device_tables(DEV)
        hw = side * side
        partials = torch.empty(lib.depth_project_blocks(n, hw), dtype=torch.float64, device=DEV)
        s2 = torch.empty(n, dtype=torch.float64, device=DEV)
        el, vx = z.numel(), x.numel()

        def replaced():
            lib.depth_measure(p(x), p(W32), p(bw), p(m), n, 8, d, hw, sp)
            torch.sub(y, m, out=m)
            lib.depth_measure_adj(p(m), p(W32), p(bw), p(gx), -1.0, 0, n, 8, d, hw, sp)

        variants = [
            ("ctsi_nan_to_num_f32 on the latent", lambda: lib.nan_to_num_f32(p(z), el, sp), 8 * el),
            ("ctsi_guide_z0", lambda: lib.guide_z0(p(z), p(eps), 0.9, 0.436, 0, 10.0, p(z0), n, L, d, h, w, sp), 12 * el),
            ("ctsi_guide_apply (z, zin)", lambda: lib.guide_apply(p(z), None, p(g), p(sumsq), -1.0, -1.0, 1, p(zin), 2 * L, 0, n, L, d,
                                                                 h, w, sp), 14 * el),
            ("ctsi_guide_apply (z, hist, zin)", lambda: lib.guide_apply(p(z), p(hist), p(g), p(sumsq), -1.0, -1.0, 1, p(zin), 2 * L, 0,
                                                                       n, L, d, h, w, sp), 22 * el),
            ("ctsi_nan_to_num_f32 on the decoded volume", lambda: lib.nan_to_num_f32(p(x), vx, sp), 8 * vx),
            ("ctsi_depth_residual_adj (kernel + finalize)", lambda: lib.depth_residual_adj(
                p(x), p(y), p(W32), p(bw), p(gx), p(partials), p(s2), n, 1, 8, d, hw, sp), 4 * (2 * vx + y.numel())),
            ("depth_measure -> subtract -> depth_measure_adj", replaced, 4 * (2 * vx + 5 * y.numel())),
        ]
        times = alternate([(k, f) for k, f, _ in variants], a.rounds, a.warmup, a.reps)
        print(f"[kernels, {cfg}: latent (1,8,48,{h},{w}) = {el / 1e6:.2f} M elements, volume (1,1,48,{side},{side}) = {vx / 1e6:.1f} M "
              f"voxels, y 8 slices] {a.rounds} alternated rounds after {a.warmup} warm-up; {a.reps} back-to-back calls per timing")
        floor = {}
        for k, _, nbytes in variants:
            ts = times[k]
            per_byte = med(ts) / nbytes
            if k.startswith("ctsi_nan_to_num"):
                floor["now"] = per_byte
            s = sorted(ts)
            print(f"  ({k:48s}) min {1e3 * s[0]:8.1f} us  median {1e3 * med(ts):8.1f} us  max {1e3 * s[-1]:8.1f} us   "
                  f"{nbytes / 1e6:7.1f} MB -> {nbytes / (med(ts) * 1e-3) / 1e12:5.2f} TB/s at the median   "
                  f"{per_byte / floor['now']:5.2f} x the nan_to_num pass per byte")
        r, r2 = times["ctsi_depth_residual_adj (kernel + finalize)"], times["depth_measure -> subtract -> depth_measure_adj"]
        print(f"  the one pass takes {med(r) / med(r2):.2f} x the time of the three passes it replaces")
        del z, eps, hist, g, z0, zin, x, y, gx, m
        torch.cuda.empty_cache()


def _volume(side):
    return formula_input((1, 1, 8, side, side), 18).clamp(-1, 1).to(DEV)


def _model(pkg):
    torch.manual_seed(0)
    return pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)


def _noise_fn():
    gen = torch.Generator(device=DEV).manual_seed(3)
    return lambda i, shape: torch.randn(shape, generator=gen, device=DEV)


def evaluation_mode(a, pkg):
    MG = importlib.import_module("video-to-video-diffusion_amd.measurement_guidance")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    model = _model(pkg)
    ctx = E.Ctx.get(torch.device(DEV))
    for cfg, side in CONFIGS.items():
        v_in = _volume(side)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        try:
            with torch.no_grad():
                v, z_cond = model._encode_conditioning(ctx, v_in, 48)
                shape = tuple(z_cond.shape)
                after_encode = torch.cuda.max_memory_allocated()
                sm = S.DDIMSampler(model.diffusion, model.unet)
                mg = MG.MeasurementGuidance(start=1.0)
                sm.sample(shape, z_cond, 2, DEV, progress=False, noise_fn=_noise_fn(), measurement=mg.bind(v, model.vae))
                torch.cuda.synchronize()
        except torch.cuda.OutOfMemoryError as exc:
            print(f"[one guided evaluation, {cfg}] does not fit: {str(exc).splitlines()[0]}")
            continue
        peak = torch.cuda.max_memory_allocated()
        prog = [p for k, p in model.unet.__dict__["_ctsi_programs"].items() if k[0] == "sampler" and k[3:6] == shape[2:]][-1]
        t_desc = [int(t) for t in sm._get_timesteps(2)]
        plan = S._step_plan(model.diffusion, "ddim", t_desc, 0.0, 2, None)
        e = len(t_desc) - 1
        state = {}
        with torch.no_grad(), ctx.scope():
            run = MG.GuideRun(mg.bind(v, model.vae), model.diffusion, plan, 2, ctx, shape)
            run.save_state(prog)

            def decode():
                with torch.enable_grad():
                    state["x"] = model.vae.decode_with_grad(run.z0)

            def residual():
                state["g_x"] = run.residual(state["x"], e)

            def backward():
                state["g_z"], = torch.autograd.grad(state["x"], run.z0, state["g_x"])

            variants = [("captured step replay (U-Net + update), unguided", prog.launch),
                        ("  save z_t (device copy)", lambda: run.save_state(prog)),
                        ("  ctsi_guide_z0", lambda: run.form_z0(prog, e)),
                        ("  decode forward (decode_with_grad)", decode),
                        ("  ctsi_depth_residual_adj", residual),
                        ("  decode backward (data gradients)", backward),
                        ("  ctsi_guide_apply", lambda: run.apply(prog, e, state["g_z"]))]
            times = alternate(variants, a.rounds, a.warmup, before=lambda name: prog.step_ptr.zero_())
        print(f"[one guided evaluation, {cfg}: (1,1,8,{side},{side}) -> 48 slices, latent {shape}, production model] {a.rounds} "
              f"alternated rounds after {a.warmup} warm-up; the pieces run in order, each between its own event pair")
        step = show(variants[0][0], times[variants[0][0]])
        added = 0.0
        for name, _ in variants[1:]:
            added += show(name, times[name])
        print(f"  a guided evaluation adds {added:.2f} ms to the {step:.2f} ms step: {added / step:.2f} x the step; decode backward / "
              f"forward {med(times[variants[5][0]]) / med(times[variants[3][0]]):.2f}")
        print(f"  device memory: {base / 2**30:.2f} GiB before (the model), peak {after_encode / 2**30:.2f} GiB after encode, peak "
              f"{peak / 2**30:.2f} GiB with the step program and the decoder's gradient program (every decoder activation kept) "
              f"of {torch.cuda.get_device_properties(0).total_memory / 2**30:.0f} GiB")
        model.invalidate_engine_cache()
        del prog, run, state, times, variants
        torch.cuda.empty_cache()


def generate_mode(a, pkg):
    MG = importlib.import_module("video-to-video-diffusion_amd.measurement_guidance")
    CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
    model, v_in = _model(pkg), _volume(192)
    attrs = [("generate(), measurement_guidance = None", None),
             ("generate(), MeasurementGuidance() (26 of 51 evaluations)", MG.MeasurementGuidance()),
             ("generate(), MeasurementGuidance(every=5) (6 of 51)", MG.MeasurementGuidance(every=5))]
    outs = {}

    def run(name, attr):
        def f():
            model.measurement_guidance = attr
            outs[name] = model.generate(v_in, "ddim", num_inference_steps=50, target_depth=48, noise_fn=_noise_fn())
        return f

    times = alternate([(k, run(k, v)) for k, v in attrs], a.rounds, a.warmup)
    model.measurement_guidance = None
    print(f"[generate(), config 1: (1,1,8,192,192) -> 48 slices, DDIM-50 (51 evaluations), production model] {a.rounds} alternated "
          f"rounds after {a.warmup} warm-up")
    prof = CS.SliceProfile(8, 48)
    m0 = None
    for k, attr in attrs:
        r = float((v_in - prof.measure(outs[k])).double().norm())
        extra = f"   ||y - W x|| of the result {r:9.4f}"
        if attr is not None:
            st = attr.last_stats
            extra += f"; ||y - W D(z0)|| at the first / last guided evaluation {float(st[0, 0]):.4f} / {float(st[-1, 0]):.4f}"
        m = show(k, times[k], extra)
        m0 = m if m0 is None else m0
        if attr is not None:
            n_g = len(attr.guided_evaluations(51))
            print(f"      + {m - m0:.2f} ms = {100 * (m - m0) / m0:.1f} % of generate(), {(m - m0) / n_g:.2f} ms per guided evaluation")
    print("  (random weights: the residuals are reported, nothing is said about image quality)")


def default_mode(a, pkg):
    model, v_in = _model(pkg), _volume(512)
    times = alternate([("generate()", lambda: model.generate(v_in, "ddim", num_inference_steps=50, target_depth=48,
                                                             noise_fn=_noise_fn()))], a.rounds, a.warmup)
    print(f"[default path, package from {os.path.relpath(ROOT)}] config-2 generate(), DDIM-50, {a.rounds} rounds after {a.warmup} warm-up")
    show("generate() without the attribute", times["generate()"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "evaluation", "generate", "default"), default="kernels")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="--mode kernels: back-to-back calls per event pair")
    ap.add_argument("--root", default=None, help="import the package from this checkout instead of the tool's own")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_guide_bench.py measures on a ROCm device; none is available")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print(f"device {torch.cuda.get_device_name(0)}; mode {a.mode}; HIP events, host launch included")
    {"kernels": kernels_mode, "evaluation": evaluation_mode, "generate": generate_mode, "default": default_mode}[a.mode](a, pkg)


if __name__ == "__main__":
    main()
