"""What the ResBlock options cost, measured in ONE process with everything alternated round-robin, bf16,
random-init weights (seed 0).  HIP events on the engine stream, medians after warm-up, min-max spread beside them.

  kernels   ctsi_gn_apply (SiLU + time bias: the default middle pass) against ctsi_gn_apply_mod (scale-shift; scale-shift +
            dropout 0.1; additive + dropout 0.1) on the same tensors, out of place, buffer sets rotated past the 256 MiB Infinity
            Cache -- at the U-Net's largest ResBlock tensor (1, 128, 48, 128, 128) and a mid-level one (1, 256, 48, 64, 64);
            bandwidth = 2 tensor sizes / time.  The backward pair ctsi_gn_bwd / ctsi_gn_bwd_mod likewise (5 tensor sizes: x and
            dy read by pass 1 and again by pass 3, dx written).
  step      config 2 (latent (1, 8, 48, 128, 128)): one captured DDIM step, default model vs use_scale_shift_norm=True.
  train     config 3 micro-step (latents (4, 8, 48, 24, 24), training_loss + backward): default vs scale-shift vs scale-shift +
            dropout 0.1.

    python tools/resblock_options_bench.py [--log profiles/resblock_options_bench.log]
    python tools/resblock_options_bench.py --default-only --tree <checkout> --json out.json
        the default-mode figures alone (default kernels, default step, default micro-step), with the package imported from
        another checkout: run twice on the parent commit and once on this one, then
    python tools/resblock_options_bench.py --compare parent1.json parent2.json new.json
        (the two-runs-of-the-parent method of tools/program_fingerprint.py): the new figures must sit inside the parent's own
        run-to-run spread widened by the replay spread.

Sample quality under either option is NOT measured: there are no trained weights."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import torch

DEV = "cuda:0"
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
TENSORS = {"largest": (1, 128, 48, 128, 128), "mid": (1, 256, 48, 64, 64)}
STEP_LATENT = (1, 8, 48, 128, 128)
TRAIN_LATENT = (4, 8, 48, 24, 24)
GROUPS, EPS, P_DROP = 8, 1e-5, 0.1
_LOG = None


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if _LOG is not None:
        _LOG.write(line + "\n")
        _LOG.flush()


class _Events:
    def __init__(self, lib):
        self.lib, self.ev = lib, []
        for _ in range(2):
            e = C.c_void_p()
            lib.event_create(C.byref(e))
            self.ev.append(e)

    def time_ms(self, sptr, fn):
        self.lib.event_record(self.ev[0], sptr)
        fn()
        self.lib.event_record(self.ev[1], sptr)
        torch.cuda.synchronize()
        ms = C.c_float()
        self.lib.event_elapsed_ms(self.ev[0], self.ev[1], C.byref(ms))
        return ms.value


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def kernel_times(E, shape, rounds, default_only):
    n, c, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    numel = n * c * d * h * w
    nsets = max(2, int(600e6 // (4 * numel)) + 1)
    gen = torch.Generator(device=DEV).manual_seed(1)
    sets = [dict(x=torch.randn((numel,), device=DEV, generator=gen).to(torch.bfloat16),
                 dy=torch.randn((numel,), device=DEV, generator=gen).to(torch.bfloat16),
                 y=torch.empty((numel,), dtype=torch.bfloat16, device=DEV)) for _ in range(nsets)]
    x5 = sets[0]["x"].view(n, d * h * w, GROUPS, c // GROUPS).double()
    sums = torch.stack([x5.sum((1, 3)), (x5 * x5).sum((1, 3))], dim=-1).contiguous()      # every set ~ N(0, 1): one slot serves
    del x5
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    rows = 0.5 * torch.randn((n, 2 * c), device=DEV, generator=gen)
    dtb = torch.zeros((n, 2 * c), device=DEV)
    dg, db, dxs = (torch.zeros(c, device=DEV) for _ in range(3))
    mod = hasattr(lib, "gn_apply_mod") and not default_only
    ws_floats = lib.gn_bwd_workspace_floats(n, c, d, h, w, GROUPS)
    if mod:
        ws_floats = max(ws_floats, lib.gn_bwd_mod_workspace_floats(n, c, d, h, w, GROUPS))
    ws = torch.empty((ws_floats,), device=DEV)
    seed = torch.tensor([20240607], dtype=torch.int64, device=DEV)
    thr = int(P_DROP * 65536)
    inv = 65536.0 / (65536.0 - thr)

    def fwd(s):
        lib.gn_apply(P(s["x"]), P(s["y"]), P(sums), P(gamma), P(beta), n, c, d, h, w, d, GROUPS, EPS, 1, P(rows), 2 * c, None,
                     None, 0, sptr)

    def bwd(s):
        lib.gn_bwd(P(s["x"]), P(s["dy"]), 0, P(sums), P(gamma), P(beta), n, c, d, h, w, GROUPS, EPS, 1, None, 0, None, None,
                   P(s["y"]), P(ws), P(dg), P(db), P(dtb), 2 * c, P(dxs), sptr)

    def fwd_mod(film, t):
        return lambda s: lib.gn_apply_mod(P(s["x"]), P(s["y"]), P(sums), P(gamma), P(beta), n, c, d, h, w, d, GROUPS, EPS, 1,
                                          P(rows), 2 * c, None, None, 0, film, t, inv if t else 1.0, P(seed), 3, sptr)

    def bwd_mod(film, t):
        return lambda s: lib.gn_bwd_mod(P(s["x"]), P(s["dy"]), P(sums), P(gamma), P(beta), n, c, d, h, w, GROUPS, EPS, P(rows),
                                        2 * c, film, t, inv if t else 1.0, P(seed), 3, P(s["y"]), P(ws), P(dg), P(db), P(dtb),
                                        2 * c, P(dxs), sptr)

    kinds = {"fwd default": (fwd, 2), "bwd default": (bwd, 5)}
    if mod:
        kinds.update({"fwd scale-shift": (fwd_mod(1, 0), 2), "fwd scale-shift+dropout": (fwd_mod(1, thr), 2),
                      "fwd additive+dropout": (fwd_mod(0, thr), 2), "bwd scale-shift": (bwd_mod(1, 0), 5),
                      "bwd scale-shift+dropout": (bwd_mod(1, thr), 5), "bwd additive+dropout": (bwd_mod(0, thr), 5)})
    times = {k: [] for k in kinds}
    with ctx.scope():
        ev = _Events(lib)
        for r in range(rounds + 2):
            for k, (fn, _) in kinds.items():
                ms = ev.time_ms(sptr, lambda: [fn(s) for s in sets]) / nsets
                if r >= 2:
                    times[k].append(ms)
    E.check_device_errors(ctx)
    res = {}
    for k, (_, tensors) in kinds.items():
        st = _stat(times[k])
        st["tb_s"] = tensors * 2.0 * numel / (st["median"] * 1e-3) / 1e12
        res[k] = st
        say(f"  {k:26s} {st['median'] * 1e3:8.1f} us [{st['min'] * 1e3:.1f}-{st['max'] * 1e3:.1f}]  {st['tb_s']:.2f} TB/s "
            f"({tensors} tensor sizes)")
    del sets
    torch.cuda.empty_cache()
    return res


def step_times(pkg, E, S, models, replays, warmup):
    n, L, d, h, w = STEP_LATENT
    ctx = E.Ctx.get(torch.device(DEV))
    progs = {}
    with ctx.scope():
        for name, model in models.items():
            g = pkg.GaussianDiffusion()
            t_ddim = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(50)]
            prog = E.UNetProgram(ctx, model.unet, n, d, h, w, g.timesteps + 1, "fast")
            prog.add_sampler_step("ddim", False)
            gen = torch.Generator().manual_seed(7)
            prog.load_latents(torch.randn(STEP_LATENT, generator=gen).to(DEV), torch.randn(STEP_LATENT, generator=gen).to(DEV))
            prog.set_schedule(t_ddim, S.ddim_coef_rows(g.alphas_cumprod, t_ddim, 0.0).to(DEV))
            prog.capture()
            progs[name] = prog
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for name, prog in progs.items():
                prog.step_ptr.fill_(r % 50)
                ms = ev.time_ms(ctx.sptr, prog.launch)
                if r >= warmup:
                    times[name].append(ms)
    E.check_device_errors(ctx)
    res = {k: _stat(v) for k, v in times.items()}
    for k, st in res.items():
        say(f"  config-2 step, {k:24s} {st['median']:8.3f} ms [{st['min']:.3f}-{st['max']:.3f}]  ({len(progs[k].ops)} launches)")
    del progs
    torch.cuda.empty_cache()
    return res


def train_times(pkg, runs, steps, warmup):
    """runs: name -> (model, dropout probability)."""
    gen = torch.Generator().manual_seed(11)
    z0, cond, noise = (torch.randn(TRAIN_LATENT, generator=gen).to(DEV) for _ in range(3))
    t = torch.randint(0, 1000, (TRAIN_LATENT[0],), generator=gen).to(DEV)
    times = {k: [] for k in runs}
    for r in range(warmup + steps):
        for name, (model, p) in runs.items():
            un = model.unet
            un.train()
            if hasattr(un, "dropout"):
                un.dropout = p
            for q in un.parameters():
                q.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = model.diffusion.training_loss(un, z0, cond, t=t, noise=noise)
            loss.backward()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
            un.eval()
    res = {k: _stat(v) for k, v in times.items()}
    for k, st in res.items():
        say(f"  config-3 micro-step, {k:24s} {st['median']:8.2f} ms [{st['min']:.2f}-{st['max']:.2f}]")
    return res


def compare(paths):
    a1, a2, b = (json.load(open(p)) for p in paths)
    say(f"default mode against the parent commit: {paths[0]}, {paths[1]} (two runs of the parent), {paths[2]} (this commit)")
    bad = 0

    def walk(x1, x2, y, path):
        nonlocal bad
        if isinstance(y, dict) and "median" in y:
            lo = min(x1["min"], x2["min"])
            hi = max(x1["max"], x2["max"])
            inside = lo <= y["median"] <= hi
            bad += 0 if inside else 1
            say(f"  {path:42s} parent {x1['median']:.4f} / {x2['median']:.4f} ms (replays {lo:.4f}-{hi:.4f}), this commit "
                f"{y['median']:.4f} ms: {'inside' if inside else 'OUTSIDE'} the parent's spread")
        elif isinstance(y, dict):
            for k in y:
                if k in x1 and k in x2:
                    walk(x1[k], x2[k], y[k], (path + " / " + k) if path else k)

    walk(a1, a2, b, "")
    say(f"{bad} default-mode figure(s) outside the spread of the parent's own two runs")
    return bad


def main():
    global _LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=6)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default="")
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "resblock_options_bench.log"), help="append every printed line here")
    ap.add_argument("--compare", nargs=3, default=None)
    args = ap.parse_args()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        _LOG = open(args.log, "a")
    if args.compare:
        raise SystemExit(1 if compare(args.compare) else 0)
    if not torch.cuda.is_available():
        raise SystemExit("resblock_options_bench.py measures on a ROCm device; none is visible")
    sys.path.insert(0, os.path.abspath(args.tree))
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    say(f"resblock_options_bench: package from {os.path.relpath(os.path.dirname(os.path.abspath(pkg.__file__)), here)}, "
        f"default_only={args.default_only}")
    say("NOTE: random-init weights; sample quality under either option is not measured.")
    out = {"kernels": {}}
    for name, shape in TENSORS.items():
        say(f"{name} tensor {shape}, bf16 NDHWC, {2 * torch.Size(shape).numel() / 1e6:.0f} MB:")
        out["kernels"][name] = kernel_times(E, shape, args.rounds, args.default_only)
    torch.manual_seed(0)
    models = {"default": pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)}
    if not args.default_only:
        torch.manual_seed(0)
        models["scale-shift"] = pkg.VideoToVideoDiffusion(dict(FULL_CFG, unet_use_scale_shift_norm=True)).eval().to(DEV)
    out["step"] = step_times(pkg, E, S, models, args.replays, 3)
    for m in models.values():
        m.invalidate_engine_cache()
    torch.cuda.empty_cache()
    runs = {"default": (models["default"], 0.0)}
    if not args.default_only:
        runs["scale-shift"] = (models["scale-shift"], 0.0)
        runs["scale-shift+dropout"] = (models["scale-shift"], P_DROP)
    out["train"] = train_times(pkg, runs, args.train_steps, 2)
    if not args.default_only:
        d, f = out["step"]["default"], out["step"]["scale-shift"]
        spread = max(d["max"] - d["min"], f["max"] - f["min"])
        say(f"config-2 step: scale-shift - default = {(f['median'] - d['median']) * 1e3:+.0f} us; largest replay spread "
            f"{spread * 1e3:.0f} us")
    if args.json:
        with open(args.json, "w") as fjs:
            json.dump(out, fjs, indent=1)


if __name__ == "__main__":
    main()
