"""What the learned reverse variance and the strided ancestral sampler cost, measured on a ROCm device with
random-init weights (seed 0), bf16.  HIP events around captured replays / launches on the engine stream, medians after warm-up,
the variants of a comparison alternated round-robin in ONE process:

  step     config 2 (latent (1, 8, 48, 128, 128)) and config 1 ((1, 8, 48, 48, 48)): one captured ancestral step of a default
           model ('ddpm': ctsi_ddpm_step) against a learn_sigma model ('ddpm_lv' with the learned variance: the 2L-channel head,
           ctsi_sigma_split, ctsi_ddpm_lv_step), plus the default model's DDIM step (the headline step).
  kernels  ctsi_sigma_split and ctsi_ddpm_lv_step (with and without the variance channels) alone, bytes / s, beside ctsi_ddpm_step
           on the same buffers (buffer sets rotated past the 256 MiB Infinity Cache); the ratio to the sibling per byte moved.
  sample   one 192 x 192 patch (latent (1, 8, 48, 48, 48)): 'ddpm_spaced' at N = 50 / 100 / 250 beside 'ddpm' at full length and
           DDIM-50, wall clock of sample() ending in a device synchronise.
  train    config-3 micro-step (latents (4, 8, 48, 24, 24), training_loss + backward): default model / MSE against a learn_sigma
           model / hybrid loss.

    python tools/learned_sigma_bench.py [--log profiles/learned_sigma_bench.log]
    python tools/learned_sigma_bench.py --default-only --tree <checkout> --label parent --json out.json
        the default model's figures alone (DDIM step, 'ddpm' step, micro-step), with the package imported from another checkout:
        run on the parent commit and on this one in the same session; --compare a.json b.json ... prints them side by side.

Sample quality is NOT measured: there are no trained weights."""
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
LATENTS = {2: (1, 8, 48, 128, 128), 1: (1, 8, 48, 48, 48)}
TRAIN_LATENT = (4, 8, 48, 24, 24)
_LOG = None


def say(msg=""):
    print(msg, flush=True)
    if _LOG is not None:
        _LOG.write(msg + "\n")
        _LOG.flush()


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


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

    def close(self):
        for e in self.ev:
            self.lib.event_destroy(e)


def _models(pkg, default_only):
    torch.manual_seed(0)
    out = {"default": (pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV), "fixed_small")}
    if not default_only:
        torch.manual_seed(0)
        cfg = {**FULL_CFG, "unet_learn_sigma": True, "var_type": "learned_range"}
        out["learn_sigma"] = (pkg.VideoToVideoDiffusion(cfg).eval().to(DEV), "learned_range")
    return out


def step_times(pkg, models, shape, replays, warmup):
    """Median captured-replay time (ms) of the step programs, alternated per round."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    n, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    progs, nrows = {}, {}
    with ctx.scope():
        for mname, (model, var_type) in models.items():
            g = model.diffusion
            t50 = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(50)]
            variants = [("ddim", "ddim", None)] if mname == "default" else []
            if var_type == "learned_range":
                variants.append(("ddpm_lv", "ddpm_lv", S.lv_rows(g, t50)))
            else:
                variants.append(("ddpm", "ddpm", None))
            for tag, kind, rows in variants:
                plan = S._step_plan(g, kind, t50, 0.0, 2, rows)
                prog = E.UNetProgram(ctx, model.unet, n, d, h, w, (g.timesteps + 1) * n, model.unet.attention_mode)
                prog.add_sampler_step(plan.kind, plan.with_noise, **(dict(learned_variance=True) if getattr(plan, "learned", False)
                                                                     else {}))
                gen = torch.Generator().manual_seed(7)
                z, c = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
                prog.load_latents(z.to(DEV), c.to(DEV))
                prog.set_schedule([t for t in plan.t for _ in range(n)], plan.coef.to(DEV), plan.pred)
                if prog.noise is not None:
                    prog.noise.normal_()
                prog.capture()
                prog.step_ptr.zero_()
                progs[f"{mname}:{tag}"], nrows[f"{mname}:{tag}"] = prog, len(t50)
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for name, prog in progs.items():
                prog.step_ptr.fill_(r % (nrows[name] - 1))          # a valid row with noise, the same for every variant
                ms = ev.time_ms(ctx.sptr, prog.launch)
                if r >= warmup:
                    times[name].append(ms)
        ev.close()
    E.check_device_errors(ctx)
    launches = {k: len(p.ops) - p.unet_op_count for k, p in progs.items()}
    ops = {k: len(p.ops) for k, p in progs.items()}
    del progs
    torch.cuda.empty_cache()
    return {k: _stat(v) for k, v in times.items()}, launches, ops


def kernel_times(shape, repeats):
    """The new streaming kernels alone beside ctsi_ddpm_step on the same fp32 buffers.  Bytes per element of the latent:
    ddpm_step 4 (z r) + 4 (eps) + 4 (noise) + 4 (z w) + 2 (bf16 zin) = 18; ddpm_lv_step the same, + 4 with the variance channels;
    sigma_split 8 (out2 r) + 4 (eps w) + 4 (vraw w) = 16."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    n, L, d, h, w = shape
    numel = n * L * d * h * w
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    coef = torch.tensor([[0.6, 0.8, 0.3, 0.7, -3.0, -3.5, 1.0, 1.0]], dtype=torch.float32, device=DEV)
    coef_ddpm = torch.tensor([[0.6, 0.8, 0.3, 0.7, 0.17, 0.0, 0.0, 0.0]], dtype=torch.float32, device=DEV)
    nsets = max(8, int(300e6 // (18 * numel)) + 1)
    sets = []
    for k in range(nsets):
        gen = torch.Generator(device=DEV).manual_seed(k)
        s = dict(z=torch.randn((n, d, h, w, L), device=DEV, generator=gen), eps=torch.randn((n, d, h, w, L), device=DEV, generator=gen),
                 v=torch.rand((n, d, h, w, L), device=DEV, generator=gen) * 2 - 1,
                 noise=torch.randn((n, L, d, h, w), device=DEV, generator=gen),
                 out2=torch.randn((n, d, h, w, 2 * L), device=DEV, generator=gen),
                 zin=torch.zeros((n, d, h, w, 2 * L), dtype=torch.bfloat16, device=DEV))
        sets.append(s)
    calls = {
        "ddpm_step": (18, lambda s: lib.ddpm_step(P(s["z"]), P(s["eps"]), P(s["noise"]), P(s["zin"]), 2 * L, 0, P(coef_ddpm), None,
                                                   n, L, d, h, w, sptr)),
        "ddpm_lv_step (fixed-small)": (18, lambda s: lib.ddpm_lv_step(P(s["z"]), P(s["eps"]), None, P(s["noise"]), P(s["zin"]), 2 * L,
                                                                       0, P(coef), None, n, L, d, h, w, sptr)),
        "ddpm_lv_step (learned)": (22, lambda s: lib.ddpm_lv_step(P(s["z"]), P(s["eps"]), P(s["v"]), P(s["noise"]), P(s["zin"]), 2 * L,
                                                                   0, P(coef), None, n, L, d, h, w, sptr)),
        "sigma_split": (16, lambda s: lib.sigma_split(P(s["out2"]), P(s["eps"]), P(s["v"]), n, n, L, d, h, w, sptr)),
    }
    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        ev = _Events(lib)
        iters = 10 * nsets
        for name in list(calls) * 2:                           # two alternated passes; the second is reported
            bpe, fn = calls[name]
            for s in sets:
                fn(s)
            ts = [ev.time_ms(sptr, lambda: [fn(sets[i % nsets]) for i in range(iters)]) / iters for _ in range(repeats)]
            us = statistics.median(ts) * 1e3
            res[name] = dict(us=us, bytes=bpe * numel, tb_s=bpe * numel / (us * 1e-6) / 1e12)
        ev.close()
    for name, r in res.items():
        r["ratio_to_ddpm_step_per_byte"] = r["tb_s"] / res["ddpm_step"]["tb_s"]
    del sets
    torch.cuda.empty_cache()
    return res


def sample_times(pkg, models, shape, repeats):
    """Wall clock (s) of whole sampling runs on one patch, each ending in a synchronise; the first run of each (program build,
    capture) is not timed."""
    runs = []
    dm, _ = models["default"]
    cond = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    runs.append(("ddim-50 (default model)", lambda: pkg.DDIMSampler(dm.diffusion, dm.unet).sample(shape, cond, 50, DEV, progress=False)))
    for mname, (model, var_type) in models.items():
        sp = pkg.DDPMSampler(model.diffusion, model.unet)
        for n_steps in (50, 100, 250):
            runs.append((f"ddpm_spaced-{n_steps} ({mname} model, {var_type})",
                         lambda sp=sp, n_steps=n_steps: sp.sample(shape, cond, DEV, progress=False, num_inference_steps=n_steps)))
        runs.append((f"ddpm, all 1000 steps ({mname} model, {var_type})", lambda sp=sp: sp.sample(shape, cond, DEV, progress=False)))
    res = {}
    for name, fn in runs:
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[name] = _stat(ts)
        say(f"  {name:52s} {res[name]['median']:7.3f} s [{res[name]['min']:.3f}-{res[name]['max']:.3f}]")
    return res


def train_times(models, steps, warmup):
    gen = torch.Generator().manual_seed(11)
    z0, cond, noise = (torch.randn(TRAIN_LATENT, generator=gen).to(DEV) for _ in range(3))
    t = torch.randint(0, 1000, (TRAIN_LATENT[0],), generator=gen).to(DEV)
    times = {k: [] for k in models}
    for model, _ in models.values():
        model.unet.train()
    for r in range(warmup + steps):
        for name, (model, _) in models.items():
            un = model.unet
            for p in un.parameters():
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = model.diffusion.training_loss(un, z0, cond, t=t, noise=noise)
            loss.backward()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    for model, _ in models.values():
        model.unet.eval()
        for p in model.unet.parameters():
            p.grad = None
    res = {k: _stat(v) for k, v in times.items()}
    for k, st in res.items():
        say(f"  config-3 micro-step, {k:12s} {st['median']:8.2f} ms [{st['min']:.2f}-{st['max']:.2f}]")
    return res


def compare(paths):
    for p in paths:
        with open(p) as f:
            r = json.load(f)
        say(f"{os.path.basename(p)}: {r.get('tree')}")
        for cfg, v in r.get("step", {}).items():
            for name, st in v["ms"].items():
                say(f"  config {cfg} {name:22s} {st['median']:.3f} ms [{st['min']:.3f}-{st['max']:.3f}], {v['ops'][name]} launches")
        for name, st in r.get("train", {}).items():
            say(f"  config-3 micro-step {name:12s} {st['median']:.2f} ms [{st['min']:.2f}-{st['max']:.2f}]")


def main():
    global _LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="2,1")
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--skip-sample", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--json", default="")
    ap.add_argument("--log", default="")
    ap.add_argument("--compare", nargs="+", default=None)
    args = ap.parse_args()
    if args.log:
        _LOG = open(args.log, "a")
    if args.compare:
        return compare(args.compare)
    if not torch.cuda.is_available():
        raise SystemExit("learned_sigma_bench.py measures on a ROCm device; none is visible")
    sys.path.insert(0, os.path.abspath(args.tree))
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    say(f"learned_sigma_bench: {args.label}; random-init weights (seed 0), bf16; sample quality is not measured")
    models = _models(pkg, args.default_only)
    out = {"tree": args.label, "replays": args.replays, "step": {}, "kernels": {}}
    for cfg in [int(c) for c in args.configs.split(",")]:
        shape = LATENTS[cfg]
        ms, launches, ops = step_times(pkg, models, shape, args.replays, args.warmup)
        out["step"][str(cfg)] = dict(latent=shape, ms=ms, launches_after_unet=launches, ops=ops)
        say(f"config {cfg} latent {shape}: captured step, median of {args.replays} alternated replays")
        for k, st in ms.items():
            say(f"  {k:24s} {st['median']:8.3f} ms [{st['min']:.3f}-{st['max']:.3f}]  ({ops[k]} launches, {launches[k]} behind the U-Net)")
        if not args.default_only:
            d = ms["learn_sigma:ddpm_lv"]["median"] - ms["default:ddpm"]["median"]
            spread = max(st["max"] - st["min"] for st in ms.values())
            say(f"  learn_sigma step - default 'ddpm' step = {d * 1e3:+.1f} us (the wider head + the split launch + 4 B per element in "
                f"the update); replay-to-replay spread {spread * 1e3:.0f} us")
            kr = kernel_times(shape, 5)
            out["kernels"][str(cfg)] = kr
            for name, r in kr.items():
                say(f"  alone: {name:28s} {r['us']:7.1f} us, {r['bytes'] / 1e6:7.2f} MB, {r['tb_s']:.2f} TB/s, "
                    f"{r['ratio_to_ddpm_step_per_byte']:.2f} x ctsi_ddpm_step per byte")
        for model, _ in models.values():
            model.invalidate_engine_cache()
    if not args.default_only and not args.skip_sample:
        say(f"one 192 x 192 patch, latent {LATENTS[1]}: whole sampling runs")
        out["sample"] = sample_times(pkg, models, LATENTS[1], 2)
        for model, _ in models.values():
            model.invalidate_engine_cache()
    say(f"config-3 micro-step, latents {TRAIN_LATENT}: training_loss + backward, median of {args.train_steps}")
    out["train"] = train_times(models, args.train_steps, 2)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    say(json.dumps({"step_ms": {c: {k: round(v["median"], 4) for k, v in r["ms"].items()} for c, r in out["step"].items()},
                    "train_ms": {k: round(v["median"], 2) for k, v in out["train"].items()}}))


if __name__ == "__main__":
    main()
