"""What the x0 update form costs per sampler step, measured in ONE process with the two step programs of a
v-prediction model alternated round-robin, at config 2 (latent (1,8,48,128,128)) and config 1 ((1,8,48,48,48)), bf16,
random-init weights (seed 0).  HIP events around captured replays on the engine stream, medians over --replays replays after
warm-up:

  VE  v-prediction DDIM step, eps form: U-Net, ctsi_pred_to_eps (12 B per element), ctsi_ddim_step (14 B per element)
  VX  v-prediction DDIM step, x0 form:  U-Net, ctsi_x0_step (14 B per element): one launch and 12 B per element fewer

then the two update kernels alone on the same buffers (buffer sets rotated past the 256 MiB Infinity Cache): ctsi_ddim_step
and ctsi_x0_step without history or noise, and ctsi_x0_step with both (the DPM-Solver++ / stochastic rows, 26 B per element).
The expectation: VX is not slower than VE beyond the replay-to-replay spread printed beside the medians.

Sample quality under the x0 form or the rescaled schedule is NOT measured: there are no trained weights.

usage: python tools/x0_form_bench.py [--replays 30] [--configs 2,1] [--json out.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PEAK_HBM_GBS = 8000.0
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
LATENTS = {2: (1, 8, 48, 128, 128), 1: (1, 8, 48, 48, 48)}


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


def step_times(pkg, model, shape, replays, warmup):
    """Median captured-replay time (ms) of the two step programs, alternated VE, VX per round."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    unet = model.unet
    n, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    progs = {}
    with ctx.scope():
        for name, form in (("VE", "eps"), ("VX", "x0")):
            g = pkg.GaussianDiffusion(prediction_type="v_prediction")
            g.update_form = form
            t_ddim = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(50)]
            plan = S._step_plan(g, "ddim", t_ddim, 0.0, 2, None)
            prog = E.UNetProgram(ctx, unet, n, d, h, w, (g.timesteps + 1) * n, unet.attention_mode,
                                 prediction="v_prediction")
            prog.add_sampler_step(plan.kind, plan.with_noise, update_form=form)
            gen = torch.Generator().manual_seed(7)
            z = torch.randn((n, L, d, h, w), generator=gen)
            c = torch.randn((n, L, d, h, w), generator=gen)
            prog.load_latents(z.to(DEV), c.to(DEV))
            prog.set_schedule([t for t in plan.t for _ in range(n)], plan.coef.to(DEV), plan.pred)
            prog.capture()
            prog.step_ptr.zero_()
            progs[name] = prog
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for name, prog in progs.items():
                prog.step_ptr.fill_(r % len(t_ddim))            # a valid row of the schedule, the same for both
                ms = ev.time_ms(ctx.sptr, prog.launch)
                if r >= warmup:
                    times[name].append(ms)
        ev.close()
    E.check_device_errors(ctx)
    launches = {k: len(p.ops) - p.unet_op_count for k, p in progs.items()}
    del progs
    torch.cuda.empty_cache()
    return ({k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}, launches)


def launch_times(shape, repeats):
    """ctsi_ddim_step and ctsi_x0_step alone at `shape` on the same buffers (fp32 z / output / history, fp32 NCDHW noise, the
    bf16 [z | cond] input slice), HIP events over launches that rotate through buffer sets larger than the Infinity Cache.
    Bytes per element: 14 (z r/w, output r, bf16 slice w), 26 with history (r/w) and noise (r)."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    n, L, d, h, w = shape
    numel = n * L * d * h * w
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    # finite, contractive rows: the launches are repeated in place on the same z
    ddim = torch.tensor([[0.8, 0.6, 0.5, 0.4, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device=DEV)
    x0 = torch.tensor([[0.6, 0.8, 0.5, 0.3, 0.0, 0.0, 10.0, 0.0], [0.6, 0.8, 0.5, 0.3, -0.1, 0.2, 10.0, 0.0]],
                      dtype=torch.float32, device=DEV)
    steps = [torch.full((1,), k, dtype=torch.int32, device=DEV) for k in (0, 1)]
    nsets = max(8, int(300e6 // (14 * numel)) + 1)
    sets = []
    for k in range(nsets):
        gen = torch.Generator(device=DEV).manual_seed(k)
        f = [torch.randn((numel,), device=DEV, generator=gen) for _ in range(4)]        # z, output, history, noise
        sets.append(f + [torch.zeros((2 * numel,), dtype=torch.bfloat16, device=DEV)])
    nf = torch.zeros((4, 6), dtype=torch.int32, device=DEV)
    nbytes = {"ddim_step": 14 * numel, "x0_step": 14 * numel, "x0_step_hist_noise": 26 * numel}
    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        ev = _Events(lib)
        iters = 10 * nsets

        def launch(kind, s):
            if kind == "ddim_step":
                lib.ddim_step(P(s[0]), P(s[1]), None, P(s[4]), 2 * L, 0, P(ddim), P(steps[0]), n, L, d, h, w, P(nf), sptr)
            elif kind == "x0_step":
                lib.x0_step(P(s[0]), P(s[1]), None, None, P(s[4]), 2 * L, 0, P(x0), P(steps[0]), n, L, d, h, w, P(nf), sptr)
            else:
                lib.x0_step(P(s[0]), P(s[1]), P(s[2]), P(s[3]), P(s[4]), 2 * L, 0, P(x0), P(steps[1]), n, L, d, h, w,
                            P(nf), sptr)

        for kind in list(nbytes) * 2:                           # two alternated passes; the second is reported
            for s in sets:
                launch(kind, s)
            ts = [ev.time_ms(sptr, lambda: [launch(kind, sets[i % nsets]) for i in range(iters)]) / iters
                  for _ in range(repeats)]
            us = statistics.median(ts) * 1e3
            res[kind] = dict(us=us, bytes=nbytes[kind], tb_s=nbytes[kind] / (us * 1e-6) / 1e12,
                             share_of_hbm_peak=nbytes[kind] / (us * 1e-6) / 1e9 / PEAK_HBM_GBS)
        ev.close()
    E.check_device_errors(ctx)
    del sets
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="2,1")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.replays < 20:
        raise SystemExit("--replays must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("x0_form_bench.py measures on a ROCm device; none is visible")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print("NOTE: random-init weights; sample quality under the x0 form / the rescaled schedule is not measured.", flush=True)
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    out = {"weights": "random init, torch.manual_seed(0)", "precision": "bf16", "replays": args.replays, "configs": {}}
    for cfg in [int(c) for c in args.configs.split(",")]:
        shape = LATENTS[cfg]
        med, span, launches = step_times(pkg, model, shape, args.replays, args.warmup)
        alone = launch_times(shape, 5)
        diff = (med["VX"] - med["VE"]) * 1e3
        spread = max(span[k][1] - span[k][0] for k in span) * 1e3
        res = {"latent": shape, "step_ms": med, "step_ms_min_max": span, "launches_after_unet": launches, "alone": alone,
               "VX_minus_VE_us": diff, "replay_spread_us": spread}
        print(f"config {cfg} latent {shape}: captured step, median of {args.replays} replays (ms): "
              + ", ".join(f"{k} {med[k]:.3f} [{span[k][0]:.3f}-{span[k][1]:.3f}]" for k in med), flush=True)
        print(f"config {cfg}: launches behind the U-Net: {launches}", flush=True)
        for k, v in alone.items():
            print(f"config {cfg} {k} alone: {v['us']:.1f} us, {v['bytes'] / 1e6:.2f} MB, {v['tb_s']:.2f} TB/s "
                  f"({100 * v['share_of_hbm_peak']:.0f} % of 8 TB/s)", flush=True)
        print(f"config {cfg}: VX - VE = {diff:+.1f} us; largest min-max spread of the replays {spread:.1f} us: the x0 step is "
              f"{'NOT slower beyond the spread' if diff <= spread else 'SLOWER beyond the spread'}", flush=True)
        model.invalidate_engine_cache()         # the next config builds its own programs
        out["configs"][str(cfg)] = res
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({c: {"step_ms": {k: round(v, 4) for k, v in r["step_ms"].items()},
                          "VX_minus_VE_us": round(r["VX_minus_VE_us"], 1),
                          "alone_us": {k: round(v["us"], 1) for k, v in r["alone"].items()}}
                      for c, r in out["configs"].items()}))


if __name__ == "__main__":
    main()
