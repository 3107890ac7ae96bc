"""What v-prediction costs per sampler step, measured in ONE process with the epsilon and the v step
programs alternated round-robin, at config 2 (latent (1,8,48,128,128)) and config 1 ((1,8,48,48,48)), bf16, random-init
weights (seed 0).  HIP events around captured replays on the engine stream, medians over --replays replays after warm-up:

  E   epsilon DDIM step (the headline step: prediction_type='epsilon' runs no new code)
  V   v-prediction DDIM step (+ one ctsi_pred_to_eps launch, 12 B per element)
  EH  epsilon Heun step on a corrector row
  VH  v-prediction Heun step on a corrector row (+ one ctsi_pred_to_eps launch that also reads D1: 16 B per element)

then ctsi_pred_to_eps on its own (buffer sets rotated past the 256 MiB Infinity Cache), its bytes and achieved TB/s, and the
figure to beat: V - E against "one launch + that traffic at the GroupNorm-apply bandwidth the README quotes (5.7 TB/s)";
twice that estimate is the point past which DESIGN has to say where the rest goes.

Sample quality under v-prediction is NOT measured: there are no trained weights.

usage: python tools/vpred_bench.py [--replays 30] [--configs 2,1] [--json out.json]"""
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
GN_APPLY_TBS = 5.7          # README, "HBM-bound passes"
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
    """Median captured-replay time (ms) of the four step programs, alternated E, V, EH, VH per round."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    unet = model.unet
    n, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    diff = {"epsilon": pkg.GaussianDiffusion(), "v_prediction": pkg.GaussianDiffusion(prediction_type="v_prediction")}
    t_ddim = [int(t) for t in S.DDIMSampler(diff["epsilon"], None)._get_timesteps(50)]
    heun = S.HeunSampler(diff["epsilon"], None, order=2).coef_rows(10)
    corrector = next(e for e in range(1, len(heun.t)) if not heun.closes[e - 1])
    variants = {"E": ("epsilon", "ddim"), "V": ("v_prediction", "ddim"), "EH": ("epsilon", "heun"),
                "VH": ("v_prediction", "heun")}
    progs, row = {}, {}
    with ctx.scope():
        for name, (ptype, kind) in variants.items():
            g = diff[ptype]
            plan = S._step_plan(g, kind, t_ddim if kind == "ddim" else list(heun.t), 0.0, 2, heun if kind == "heun" else None)
            kw = dict(prediction=ptype) if ptype != "epsilon" else {}
            prog = E.UNetProgram(ctx, unet, n, d, h, w, (g.timesteps + 1) * n, unet.attention_mode, **kw)
            prog.add_sampler_step(plan.kind, plan.with_noise)
            gen = torch.Generator().manual_seed(7)
            z = torch.randn((n, L, d, h, w), generator=gen)
            c = torch.randn((n, L, d, h, w), generator=gen)
            prog.load_latents(z.to(DEV), c.to(DEV))
            prog.set_schedule([t for t in plan.t for _ in range(n)], plan.coef.to(DEV), plan.pred)
            prog.capture()
            prog.step_ptr.zero_()
            progs[name], row[name] = prog, (None if kind == "ddim" else corrector)
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for name, prog in progs.items():
                # a valid row of the schedule, the same for both members of a pair (Heun: always a corrector row)
                prog.step_ptr.fill_(r % len(t_ddim) if row[name] is None else row[name])
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
    """ctsi_pred_to_eps alone at `shape` (fp32 buffers of the step program's size), HIP events over launches that rotate
    through buffer sets larger than the Infinity Cache.  Bytes per element: 12 (out r/w, z r), 16 when the row reads hist."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    n, L, d, h, w = shape
    per = L * d * h * w
    numel = n * per
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    rows = torch.tensor([[0.6, 0.8, 0.0, 0.0], [0.6, 0.5, 0.3, 0.0]], dtype=torch.float32, device=DEV)
    steps = [torch.full((1,), k, dtype=torch.int32, device=DEV) for k in (0, 1)]
    nsets = max(8, int(300e6 // (12 * numel)) + 1)
    sets = []
    for k in range(nsets):
        gen = torch.Generator(device=DEV).manual_seed(k)
        sets.append([torch.randn((n, per), device=DEV, generator=gen) for _ in range(3)])
    nbytes = {"vp_row": 12 * numel, "heun_corrector_row": 16 * numel}
    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        ev = _Events(lib)
        iters = 10 * nsets

        def launch(kind, s):
            lib.pred_to_eps(P(s[0]), P(s[1]), P(s[2]), P(rows), P(steps[0 if kind == "vp_row" else 1]), 1, n, n, per, sptr)

        for kind in list(nbytes) * 2:                           # two alternated passes; the second is reported
            for s in sets:
                launch(kind, s)
            ts = [ev.time_ms(sptr, lambda: [launch(kind, sets[i % nsets]) for i in range(iters)]) / iters
                  for _ in range(repeats)]
            us = statistics.median(ts) * 1e3
            res[kind] = dict(us=us, bytes=nbytes[kind], tb_s=nbytes[kind] / (us * 1e-6) / 1e12,
                             share_of_hbm_peak=nbytes[kind] / (us * 1e-6) / 1e9 / PEAK_HBM_GBS)
        ev.close()
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
        raise SystemExit("vpred_bench.py measures on a ROCm device; none is visible")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print("NOTE: random-init weights; sample quality under v-prediction is not measured.", flush=True)
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    out = {"weights": "random init, torch.manual_seed(0)", "precision": "bf16", "replays": args.replays, "configs": {}}
    for cfg in [int(c) for c in args.configs.split(",")]:
        shape = LATENTS[cfg]
        med, span, launches = step_times(pkg, model, shape, args.replays, args.warmup)
        alone = launch_times(shape, 5)
        res = {"latent": shape, "step_ms": med, "step_ms_min_max": span, "launches_after_unet": launches, "alone": alone}
        print(f"config {cfg} latent {shape}: captured step, median of {args.replays} replays (ms): "
              + ", ".join(f"{k} {med[k]:.3f} [{span[k][0]:.3f}-{span[k][1]:.3f}]" for k in med), flush=True)
        print(f"config {cfg}: launches behind the U-Net: {launches}", flush=True)
        for k, v in alone.items():
            print(f"config {cfg} pred_to_eps alone, {k}: {v['us']:.1f} us, {v['bytes'] / 1e6:.2f} MB, {v['tb_s']:.2f} TB/s "
                  f"({100 * v['share_of_hbm_peak']:.0f} % of 8 TB/s)", flush=True)
        for name, base, kind in (("V", "E", "vp_row"), ("VH", "EH", "heun_corrector_row")):
            diff = (med[name] - med[base]) * 1e3
            est = alone[kind]["bytes"] / (GN_APPLY_TBS * 1e12) * 1e6
            res[f"{name}_minus_{base}_us"], res[f"{name}_estimate_us"] = diff, est
            print(f"config {cfg}: {name} - {base} = {diff:+.1f} us; estimate (its traffic at {GN_APPLY_TBS} TB/s, launch "
                  f"excluded) {est:.1f} us, measured alone {alone[kind]['us']:.1f} us; "
                  f"{'within' if diff <= 2 * max(est, alone[kind]['us']) else 'MORE than'} twice the estimate", flush=True)
        model.invalidate_engine_cache()         # the next config builds its own programs
        out["configs"][str(cfg)] = res
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({c: {"step_ms": {k: round(v, 4) for k, v in r["step_ms"].items()},
                          "V_minus_E_us": round(r["V_minus_E_us"], 1), "VH_minus_EH_us": round(r["VH_minus_EH_us"], 1)}
                      for c, r in out["configs"].items()}))


if __name__ == "__main__":
    main()
