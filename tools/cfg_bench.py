"""What classifier-free guidance costs per sampler step, measured in ONE process with the variants
alternated round-robin, at config 2 (latent (1,8,48,128,128)) and config 1 ((1,8,48,48,48)), bf16, DDIM, random-init
weights (seed 0).  HIP events around captured replays on the engine stream, medians over --replays replays after warm-up:

  A  unguided step, batch 1 (the headline step; for reference only: guidance_scale = 1.0 runs no new code)
  B  unguided step, batch 2 (existing code: the yardstick -- a guided step IS a batch-2 evaluation plus the launches below)
  C  guided step, n = 1, phi = 0        (+ ctsi_cfg_combine, ctsi_cfg_mirror)
  D  guided step, n = 1, phi = 0.7      (+ ctsi_cfg_stats, ctsi_cfg_stats_finalize as well)

then the added launches on their own (buffer sets rotated past the 256 MiB Infinity Cache), their bytes and achieved
TB/s, and the acceptance figure: C - B and D - B against twice the summed stand-alone time of the launches each adds.
Last, the warm whole-volume wall time of generate(v_in, 'ddim', 50, target_depth=48) unguided and at guidance_scale = 3.

Sample quality under guidance is NOT measured: there are no trained weights, and a random U-Net has never seen the null
conditioning.

usage: python tools/cfg_bench.py [--replays 30] [--configs 2,1] [--no-volume] [--json out.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PEAK_HBM_GBS = 8000.0
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
LATENTS = {2: (1, 8, 48, 128, 128), 1: (1, 8, 48, 48, 48)}
VOLUMES = {2: (1, 1, 8, 512, 512), 1: (1, 1, 8, 192, 192)}


def _noise_fn(i, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i), dtype=torch.float32).to(DEV)


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


def step_times(model, shape, replays, warmup):
    """Median captured-replay time (ms) of the four step programs, alternated A, B, C, D per round."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    g, unet = model.diffusion, model.unet
    n, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    t_desc = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(50)]
    coef = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).to(DEV)
    variants = {"A": dict(n=n), "B": dict(n=2 * n), "C": dict(n=n, guided=True), "D": dict(n=n, guided=True, rescale=True)}
    progs = {}
    with ctx.scope():
        for name, kw in variants.items():
            nn_ = kw["n"]
            rows = nn_ * (2 if kw.get("guided") else 1)
            prog = E.UNetProgram(ctx, unet, nn_, d, h, w, (g.timesteps + 1) * rows, unet.attention_mode,
                                 guided=kw.get("guided", False), rescale=kw.get("rescale", False))
            prog.add_sampler_step("ddim", False)
            gen = torch.Generator().manual_seed(7)
            z = torch.randn((nn_, L, d, h, w), generator=gen)
            c = torch.randn((nn_, L, d, h, w), generator=gen)
            prog.load_latents(z.to(DEV), c.to(DEV))
            prog.set_schedule([t for t in t_desc for _ in range(rows)], coef)
            if kw.get("guided"):
                prog.set_guidance(3.0, 0.7 if kw.get("rescale") else 0.0)
            prog.capture()
            prog.step_ptr.zero_()
            progs[name] = prog
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for name, prog in progs.items():
                prog.step_ptr.fill_(r % len(t_desc))          # a valid row of the schedule, the same for every variant
                ms = ev.time_ms(ctx.sptr, prog.launch)
                if r >= warmup:
                    times[name].append(ms)
        ev.close()
    E.check_device_errors(ctx)
    launches = {k: len(p.ops) - p.unet_op_count for k, p in progs.items()}
    del progs
    torch.cuda.empty_cache()
    return ({k: statistics.median(v) for k, v in times.items()},
            {k: (min(v), max(v)) for k, v in times.items()}, launches)


def launch_times(shape, repeats):
    """The added launches alone at `shape` (the engine's layout: fp32 NDHWC eps of batch 2n, bf16 [z | cond] input of
    batch 2n), HIP events over launches that rotate through buffer sets larger than the Infinity Cache.  Bytes per
    element of one sample's latent: combine 12 (eps_c r/w, eps_u r), stats 8 (both read), mirror 4 (bf16 r + w)."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    n, L, d, h, w = shape
    numel, vox = n * L * d * h * w, n * d * h * w
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    scale = torch.tensor([[0.5, 0.7]], dtype=torch.float32, device=DEV)    # s < 1: repeated in-place passes stay finite
    bps = lib.cfg_stats_blocks(L * d * h * w)
    nsets = max(8, int(300e6 // (8 * numel)) + 1)                  # eps alone (8 bytes per element) past 256 MiB
    sets = []
    for k in range(nsets):
        gen = torch.Generator(device=DEV).manual_seed(k)
        sets.append(dict(eps=torch.randn((2 * n, d, h, w, L), device=DEV, generator=gen),
                         xin=torch.randn((2 * n, d, h, w, 2 * L), device=DEV, generator=gen).to(torch.bfloat16),
                         part=torch.zeros(n * bps * 4, dtype=torch.float64, device=DEV),
                         stats=torch.ones((n, 4), dtype=torch.float64, device=DEV)))

    def launch(kind, s):
        if kind == "combine":
            lib.cfg_combine(P(s["eps"]), P(scale), None, None, n, L, d, h, w, sptr)
        elif kind == "combine_rescaled":
            lib.cfg_combine(P(s["eps"]), P(scale), None, P(s["stats"]), n, L, d, h, w, sptr)
        elif kind == "stats":
            lib.cfg_stats(P(s["eps"]), P(scale), None, P(s["part"]), n, L, d, h, w, sptr)
        elif kind == "stats_finalize":
            lib.cfg_stats_finalize(P(s["part"]), P(s["stats"]), n, L, d, h, w, sptr)
        else:
            x = s["xin"]
            lib.cfg_mirror(P(x), C.c_void_p(x.data_ptr() + vox * 2 * L * 2), vox, L * 2, 2 * L * 2, sptr)

    nbytes = {"combine": 12 * numel, "combine_rescaled": 12 * numel, "stats": 8 * numel,
              "stats_finalize": n * bps * 32, "mirror": 4 * numel}
    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        ev = _Events(lib)
        iters = 10 * nsets
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


def volume_walls(model, v_in, repeats):
    """Warm wall time of the whole volume, unguided and guided alternated."""
    calls = {"unguided": {}, "guided_s3": dict(guidance_scale=3.0), "guided_s3_phi0.7": dict(guidance_scale=3.0,
                                                                                            guidance_rescale=0.7)}
    for kw in calls.values():
        model.generate(v_in, "ddim", 50, target_depth=48, noise_fn=_noise_fn, **kw)     # plans, weight pack, capture
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(repeats):
        for k, kw in calls.items():
            t0 = time.perf_counter()
            model.generate(v_in, "ddim", 50, target_depth=48, noise_fn=_noise_fn, **kw)
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return {k: dict(median_s=statistics.median(v), all_s=v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="2,1")
    ap.add_argument("--no-volume", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.replays < 20:
        raise SystemExit("--replays must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("cfg_bench.py measures on a ROCm device; none is visible")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print("NOTE: random-init weights; sample quality under guidance is not measured.", flush=True)
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    out = {"weights": "random init, torch.manual_seed(0)", "precision": "bf16", "sampler": "ddim",
           "replays": args.replays, "configs": {}}
    for cfg in [int(c) for c in args.configs.split(",")]:
        shape = LATENTS[cfg]
        med, span, launches = step_times(model, shape, args.replays, args.warmup)
        alone = launch_times(shape, 5)
        res = {"latent": shape, "step_ms": med, "step_ms_min_max": span, "launches_after_unet": launches, "alone": alone}
        print(f"config {cfg} latent {shape}: captured DDIM step, median of {args.replays} replays (ms): "
              + ", ".join(f"{k} {med[k]:.3f} [{span[k][0]:.3f}-{span[k][1]:.3f}]" for k in med), flush=True)
        print(f"config {cfg}: C / A = {med['C'] / med['A']:.3f}, C / B = {med['C'] / med['B']:.4f}, "
              f"D / B = {med['D'] / med['B']:.4f}, B / A = {med['B'] / med['A']:.3f}", flush=True)
        for k, v in alone.items():
            print(f"config {cfg} alone {k}: {v['us']:.1f} us, {v['bytes'] / 1e6:.2f} MB, {v['tb_s']:.2f} TB/s "
                  f"({100 * v['share_of_hbm_peak']:.0f} % of 8 TB/s)", flush=True)
        add_c = alone["combine"]["us"] + alone["mirror"]["us"]
        add_d = (alone["stats"]["us"] + alone["stats_finalize"]["us"] + alone["combine_rescaled"]["us"]
                 + alone["mirror"]["us"])
        for name, add in (("C", add_c), ("D", add_d)):
            diff = (med[name] - med["B"]) * 1e3
            ok = diff <= 2 * add
            res[f"{name}_minus_B_us"], res[f"{name}_added_alone_us"], res[f"{name}_within_2x"] = diff, add, ok
            print(f"config {cfg}: {name} - B = {diff:.1f} us; its added launches alone {add:.1f} us; "
                  f"acceptance (<= 2x = {2 * add:.1f} us): {'met' if ok else 'NOT met'}", flush=True)
        if not args.no_volume:
            v_in = (torch.rand(VOLUMES[cfg], generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
            res["volume_wall"] = volume_walls(model, v_in, 3)
            w = res["volume_wall"]
            print(f"config {cfg} generate(v_in {VOLUMES[cfg]}, 'ddim', 50, target_depth=48) warm wall (s): "
                  + ", ".join(f"{k} {v['median_s']:.3f}" for k, v in w.items())
                  + f"; guided / unguided = {w['guided_s3']['median_s'] / w['unguided']['median_s']:.3f}", flush=True)
        model.invalidate_engine_cache()         # the next config builds its own programs
        out["configs"][str(cfg)] = res
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({c: {"step_ms": {k: round(v, 4) for k, v in r["step_ms"].items()},
                          "C_minus_B_us": round(r["C_minus_B_us"], 1), "D_minus_B_us": round(r["D_minus_B_us"], 1)}
                      for c, r in out["configs"].items()}))


if __name__ == "__main__":
    main()
