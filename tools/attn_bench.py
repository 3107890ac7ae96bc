"""What attention_mode='softmax' costs, measured in ONE process with both modes alternated round-robin,
bf16, random-init weights (seed 0).  HIP events on the engine stream, medians after warm-up:

  core   ctsi_attn_core and ctsi_attn_core_bwd alone at the three attention shapes of the production U-Net at config 2
         (C 256 @ 64x64, C 512 @ 32x32, C 512 @ 16x16, 48 slices, 4 heads), buffer sets rotated past the 256 MiB Infinity
         Cache, next to ctsi_attn_broadcast_add (the fast mode's closing pass: 4 C bytes per voxel) on the same shape in the
         same run: bytes / time of each.  Forward 8 C bytes per voxel (6 read, 2 written), backward 14 C (8 read, 6 written).
  step   the captured config-2 DDIM step (latent (1,8,48,128,128)), 'fast' against 'softmax', and an event-per-launch profile
         of the softmax program that says which launches of the 11 attention blocks the difference belongs to.
  train  one config-3 U-Net training micro-step (forward + backward launches of UNetTrainProgram at (4,8,48,48,48)) in both
         modes.

The yardstick of the step is the 'fast' step of the same process: the parent commit's behaviour.  Sample quality is NOT
measured: there are no trained weights.

usage: python tools/attn_bench.py [--replays 20] [--skip-train] [--json out.json]"""
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
CORE_SHAPES = [(1, 256, 4, 48, 64, 64), (1, 512, 4, 48, 32, 32), (1, 512, 4, 48, 16, 16)]    # (n, C, heads, D, h, w)
ATTN_OPS = ("gn.colsum", "gn.finalize", "gn.apply", "attn.qkv", "attn.core", "attn.proj", "attn.residual_add")


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


def core_times(shape, repeats):
    """The two core kernels and attn.broadcast_add alone at `shape`, alternated; returns {name: dict(us, bytes, tb_s)}."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    n, c, heads, d, h, w = shape
    vox = n * d * h * w
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    nbytes = {"attn_core": 8 * c * vox, "attn_core_bwd": 14 * c * vox, "attn_broadcast_add": 4 * c * vox + 2 * c * n * h * w}
    nsets = max(2, min(16, int(600e6 // (14 * c * vox)) + 1))
    sets = []
    for k in range(nsets):
        g = torch.Generator(device=DEV).manual_seed(k)
        qkv = torch.randn((vox, 3 * c), device=DEV, generator=g)
        qkv[:, :2 * c] *= 2.0 ** 0.5
        sets.append(dict(qkv=qkv.to(torch.bfloat16), da=torch.randn((vox, c), device=DEV, generator=g).to(torch.bfloat16),
                         out=torch.empty((vox, c), dtype=torch.bfloat16, device=DEV),
                         dqkv=torch.empty((vox, 3 * c), dtype=torch.bfloat16, device=DEV),
                         p=torch.randn((n * h * w, c), device=DEV, generator=g).to(torch.bfloat16)))
        del qkv

    def launch(kind, s):
        if kind == "attn_core":
            lib.attn_core(P(s["qkv"]), P(s["out"]), n, c, d, h, w, heads, sptr)
        elif kind == "attn_core_bwd":
            lib.attn_core_bwd(P(s["qkv"]), P(s["da"]), P(s["dqkv"]), n, c, d, h, w, heads, sptr)
        else:
            lib.attn_broadcast_add(P(s["da"]), P(s["p"]), None, heads, P(s["out"]), n, c, d, h, w, sptr)

    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        ev = _Events(lib)
        iters = 4 * nsets
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


def step_times(pkg, model, shape, replays, warmup):
    """Median captured-replay time (ms) of the DDIM step in both modes, alternated per round, and the per-launch profile."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    unet = model.unet
    n, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    g = pkg.GaussianDiffusion()
    t_ddim = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(50)]
    plan = S._step_plan(g, "ddim", t_ddim, 0.0, 2, None)
    progs = {}
    with ctx.scope():
        for mode in ("fast", "softmax"):
            prog = E.UNetProgram(ctx, unet, n, d, h, w, (g.timesteps + 1) * n, mode)
            prog.add_sampler_step(plan.kind, plan.with_noise)
            gen = torch.Generator().manual_seed(7)
            z = torch.randn((n, L, d, h, w), generator=gen)
            c = torch.randn((n, L, d, h, w), generator=gen)
            prog.load_latents(z.to(DEV), c.to(DEV))
            prog.set_schedule([t for t in plan.t for _ in range(n)], plan.coef.to(DEV), plan.pred)
            prog.capture()
            prog.step_ptr.zero_()
            progs[mode] = prog
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for mode, prog in progs.items():
                prog.step_ptr.fill_(r % len(t_ddim))
                ms = ev.time_ms(ctx.sptr, prog.launch)
                if r >= warmup:
                    times[mode].append(ms)
        ev.close()
        prof = {}
        for mode, prog in progs.items():
            prog.step_ptr.zero_()
            rows = prog.profile_ops(repeats=3)
            names = [r[0] for r in rows]
            agg = {}
            if mode == "softmax":
                for j, nm in enumerate(names):
                    if nm == "attn.qkv":                         # the block's seven launches sit at j - 3 .. j + 3
                        assert tuple(names[j - 3:j + 4]) == ATTN_OPS, names[j - 3:j + 4]
                        for k in range(j - 3, j + 4):
                            a = agg.setdefault(names[k], [0, 0.0, 0.0])
                            a[0] += 1
                            a[1] += rows[k][2]
                            a[2] += rows[k][3]
            else:
                for j, nm in enumerate(names):
                    if nm == "attn.depthsum":                    # depthsum, gn.finalize, pv, broadcast_add
                        assert names[j + 1] == "gn.finalize" and names[j + 3] == "attn.broadcast_add", names[j:j + 4]
                        for k in range(j, j + 4):
                            a = agg.setdefault(names[k], [0, 0.0, 0.0])
                            a[0] += 1
                            a[1] += rows[k][2]
                            a[2] += rows[k][3]
            prof[mode] = dict(total_ms=sum(r[3] for r in rows), attention=agg, flops=prog.flops, launches=len(rows))
    E.check_device_errors(ctx)
    del progs
    torch.cuda.empty_cache()
    return ({k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}, prof)


def train_times(pkg, model, shape, repeats, warmup):
    """One U-Net training micro-step (forward + backward launches, eager) in both modes, alternated."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
    B, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    dev = torch.device(DEV)
    progs = {}
    with ctx.scope():
        for mode in ("fast", "softmax"):
            model.unet.attention_mode = mode
            prog = T.UNetTrainProgram(ctx, model.unet, B, d, h, w)
            prog.set_diffusion(model.diffusion)
            progs[mode] = prog
        model.unet.attention_mode = "fast"
        gen = torch.Generator(device=DEV).manual_seed(3)
        z0, cond, noise = (torch.randn(shape, device=dev, generator=gen) for _ in range(3))
        t = torch.tensor([37, 412, 688, 951][:B], device=dev)
        norm = torch.full((B,), 1.0 / z0[0].numel() / B, device=dev)
        one = torch.ones(1, device=dev)
        ev = _Events(ctx.lib)
        times = {k: dict(fwd=[], bwd=[]) for k in progs}
        for r in range(warmup + repeats):
            for mode, prog in progs.items():
                f = ev.time_ms(ctx.sptr, lambda: prog.run_forward(z0, cond, t, noise, norm))
                b = ev.time_ms(ctx.sptr, lambda: prog.run_backward(one))
                if r >= warmup:
                    times[mode]["fwd"].append(f)
                    times[mode]["bwd"].append(b)
        ev.close()
        info = {m: dict(flops=p.flops, launches=len(p.ops), pool_gib=p.pool.total_bytes / 2 ** 30) for m, p in progs.items()}
    E.check_device_errors(ctx)
    del progs
    torch.cuda.empty_cache()
    return {m: dict(fwd_ms=statistics.median(v["fwd"]), bwd_ms=statistics.median(v["bwd"]), **info[m])
            for m, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench.py measures on a ROCm device; none is visible")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print("NOTE: random-init weights; sample quality of either attention mode is not measured.", flush=True)
    out = {"weights": "random init, torch.manual_seed(0)", "precision": "bf16", "replays": args.replays, "core": {}}
    for shape in CORE_SHAPES:
        res = core_times(shape, 5)
        out["core"]["x".join(str(v) for v in shape)] = res
        ba = res["attn_broadcast_add"]
        for k, v in res.items():
            print(f"core {shape} {k:20s}: {v['us']:8.1f} us, {v['bytes'] / 1e6:8.2f} MB, {v['tb_s']:.2f} TB/s "
                  f"({100 * v['share_of_hbm_peak']:.0f} % of 8 TB/s; {v['tb_s'] / ba['tb_s']:.2f} x the broadcast_add pass)",
                  flush=True)
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    shape = (1, 8, 48, 128, 128)
    med, span, prof = step_times(pkg, model, shape, args.replays, args.warmup)
    out["step"] = dict(latent=shape, step_ms=med, step_ms_min_max=span, profile=prof)
    print(f"config 2 latent {shape}: captured DDIM step, median of {args.replays} replays (ms): "
          + ", ".join(f"{k} {med[k]:.3f} [{span[k][0]:.3f}-{span[k][1]:.3f}]" for k in med)
          + f"; softmax - fast = {med['softmax'] - med['fast']:+.3f} ms", flush=True)
    for mode in ("fast", "softmax"):
        p = prof[mode]
        tot = sum(v[2] for v in p["attention"].values())
        print(f"config 2 {mode}: event-per-launch profile {p['total_ms']:.3f} ms over {p['launches']} launches, "
              f"{p['flops'] / 1e12:.3f} TFLOP; launches of the 11 attention blocks {tot:.3f} ms:", flush=True)
        for nm, (cnt, fl, ms) in p["attention"].items():
            tf = f", {fl / 1e12:.3f} TFLOP at {fl / (ms * 1e-3) / 1e12:.0f} TFLOP/s" if fl else ""
            print(f"    {nm:20s} n={cnt:3d} {ms:8.3f} ms{tf}", flush=True)
    model.invalidate_engine_cache()
    if not args.skip_train:
        model.train()
        tr = train_times(pkg, model, (4, 8, 48, 48, 48), 5, 2)
        out["train"] = tr
        for mode, v in tr.items():
            print(f"config 3 U-Net micro-step {mode}: forward {v['fwd_ms']:.2f} ms + backward {v['bwd_ms']:.2f} ms = "
                  f"{v['fwd_ms'] + v['bwd_ms']:.2f} ms; {v['launches']} launches, {v['flops'] / 1e12:.2f} TFLOP, activation pool "
                  f"{v['pool_gib']:.2f} GiB", flush=True)
        d = (tr["softmax"]["fwd_ms"] + tr["softmax"]["bwd_ms"]) - (tr["fast"]["fwd_ms"] + tr["fast"]["bwd_ms"])
        print(f"config 3 U-Net micro-step: softmax - fast = {d:+.2f} ms", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"step_ms": {k: round(v, 4) for k, v in med.items()},
                      "core_tb_s": {s: {k: round(v["tb_s"], 3) for k, v in r.items()} for s, r in out["core"].items()}}))


if __name__ == "__main__":
    main()
