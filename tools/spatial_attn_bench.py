"""What SpatialAttention costs, measured in ONE process, alternated round-robin, bf16, random-init weights
(seed 0).  HIP events on the engine stream, medians after warm-up:

  core   ctsi_attn_plane and ctsi_attn_plane_bwd alone, in us and useful TFLOP/s (forward 4 N^2 hd, backward 10 N^2 hd per item
         -- the algorithm's flops; the two-pass backward executes 14), at the production shapes: C 256 / hd 64 @ 64x64,
         C 512 / hd 128 @ 32x32 and @ 16x16 (48 slices: config 2, 512^2), and the B = 4 training planes 24x24 / 12x12 / 6x6
         (config 3, 48 slices per sample).  q, k ~ N(0, 2), v ~ N(0, 1): random data (zeros collapse the softmax work).  Next to
         each, torch's F.scaled_dot_product_attention forward and backward on views of the same tensors on the same device
         (torch events on torch's stream), as a reference point.
  step   the captured config-2 DDIM step (latent (1,8,48,128,128)) for spatial_attention_levels () / [2, 3] / [1, 2, 3], and the
         time and flops of the sattn.* launches from an event-per-launch profile.
  train  one config-3 U-Net training micro-step (UNetTrainProgram at (4,8,48,48,48)) for () / [2, 3].

Sample quality is NOT measured: there are no trained weights.

usage: python tools/spatial_attn_bench.py [--replays 20] [--skip-train] [--skip-step] [--json out.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
PEAK_BF16_TFLOPS = 2500.0       # dense bf16 MFMA rate of the MI355X
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
# (n, C, heads, D, h, w)
CORE_SHAPES = [(1, 256, 4, 48, 64, 64), (1, 512, 4, 48, 32, 32), (1, 512, 4, 48, 16, 16),
               (4, 256, 4, 48, 24, 24), (4, 512, 4, 48, 12, 12), (4, 512, 4, 48, 6, 6)]
LEVEL_SETS = [(), (2, 3), (1, 2, 3)]


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


def _torch_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def core_times(shape, repeats):
    """The two entry points and torch's SDPA at `shape`, alternated; returns {name: dict(us, tflops)}."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    n, c, heads, d, h, w = shape
    nq, hd = h * w, c // heads
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr, P = ctx.lib, ctx.sptr, E._ptr
    useful = {"fwd": 4.0 * n * d * nq * nq * c, "bwd": 10.0 * n * d * nq * nq * c}
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = torch.randn((n * d, nq, 3, heads, hd), device=DEV, generator=g)
    qkv[:, :, :2] *= 2.0 ** 0.5
    qkv = qkv.to(torch.bfloat16)
    da = torch.randn((n * d, nq, heads, hd), device=DEV, generator=g).to(torch.bfloat16)
    out = torch.empty_like(da)
    dqkv = torch.empty_like(qkv)
    lse = torch.empty((n * d, heads, nq), dtype=torch.float32, device=DEV)

    def fwd():
        lib.attn_plane(P(qkv), P(out), P(lse), n, c, d, h, w, heads, sptr)

    def bwd():
        lib.attn_plane_bwd(P(qkv), P(out), P(da), P(lse), P(dqkv), n, c, d, h, w, heads, sptr)

    # torch's SDPA on views of the same tensors: (items, heads, N, hd)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).detach().requires_grad_(True) for i in range(3))
    go = da.permute(0, 2, 1, 3)
    sdpa = {}
    try:
        o = F.scaled_dot_product_attention(q, k, v)
        torch.autograd.grad(o, (q, k, v), go, retain_graph=True)
        sdpa["fwd"] = lambda: F.scaled_dot_product_attention(q, k, v)
        sdpa["bwd"] = lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True)
        err = float((o.detach().permute(0, 2, 1, 3).float() - 0).abs().mean())
    except Exception as exc:      # noqa: BLE001  (a reference point only: say why it is missing)
        sdpa, err = {}, None
        print(f"core {shape}: torch SDPA unavailable here: {type(exc).__name__}: {str(exc)[:120]}", flush=True)
    iters = max(2, min(50, int(2e12 // useful["bwd"]) + 1))
    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        ev = _Events(lib)
        fwd()
        bwd()
        torch.cuda.synchronize()
        if sdpa:
            rel = float((out.float() - o.detach().permute(0, 2, 1, 3).float()).norm() / o.detach().float().norm())
            res["agreement_with_sdpa_rel_l2"] = rel
        ts = {k_: [] for k_ in ("fwd", "bwd", "sdpa_fwd", "sdpa_bwd")}
        for r in range(repeats + 1):                            # alternated; the first round is warm-up
            t_f = ev.time_ms(sptr, lambda: [fwd() for _ in range(iters)]) / iters
            t_b = ev.time_ms(sptr, lambda: [bwd() for _ in range(iters)]) / iters
            t_sf = _torch_ms(sdpa["fwd"], iters) if sdpa else float("nan")
            t_sb = _torch_ms(sdpa["bwd"], iters) if sdpa else float("nan")
            if r:
                for k_, t in zip(ts, (t_f, t_b, t_sf, t_sb)):
                    ts[k_].append(t)
        ev.close()
    for k_, v_ in ts.items():
        us = statistics.median(v_) * 1e3
        fl = useful["fwd" if k_.endswith("fwd") else "bwd"]
        res[k_] = dict(us=us, tflops=fl / (us * 1e-6) / 1e12 if us == us else float("nan"))
    E.check_device_errors(ctx)
    return res


def _model(pkg, levels):
    torch.manual_seed(0)
    cfg = dict(FULL_CFG)
    if levels:
        cfg["unet_spatial_attention_levels"] = list(levels)
    model = pkg.VideoToVideoDiffusion(cfg).eval().to(DEV)
    for m in model.unet.modules():      # a zero proj_out would not change a timing, but keep the blocks' arithmetic live
        if type(m).__name__ == "SpatialAttention":
            torch.nn.init.normal_(m.proj_out.weight, std=0.02)
    return model


def step_times(pkg, models, shape, replays, warmup):
    """Median captured-replay time (ms) of the DDIM step per level set, alternated per round, and the sattn.* launches."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    n, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    g = pkg.GaussianDiffusion()
    t_ddim = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(50)]
    plan = S._step_plan(g, "ddim", t_ddim, 0.0, 2, None)
    progs = {}
    with ctx.scope():
        for levels, model in models.items():
            prog = E.UNetProgram(ctx, model.unet, n, d, h, w, (g.timesteps + 1) * n, "fast")
            prog.add_sampler_step(plan.kind, plan.with_noise)
            gen = torch.Generator().manual_seed(7)
            z = torch.randn((n, L, d, h, w), generator=gen)
            c = torch.randn((n, L, d, h, w), generator=gen)
            prog.load_latents(z.to(DEV), c.to(DEV))
            prog.set_schedule([t for t in plan.t for _ in range(n)], plan.coef.to(DEV), plan.pred)
            prog.capture()
            prog.step_ptr.zero_()
            progs[levels] = prog
        ev = _Events(ctx.lib)
        times = {k: [] for k in progs}
        for r in range(warmup + replays):
            for levels, prog in progs.items():
                prog.step_ptr.fill_(r % len(t_ddim))
                ms = ev.time_ms(ctx.sptr, prog.launch)
                if r >= warmup:
                    times[levels].append(ms)
        ev.close()
        prof = {}
        for levels, prog in progs.items():
            prog.step_ptr.zero_()
            rows = prog.profile_ops(repeats=3)
            agg = {}
            for r in rows:
                if r[0].startswith("sattn."):
                    a = agg.setdefault(r[0], [0, 0.0, 0.0])
                    a[0] += 1
                    a[1] += r[2]
                    a[2] += r[3]
            prof[levels] = dict(total_ms=sum(r[3] for r in rows), sattn=agg, flops=prog.flops, launches=len(rows))
    E.check_device_errors(ctx)
    del progs
    torch.cuda.empty_cache()
    return ({k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}, prof)


def train_times(pkg, models, shape, repeats, warmup):
    """One U-Net training micro-step (forward + backward launches, eager) per level set, alternated."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
    B, L, d, h, w = shape
    ctx = E.Ctx.get(torch.device(DEV))
    dev = torch.device(DEV)
    progs = {}
    with ctx.scope():
        for levels, model in models.items():
            model.train()
            prog = T.UNetTrainProgram(ctx, model.unet, B, d, h, w)
            prog.set_diffusion(model.diffusion)
            progs[levels] = prog
        gen = torch.Generator(device=DEV).manual_seed(3)
        z0, cond, noise = (torch.randn(shape, device=dev, generator=gen) for _ in range(3))
        t = torch.tensor([37, 412, 688, 951][:B], device=dev)
        norm = torch.full((B,), 1.0 / z0[0].numel() / B, device=dev)
        one = torch.ones(1, device=dev)
        ev = _Events(ctx.lib)
        times = {k: dict(fwd=[], bwd=[]) for k in progs}
        for r in range(warmup + repeats):
            for levels, prog in progs.items():
                f = ev.time_ms(ctx.sptr, lambda: prog.run_forward(z0, cond, t, noise, norm))
                b = ev.time_ms(ctx.sptr, lambda: prog.run_backward(one))
                if r >= warmup:
                    times[levels]["fwd"].append(f)
                    times[levels]["bwd"].append(b)
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
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spatial_attn_bench.py measures on a ROCm device; none is visible")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print("NOTE: random-init weights; sample quality with or without spatial attention is not measured.", flush=True)
    out = {"weights": "random init, torch.manual_seed(0)", "precision": "bf16", "replays": args.replays, "core": {}}
    for shape in CORE_SHAPES:
        res = core_times(shape, 5)
        out["core"]["x".join(str(v) for v in shape)] = res
        agree = res.pop("agreement_with_sdpa_rel_l2", None)
        for k in ("fwd", "bwd"):
            v, s = res[k], res["sdpa_" + k]
            print(f"core {shape} {k}: {v['us']:9.1f} us, {v['tflops']:7.1f} useful TFLOP/s "
                  f"({100 * v['tflops'] / PEAK_BF16_TFLOPS:.1f} % of the {PEAK_BF16_TFLOPS:.0f} TFLOP/s bf16 MFMA rate) | torch SDPA "
                  f"{s['us']:9.1f} us, {s['tflops']:7.1f} TFLOP/s | ours / SDPA time {v['us'] / s['us']:.2f}", flush=True)
        if agree is not None:
            print(f"core {shape}: forward rel-L2 to torch SDPA's bf16 output {agree:.2e}", flush=True)
        torch.cuda.empty_cache()
    models = None
    if not (args.skip_step and args.skip_train):
        models = {lv: _model(pkg, lv) for lv in LEVEL_SETS}
    if not args.skip_step:
        shape = (1, 8, 48, 128, 128)
        med, span, prof = step_times(pkg, models, shape, args.replays, args.warmup)
        out["step"] = dict(latent=shape, step_ms={str(k): v for k, v in med.items()},
                           step_ms_min_max={str(k): v for k, v in span.items()}, profile={str(k): v for k, v in prof.items()})
        for lv in med:
            p = prof[lv]
            tot = sum(v[2] for v in p["sattn"].values())
            print(f"config 2 latent {shape} levels {list(lv)}: captured DDIM step, median of {args.replays} replays "
                  f"{med[lv]:.3f} ms [{span[lv][0]:.3f}-{span[lv][1]:.3f}] ({med[lv] - med[()]:+.3f} ms against ()); "
                  f"{p['launches']} launches, {p['flops'] / 1e12:.3f} TFLOP; sattn.* launches {tot:.3f} ms in the event-per-launch "
                  "profile:", flush=True)
            for nm, (cnt, fl, ms) in p["sattn"].items():
                tf = f", {fl / 1e12:.3f} TFLOP at {fl / (ms * 1e-3) / 1e12:.0f} TFLOP/s" if fl else ""
                print(f"    {nm:20s} n={cnt:3d} {ms:8.3f} ms{tf}", flush=True)
        for m in models.values():
            m.invalidate_engine_cache()
    if not args.skip_train:
        tm = {lv: models[lv] for lv in LEVEL_SETS[:2]}
        tr = train_times(pkg, tm, (4, 8, 48, 48, 48), 5, 2)
        out["train"] = {str(k): v for k, v in tr.items()}
        for lv, v in tr.items():
            print(f"config 3 U-Net micro-step levels {list(lv)}: forward {v['fwd_ms']:.2f} ms + backward {v['bwd_ms']:.2f} ms = "
                  f"{v['fwd_ms'] + v['bwd_ms']:.2f} ms; {v['launches']} launches, {v['flops'] / 1e12:.2f} TFLOP, activation pool "
                  f"{v['pool_gib']:.2f} GiB", flush=True)
        base = tr[()]
        for lv, v in tr.items():
            if lv:
                dlt = (v["fwd_ms"] + v["bwd_ms"]) - (base["fwd_ms"] + base["bwd_ms"])
                print(f"config 3 U-Net micro-step: {list(lv)} - () = {dlt:+.2f} ms", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"core_tflops": {s: {k: round(v["tflops"], 1) for k, v in r.items() if isinstance(v, dict)}
                                      for s, r in out["core"].items()}}))


if __name__ == "__main__":
    main()
