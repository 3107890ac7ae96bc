"""DPM-Solver++(2M) against DDIM on config 2 (generate(v_in (1,1,8,512,512), sampler, N, target_depth=48), U-Net latent
(1,8,48,128,128)), random-init weights (seed 0):

  * warm volume wall time of generate() for DDIM-50 and DPM++(2M) at N = 10, 15, 20, 25 (bf16, the default precision);
  * the update kernels alone (ctsi_dpm_step / ctsi_ddim_step at the config-2 latent, HIP events, buffer sets rotated
    so that the bytes do not stay in the 256 MiB Infinity Cache) and their effective bandwidth;
  * each sampler's final latent (rel-L2) and decoded volume (PSNR, range 2) against a converged solution: fp32 mode,
    DPM++(2M) with --ref-steps (>= 250) steps, same conditioning and the same initial noise.

Random weights say nothing about quality on a trained checkpoint: a random U-Net's eps is not the score of any data, so
these distances only show how far each discretisation is from the converged ODE solution of THIS network.

usage: python tools/dpm_bench.py [--ref-steps 250] [--repeats 3] [--json out.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
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
DPM_STEPS = (10, 15, 20, 25)


def _noise_fn(i, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i), dtype=torch.float32).to(DEV)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _psnr(a, b, rng=2.0):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else 10.0 * torch.log10(torch.tensor(rng * rng / mse)).item()


def step_kernel_bandwidth(pkg, shape, repeats):
    """ctsi_dpm_step and ctsi_ddim_step at `shape` (n, L, d, h, w) in the engine's layout (fp32 NDHWC state, bf16
    [z | cond] U-Net input), timed with HIP events on the engine stream over launches that rotate through buffer sets
    larger than the Infinity Cache.  Bytes: DPM 22 per element (z r/w, eps r, x0_prev r/w, bf16 input w), DDIM 14."""
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    g = pkg.GaussianDiffusion()
    n, L, d, h, w = shape
    numel = n * L * d * h * w
    ctx = E.Ctx.get(torch.device(DEV))
    lib, sptr = ctx.lib, ctx.sptr
    t_desc = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(20)]
    dpm = S.dpm_coef_rows(g.alphas_cumprod, t_desc, 2).to(DEV)
    ddim = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).to(DEV)
    step = torch.full((1,), 5, dtype=torch.int32, device=DEV)          # a second-order row (c != 0)
    nf = torch.zeros((len(t_desc) + 2, 6), dtype=torch.int32, device=DEV)
    sets = []
    for k in range(8):                                                  # 8 x 101 MB > 256 MiB
        gen = torch.Generator(device=DEV).manual_seed(k)
        sets.append(dict(z=torch.randn((n, d, h, w, L), device=DEV, generator=gen),
                         eps=torch.randn((n, d, h, w, L), device=DEV, generator=gen),
                         x0=torch.zeros((n, d, h, w, L), device=DEV),
                         zin=torch.zeros((n, d, h, w, 2 * L), dtype=torch.bfloat16, device=DEV)))
    P = E._ptr

    def launch(kind, s):
        if kind == "dpm":
            lib.dpm_step(P(s["z"]), P(s["eps"]), P(s["x0"]), P(s["zin"]), 2 * L, 0, P(dpm), P(step), n, L, d, h, w,
                         P(nf), sptr)
        else:
            lib.ddim_step(P(s["z"]), P(s["eps"]), None, P(s["zin"]), 2 * L, 0, P(ddim), P(step), n, L, d, h, w, P(nf),
                          sptr)

    evs = []
    for _ in range(2):
        e = C.c_void_p()
        lib.event_create(C.byref(e))
        evs.append(e)
    res = {}
    torch.cuda.synchronize()
    with ctx.scope():
        for kind, nbytes in (("dpm", 22), ("ddim", 14), ("dpm", 22)):   # alternated; the second dpm pass is reported
            iters = 20 * len(sets)
            for s in sets:
                launch(kind, s)
            times = []
            for _ in range(repeats):
                lib.event_record(evs[0], sptr)
                for i in range(iters):
                    launch(kind, sets[i % len(sets)])
                lib.event_record(evs[1], sptr)
                ms = C.c_float()
                lib.event_elapsed_ms(evs[0], evs[1], C.byref(ms))
                times.append(ms.value / iters)
            us = min(times) * 1e3
            res[kind] = dict(us=us, us_all=[t * 1e3 for t in times], bytes=nbytes * numel,
                             tb_s=nbytes * numel / (us * 1e-6) / 1e12,
                             share_of_hbm_peak=nbytes * numel / (us * 1e-6) / 1e9 / PEAK_HBM_GBS)
    for e in evs:
        lib.event_destroy(e)
    torch.cuda.synchronize()
    del sets
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-steps", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.ref_steps < 250:
        raise SystemExit("--ref-steps must be >= 250 (the converged solution)")
    if not torch.cuda.is_available():
        raise SystemExit("dpm_bench.py measures on a ROCm device; none is visible")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    hw, lat = args.hw, args.hw // 4
    print("NOTE: random-init weights.  The distances below compare discretisations of one random network's ODE; they say "
          "nothing about sample quality on a trained checkpoint.", flush=True)
    out = {"workload": f"generate(v_in (1,1,8,{hw},{hw}), sampler, N, target_depth=48), latent (1,8,48,{lat},{lat})",
           "weights": "random init, torch.manual_seed(0)"}

    out["step_kernel"] = step_kernel_bandwidth(pkg, (1, 8, 48, lat, lat), 5)
    for k, v in out["step_kernel"].items():
        print(f"step kernel {k}: {v['us']:.1f} us, {v['bytes'] / 1e6:.1f} MB, {v['tb_s']:.2f} TB/s effective "
              f"({100 * v['share_of_hbm_peak']:.0f} % of 8 TB/s)", flush=True)

    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    v_in = (torch.rand((1, 1, 8, hw, hw), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    runs = [("ddim", 50)] + [("dpmpp_2m", n) for n in DPM_STEPS]

    # (1) warm volume wall time, bf16 (the default precision)
    walls = {}
    for name, n in runs:
        model.generate(v_in, name, n, target_depth=48, noise_fn=_noise_fn)            # plans, weight pack, capture
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            model.generate(v_in, name, n, target_depth=48, noise_fn=_noise_fn)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        walls[f"{name}-{n}"] = dict(best_s=min(ts), all_s=ts)
        print(f"volume wall {name}-{n} (bf16): {min(ts):.3f} s  (runs {', '.join(f'{t:.3f}' for t in ts)})", flush=True)
    out["volume_wall_bf16"] = walls

    # (2) distance to the converged solution: final latent and decoded volume, per precision
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    ctx = E.Ctx.get(torch.device(DEV))

    def latent_and_volume(name, n, precision):
        model.set_inference_precision(precision)
        try:
            z_in = model.vae.encode(v_in)
            with ctx.scope():
                z_cond = E.trilinear_depth(ctx, z_in, 48)
            shape = tuple(z_cond.shape)
            sp = (S.DDIMSampler(model.diffusion, model.unet) if name == "ddim"
                  else S.DPMSolverSampler(model.diffusion, model.unet, order=2))
            t0 = time.perf_counter()
            z0 = sp.sample(shape, z_cond, n, DEV, progress=False, noise_fn=_noise_fn)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            vol = model.vae.decode(z0)
            torch.cuda.synchronize()
            return z0.cpu(), vol.cpu(), dt
        finally:
            model.set_inference_precision("bf16")

    z_ref, v_ref, dt = latent_and_volume("dpmpp_2m", args.ref_steps, "fp32")
    print(f"converged solution: fp32 DPM++(2M)-{args.ref_steps}, sampler {dt:.1f} s", flush=True)
    out["converged"] = dict(sampler="dpmpp_2m", steps=args.ref_steps, precision="fp32", sampler_s=dt)
    dist = {}
    for precision in ("fp32", "bf16"):
        for name, n in runs:
            z0, vol, dt = latent_and_volume(name, n, precision)
            key = f"{name}-{n}/{precision}"
            dist[key] = dict(latent_rel_l2=_rel(z0, z_ref), decoded_psnr_db=_psnr(vol, v_ref), sampler_s=dt)
            print(f"{key:20s} latent rel-L2 {dist[key]['latent_rel_l2']:.3e}  decoded PSNR "
                  f"{dist[key]['decoded_psnr_db']:6.2f} dB  vs converged", flush=True)
    out["vs_converged"] = dist
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"volume_wall_bf16_best_s": {k: round(v["best_s"], 4) for k, v in walls.items()},
                      "step_kernel_tb_s": {k: round(v["tb_s"], 2) for k, v in out["step_kernel"].items()}}))


if __name__ == "__main__":
    main()
