"""bf16x3 inference mode against fp32 and bf16, in one process, alternating fp32 / bf16x3 / bf16 in every round:

  * the captured U-Net + DDIM step at config 2 (latent (1,8,48,128,128)) and config 1 ((1,8,48,48,48)), HIP events
  * VAE encode and decode at 512^2 and 192^2
  * the DDIM-N config-2 volume, generate() wall-clock
  * useful TFLOP/s per conv family (3x3x3, 1x1x1, strided, transposed) of the fp32 and bf16x3 kernels, per-op eager timing
  * accuracy at the real size against the fp32 ENGINE (float64 is too slow there): the config-2 U-Net output, the final
    DDIM-N latent and the decoded volume in dB, for bf16x3 and for bf16.  Reported, not asserted.

usage: python tools/x3_bench.py [--steps 50] [--rounds 3] [--json out.json]"""
import argparse
import importlib
import json
import math
import os
import sys
import time
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_PEAK_TF = 157.3            # v_mfma_f32_32x32x2_f32: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
X3_PEAK_TF = 2500.0 / 3.0      # bf16 MFMA peak / 3 products = 833 TF of useful work
DEV = "cuda:0"
PRECISIONS = ("fp32", "bf16x3", "bf16")
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
CONFIGS = {"config2": (512, (48, 128, 128)), "config1": (192, (48, 48, 48))}


def _events_ms(fn, repeats):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _psnr(a, b, rng=2.0):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return math.inf if mse == 0 else 10.0 * math.log10(rng * rng / mse)


def _family(kernel, name):
    if kernel.endswith("t"):
        return "ConvTranspose3d (3,4,4)"
    if kernel.endswith("d"):
        return "Conv3d (3,4,4) s2"
    if "1x1" in name or name in ("attn.pv", "res1x1", "dec.post_quant", "enc.quant"):
        return "Conv3d 1x1x1"
    return "Conv3d 3x3x3"


def conv_families(prog, prefix, repeats):
    fam = defaultdict(lambda: [0.0, 0.0, 0])
    for name, kernel, fl, ms in prog.profile_ops(repeats):
        if kernel.startswith(prefix) and "128x" in kernel:
            f = fam[_family(kernel, name)]
            f[0] += fl
            f[1] += ms
            f[2] += 1
    return fam


def _sampler_prog(unet, precision, dims):
    progs = unet.__dict__["_ctsi_programs"]
    key = next(k for k in progs if k[0] == "sampler" and precision in k and tuple(k[3:6]) == tuple(dims))
    return progs[key]


def _vae_prog(vae, which, precision, dims):
    progs = vae.__dict__["_ctsi_programs"]
    key = next(k for k in progs if k[0] == which and k[-1] == precision and tuple(k[3:6]) == tuple(dims))
    return progs[key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    # three precisions x two configs x (sampler, forward) programs stay alive side by side: the per-module program cache (an LRU of 4
    # by default, CTSI_PROGRAM_CACHE) must hold them all, or a round would time a rebuild
    E.PROGRAM_CACHE_SIZE = max(E.PROGRAM_CACHE_SIZE, 32)
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    ctx = E.Ctx.get(torch.device(DEV))
    noise_fn = lambda i, shape: torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i)).to(DEV)
    v_ins = {c: (torch.rand((1, 1, 8, hw, hw), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
             for c, (hw, _) in CONFIGS.items()}
    res = {"steps": args.steps, "rounds": args.rounds, "order": list(PRECISIONS), "f32_peak_tflops": F32_PEAK_TF,
           "bf16x3_useful_peak_tflops": X3_PEAK_TF}

    # ---- warm-up: one volume per (config, precision) builds every program and captures the step graph.  At config 2 it is the
    # full DDIM-N run, whose final latent (the decoder's input) and volume are kept for the accuracy table.
    latents, volumes = {}, {}
    for cname in CONFIGS:
        steps = args.steps if cname == "config2" else 2
        for prec in PRECISIONS:
            seen = []
            decode = model.vae.decode
            model.vae.decode = lambda z, _d=decode, _s=seen: (_s.append(z.clone()), _d(z))[1]
            try:
                t0 = time.time()
                out = model.generate(v_ins[cname], "ddim", num_inference_steps=steps, target_depth=48, noise_fn=noise_fn,
                                     precision=prec)
                torch.cuda.synchronize()
            finally:
                del model.vae.decode
            print(f"warm-up {cname} {prec}: DDIM-{steps} volume with program builds {time.time() - t0:.1f} s", flush=True)
            if cname == "config2":
                latents[prec], volumes[prec] = seen[0], out
            del out

    # ---- accuracy at the real size, against the fp32 engine
    x = torch.randn((1, 8, 48, 128, 128), generator=torch.Generator().manual_seed(5)).to(DEV)
    c = torch.randn((1, 8, 48, 128, 128), generator=torch.Generator().manual_seed(6)).to(DEV)
    t = torch.tensor([500], device=DEV)
    eps = {}
    for prec in PRECISIONS:
        model.unet.inference_precision = prec
        eps[prec] = model.unet(x, t, c)
    model.unet.inference_precision = "bf16"
    res["accuracy_vs_fp32_engine"] = {}
    print(f"\naccuracy at config 2 against the fp32 engine (DDIM-{args.steps}):")
    for prec in ("bf16x3", "bf16"):
        row = dict(unet_output_rel_l2=_rel_l2(eps[prec], eps["fp32"]), final_latent_rel_l2=_rel_l2(latents[prec], latents["fp32"]),
                   decoded_volume_psnr_db=_psnr(volumes[prec], volumes["fp32"]))
        res["accuracy_vs_fp32_engine"][prec] = row
        print(f"  {prec:7s} U-Net output rel-L2 {row['unet_output_rel_l2']:.3g}   final latent rel-L2 "
              f"{row['final_latent_rel_l2']:.3g}   decoded volume {row['decoded_volume_psnr_db']:.2f} dB", flush=True)
    del eps, x, c, latents, volumes

    # ---- timings, alternating the three precisions in every round
    timings = defaultdict(list)
    z_conds = {}
    for cname, (hw, dims) in CONFIGS.items():
        z_in = model.vae.encode(v_ins[cname])
        with ctx.scope():
            z_conds[cname] = E.trilinear_depth(ctx, z_in, 48)
    for _ in range(args.rounds):
        for prec in PRECISIONS:
            model.set_inference_precision(prec)
            for cname, (hw, dims) in CONFIGS.items():
                sp = _sampler_prog(model.unet, prec, dims)

                def one_step(sp=sp):
                    with torch.cuda.stream(sp.ctx.stream):
                        sp.step_ptr.zero_()
                        sp.launch()
                    torch.cuda.current_stream().wait_stream(sp.ctx.stream)

                timings[cname, "step", prec] += _events_ms(one_step, 3)
                timings[cname, "encode", prec] += _events_ms(lambda: model.vae.encode(v_ins[cname]), 1)
                timings[cname, "decode", prec] += _events_ms(lambda: model.vae.decode(z_conds[cname]), 1)
    model.set_inference_precision("bf16")
    for r in range(max(1, args.rounds - 1)):
        for prec in PRECISIONS:
            torch.cuda.synchronize()
            t0 = time.time()
            model.generate(v_ins["config2"], "ddim", num_inference_steps=args.steps, target_depth=48, noise_fn=noise_fn,
                           precision=prec)
            torch.cuda.synchronize()
            timings["config2", "volume_s", prec].append(time.time() - t0)
    res["timings"] = {}
    print(f"\ntimings, min over {args.rounds} alternating rounds (spread = max - min over all replays of the run):")
    for cname, (hw, dims) in CONFIGS.items():
        for what in ("step", "encode", "decode") + (("volume_s",) if cname == "config2" else ()):
            unit = "s" if what == "volume_s" else "ms"
            row = {p: dict(min=min(timings[cname, what, p]), spread=max(timings[cname, what, p]) - min(timings[cname, what, p]),
                           n=len(timings[cname, what, p])) for p in PRECISIONS}
            res["timings"][f"{cname}.{what}"] = row
            f32, x3, bf = (row[p]["min"] for p in PRECISIONS)
            print(f"  {cname} {hw}^2 {what:8s} " + "  ".join(f"{p} {row[p]['min']:9.2f} {unit} (spread {row[p]['spread']:.2f})"
                                                               for p in PRECISIONS)
                  + f"   fp32 / bf16x3 = {f32 / x3:.2f}x, bf16x3 / bf16 = {x3 / bf:.2f}x", flush=True)
    for cname in CONFIGS:
        row = res["timings"][f"{cname}.step"]
        gain = row["fp32"]["min"] - row["bf16x3"]["min"]
        spread = max(row["fp32"]["spread"], row["bf16x3"]["spread"])
        res[f"{cname}_step_gain_exceeds_spread"] = bool(gain > spread)
        print(f"  {cname}: the bf16x3 step is {gain:.2f} ms faster than the fp32 step; replay-to-replay spread {spread:.2f} ms -> "
              f"{'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}")

    # ---- useful TFLOP/s per conv family: the config-2 step program and the 512^2 decoder, per-op eager timing
    res["families"] = {}
    for prec, prefix, peak in (("fp32", "conv_f32", F32_PEAK_TF), ("bf16x3", "conv_bf16x3", X3_PEAK_TF)):
        model.set_inference_precision(prec)
        for tag, prog in (("unet_step", _sampler_prog(model.unet, prec, CONFIGS["config2"][1])),
                          ("vae_decode", _vae_prog(model.vae, "dec", prec, CONFIGS["config2"][1]))):
            with torch.cuda.stream(prog.ctx.stream):
                if tag == "unet_step":
                    prog.step_ptr.zero_()
                fam = conv_families(prog, prefix, 1 if prec == "fp32" else 2)
            torch.cuda.synchronize()
            print(f"\n{prec} {tag}: useful TFLOP/s per conv family (fraction of {peak:.1f} TF):")
            for f, (fl, ms, cnt) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
                tf = fl / ms / 1e9
                res["families"][f"{prec}.{tag}.{f}"] = dict(launches=cnt, gflop=fl / 1e9, ms=ms, tflops=tf, frac_peak=tf / peak)
                print(f"  {f:28s} {cnt:3d} launches  {fl / 1e12:8.3f} TFLOP  {ms:9.2f} ms  {tf:7.1f} TF/s  {tf / peak:.3f}",
                      flush=True)
    model.set_inference_precision("bf16")
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
