"""fp32 inference mode on config 2 (generate(v_in (1,1,8,512,512), 'ddim', 50, target_depth=48), U-Net latent
(1,8,48,128,128)): the captured U-Net + DDIM step (HIP events), VAE encode and decode, the DDIM-50 volume, per-launch
TFLOP/s of the fp32 conv family against the f32 MFMA peak, and the fp32 torch oracle's volume on the same device.

usage: MIOPEN_FIND_MODE=FAST python tools/fp32_bench.py [--steps 50] [--repeats 5] [--no-oracle] [--json out.json]"""
import argparse
import importlib
import json
import os
import sys
import time
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_PEAK_TF = 157.3    # v_mfma_f32_32x32x2_f32: 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
DEV = "cuda:0"
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}


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


def _family(kernel, name):
    if "128x" not in kernel:
        return None
    if kernel.endswith("t"):
        return "ConvTranspose3d (3,4,4)"
    if kernel.endswith("d"):
        return "Conv3d (3,4,4) s2"
    if "1x1" in name or name in ("attn.pv", "res1x1", "dec.post_quant", "enc.quant"):
        return "Conv3d 1x1x1"
    return "Conv3d 3x3x3"


def conv_table(prog, repeats):
    rows = prog.profile_ops(repeats)
    fam = defaultdict(lambda: [0.0, 0.0, 0])
    per_launch = []
    for name, kernel, fl, ms in rows:
        if not kernel.startswith("conv_f32"):
            continue
        f = _family(kernel, name)
        fam[f][0] += fl
        fam[f][1] += ms
        fam[f][2] += 1
        per_launch.append((name, kernel, fl / 1e9, ms, fl / ms / 1e9 if ms > 0 else 0.0))
    total_ms = sum(r[3] for r in rows)
    return fam, per_launch, total_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    model.set_inference_precision("fp32")
    v_in = (torch.rand((1, 1, 8, 512, 512), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    noise_fn = lambda i, shape: torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i)).to(DEV)
    res = {"precision": "fp32", "config": "config 2: (1,1,8,512,512) -> 48 slices, DDIM-%d" % args.steps,
           "f32_peak_tflops": F32_PEAK_TF}

    # warm-up volume: builds and packs every program, captures the step graph
    t0 = time.time()
    model.generate(v_in, "ddim", num_inference_steps=args.steps, target_depth=48, noise_fn=noise_fn)
    torch.cuda.synchronize()
    res["first_volume_s"] = time.time() - t0
    vols = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.time()
        model.generate(v_in, "ddim", num_inference_steps=args.steps, target_depth=48, noise_fn=noise_fn)
        torch.cuda.synchronize()
        vols.append(time.time() - t0)
    res["volume_s"] = min(vols)
    res["volume_s_all"] = vols
    print(f"DDIM-{args.steps} volume (fp32 mode): {min(vols):.2f} s  (runs {['%.2f' % v for v in vols]}; first, with "
          f"program builds: {res['first_volume_s']:.1f} s)", flush=True)

    # the captured U-Net + sampler step
    progs = model.unet.__dict__["_ctsi_programs"]
    key = next(k for k in progs if k[0] == "sampler" and k[-1] == "fp32")
    sp = progs[key]
    ctx = sp.ctx

    def one_step():
        with torch.cuda.stream(ctx.stream):
            sp.step_ptr.zero_()
            sp.launch()
        torch.cuda.current_stream().wait_stream(ctx.stream)

    step_ms = _events_ms(one_step, args.repeats)
    res["unet_step_ms"] = min(step_ms)
    res["unet_step_flops"] = sp.flops
    res["unet_step_tflops"] = sp.flops / min(step_ms) / 1e9
    print(f"U-Net + DDIM step (captured graph): {min(step_ms):.1f} ms, {sp.flops / 1e12:.2f} TFLOP -> "
          f"{res['unet_step_tflops']:.1f} TF/s = {res['unet_step_tflops'] / F32_PEAK_TF:.3f} of the f32 peak", flush=True)

    # VAE legs
    ctxe = E.Ctx.get(torch.device(DEV))
    z_in = model.vae.encode(v_in)
    with ctxe.scope():
        z_cond = E.trilinear_depth(ctxe, z_in, 48)
    enc_ms = _events_ms(lambda: model.vae.encode(v_in), args.repeats)
    dec_ms = _events_ms(lambda: model.vae.decode(z_cond), max(2, args.repeats // 2))
    res["vae_encode_ms"], res["vae_decode_ms"] = min(enc_ms), min(dec_ms)
    print(f"VAE encode (1,1,8,512,512): {min(enc_ms):.1f} ms; decode (1,8,48,128,128) -> 512^2: {min(dec_ms):.1f} ms",
          flush=True)

    # per-launch conv table of the U-Net step and of the decoder
    dkey = next(k for k in model.vae.__dict__["_ctsi_programs"] if k[0] == "dec" and k[-1] == "fp32")
    for tag, prog in (("unet", sp), ("vae_decode", model.vae.__dict__["_ctsi_programs"][dkey])):
        with torch.cuda.stream(prog.ctx.stream):
            if tag == "unet":
                prog.step_ptr.zero_()
            fam, per_launch, total_ms = conv_table(prog, 1 if tag == "vae_decode" else 2)
        torch.cuda.synchronize()
        res[tag + "_families"] = {}
        print(f"\n{tag}: eager op sum {total_ms:.1f} ms; fp32 conv family (TFLOP/s, fraction of {F32_PEAK_TF} TF):")
        for f, (fl, ms, cnt) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
            tf = fl / ms / 1e9
            res[tag + "_families"][f] = dict(launches=cnt, gflop=fl / 1e9, ms=ms, tflops=tf, frac_peak=tf / F32_PEAK_TF)
            print(f"  {f:28s} {cnt:3d} launches  {fl / 1e12:8.3f} TFLOP  {ms:9.2f} ms  {tf:6.1f} TF/s  "
                  f"{tf / F32_PEAK_TF:.3f}")
        per_launch.sort(key=lambda r: -r[3])
        res[tag + "_top_launches"] = [dict(name=n, kernel=k, gflop=g, ms=m, tflops=t) for n, k, g, m, t in per_launch[:12]]
        for n, k, g, m, t in per_launch[:12]:
            print(f"    {n:18s} {k:26s} {g:9.1f} GFLOP {m:8.3f} ms {t:6.1f} TF/s")

    if not args.no_oracle:
        from oracle import ref_ops as R
        R.CONVT_AS_CONV = True
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        cfg = dict(model_channels=128, num_res_blocks=2, attention_levels=[1, 2], channel_mult=[1, 2, 4, 4],
                   num_heads=4, scaling_factor=1.0)
        R.generate(sd, cfg, v_in, "ddim", 2, 48, noise_fn=noise_fn)      # MIOpen solver search / warm-up
        torch.cuda.synchronize()
        t0 = time.time()
        R.generate(sd, cfg, v_in, "ddim", args.steps, 48, noise_fn=noise_fn)
        torch.cuda.synchronize()
        res["oracle_fp32_volume_s"] = time.time() - t0
        print(f"\nfp32 torch oracle, same volume: {res['oracle_fp32_volume_s']:.1f} s -> fp32 mode is "
              f"{res['oracle_fp32_volume_s'] / res['volume_s']:.2f}x faster", flush=True)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
