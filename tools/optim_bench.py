"""What the EMA of the weights and global-norm clipping cost per optimizer step, fused into the update launch against the
separate passes they replace, on the config-3 U-Net parameter set (264.66 M parameters, random fp32 gradients; no forward).

Alternates in ONE process, HIP events around each variant, warm, medians over the rounds (and the min-max spread, which is what
a difference between two rows has to exceed):
  (a) FusedAdamW.step()                                   (b) (a) + torch._foreach_lerp_ over the shadows
  (c) FusedAdamW(ema=...).step()                          (d) torch.nn.utils.clip_grad_norm_ + (a)
  (e) FusedAdamW(max_grad_norm=...).step()                (f) FusedAdamW(ema=..., max_grad_norm=...).step()
and, for users of a torch optimizer, the stand-alone launches: (g) EMAWeights.update(), (h) clip_grad_norm_ of this package.
The gradients are restored between variants (outside the timed windows), so every variant clips the same gradients.

    python tools/optim_bench.py [--rounds 15] [--warmup 3] > profiles/optim_ema_bench.log"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py measures on a ROCm device; none is available")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    unet = pkg.UNet3D(latent_dim=8).to(dev)
    params = [p for p in unet.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    gen = torch.Generator(device=dev).manual_seed(1)
    grads0 = [torch.randn(p.shape, device=dev, generator=gen) * 1e-3 for p in params]
    for p, g in zip(params, grads0):
        p.grad = g.clone()
    grads = [p.grad for p in params]
    norm = float(torch.linalg.vector_norm(torch.cat([g.double().reshape(-1) for g in grads0])))
    clip = 0.5 * norm                                        # every clipping variant really scales
    kw = dict(lr=1e-7, weight_decay=0.01)
    named = lambda: list(unet.named_parameters())
    o_a = pkg.FusedAdamW(params, **kw)
    o_c = pkg.FusedAdamW(params, ema=pkg.EMAWeights(named()), **kw)
    o_e = pkg.FusedAdamW(params, max_grad_norm=clip, **kw)
    o_f = pkg.FusedAdamW(params, ema=pkg.EMAWeights(named()), max_grad_norm=clip, **kw)
    shadows = [p.detach().clone() for p in params]
    datas = [p.detach() for p in params]
    ema_g = pkg.EMAWeights(named())

    def v_b():
        o_a.step()
        torch._foreach_lerp_(shadows, datas, 1e-4)

    def v_d():
        torch.nn.utils.clip_grad_norm_(params, clip)
        o_a.step()

    def v_h():
        pkg.clip_grad_norm_(params, clip)
        o_a.step()

    variants = [("a  FusedAdamW.step()", o_a.step, 28), ("b  (a) + torch._foreach_lerp_", v_b, 40),
                ("c  fused step with EMA", o_c.step, 36), ("d  torch clip_grad_norm_ + (a)", v_d, None),
                ("e  fused clipped step", o_e.step, 32), ("f  fused step, EMA + clipping", o_f.step, 40),
                ("g  EMAWeights.update() alone", ema_g.update, 12), ("h  this package's clip_grad_norm_ + (a)", v_h, 40)]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in variants]
    times = [[] for _ in variants]
    for rnd in range(a.warmup + a.rounds):
        for i, (_, fn, _) in enumerate(variants):
            torch._foreach_copy_(grads, grads0)              # (outside the timed window)
            ev[i][0].record()
            fn()
            ev[i][1].record()
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            for i in range(len(variants)):
                times[i].append(ev[i][0].elapsed_time(ev[i][1]))
    print(f"device {torch.cuda.get_device_name(0)}; {len(params)} tensors, {n / 1e6:.2f} M parameters; gradient norm {norm:.6g}, "
          f"max_grad_norm {clip:.6g}; {a.rounds} alternated rounds after {a.warmup} warm-up rounds; HIP events, host launch included")
    print(f"fused clipped step: norm {float(o_e.last_grad_norm):.9g} (float64 {norm:.9g})")
    med = []
    for (name, _, bpe), ts in zip(variants, times):
        ts = sorted(ts)
        m = ts[len(ts) // 2]
        med.append(m)
        rate = f"{bpe} B/element -> {bpe * n / (m * 1e-3) / 1e12:5.2f} TB/s" if bpe else "(torch: several passes)"
        print(f"({name:40s}) median {m:7.3f} ms   min {ts[0]:7.3f}  max {ts[-1]:7.3f}   {rate}")
    print(f"c / a = {med[2] / med[0]:.3f} (36/28 = {36 / 28:.3f} from bytes);  e - a = {med[4] - med[0]:.3f} ms "
          f"(4/28 of a = {med[0] * 4 / 28:.3f} ms from bytes)")
    print(f"fused EMA step vs step + foreach lerp:   c {med[2]:.3f} ms vs b {med[1]:.3f} ms -> {'c wins' if med[2] < med[1] else 'c LOSES'}")
    print(f"fused clipped step vs torch clip + step: e {med[4]:.3f} ms vs d {med[3]:.3f} ms -> {'e wins' if med[4] < med[3] else 'e LOSES'}")


if __name__ == "__main__":
    main()
