"""Times one VAE training micro-step on the HIP engine at config/vae_training.yaml's shape (base 128, latent 16, in_channels 1)
for a thin (1,1,48,192,192) and a thick (1,1,8,192,192) patch: forward and backward separately, the executed TFLOP and the
fraction of the 2.5 PFLOP/s bf16 dense peak; then the same step through the oracle (fp32 torch ops) under
torch.autocast(bf16) on the same device as a baseline.

    python tools/vae_train_bench.py [--steps 5] [--warmup 2] [--no-baseline] [--depths 48 8]
CTSI_VAE_THIN_WGRAD=0 switches the one-channel stem / head weight gradients to the MFMA kernel on padded channels (A/B)."""
import argparse
import importlib
import os
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")     # (as tests/conftest.py: no exhaustive MIOpen search for the baseline)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_ops as R                   # noqa: E402
from tests.helpers import formula_input, load_formula  # noqa: E402

PEAK = 2.5e15


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        ms.append(fn())
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--depths", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    dev = "cuda:0"
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=1.0)
    sd = load_formula(vae, 76)
    vae.train().to(dev)
    print(f"device {torch.cuda.get_device_name(0)}  thin-channel wgrad {'off' if os.environ.get('CTSI_VAE_THIN_WGRAD') == '0' else 'on'}")
    for depth in a.depths:
        x = formula_input((1, 1, depth, 192, 192), 45).clamp(-1, 1).to(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        split = []

        def step():
            vae.zero_grad(set_to_none=True)
            ev[0].record()
            recon, _ = vae(x)
            ev[1].record()
            F.mse_loss(recon, x).backward()
            ev[2].record()
            torch.cuda.synchronize()
            split.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
            return ev[0].elapsed_time(ev[2])

        t0 = time.time()
        step()
        build_s = time.time() - t0
        ms = timed(step, a.steps, a.warmup)
        fwd = sorted(s[0] for s in split[-a.steps:])[a.steps // 2]
        bwd = sorted(s[1] for s in split[-a.steps:])[a.steps // 2]
        prog = [p for k, p in vae.__dict__["_ctsi_programs"].items() if k[0] == "train" and k[3] == depth][0]
        n_fwd = prog.n_fwd
        fl_fwd = sum(m[1] for m in prog.op_meta[:n_fwd])
        fl_all = sum(m[1] for m in prog.op_meta)
        act_gb = sum(t.numel() * t.element_size() for t in prog.pool.all) / 1e9
        print(f"[depth {depth}] step {ms:.1f} ms (forward {fwd:.1f} ms, backward {bwd:.1f} ms; first call incl. build {build_s:.1f} s)")
        print(f"[depth {depth}] executed {fl_all / 1e12:.1f} TFLOP (forward {fl_fwd / 1e12:.1f}, backward {(fl_all - fl_fwd) / 1e12:.1f}) "
              f"-> {fl_all / (ms * 1e-3) / 1e12:.0f} TFLOP/s = {100 * fl_all / (ms * 1e-3) / PEAK:.1f} % of the bf16 peak; "
              f"activation + gradient buffers {act_gb:.1f} GB, peak allocated {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
        if not a.no_baseline:
            R.CONVT_AS_CONV = True
            sdd = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}

            def ref_step():
                for v in sdd.values():
                    v.grad = None
                ev[0].record()
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    recon = R.vae_decode(sdd, R.vae_encode(sdd, x, 1.0), 1.0)
                F.mse_loss(recon.float(), x).backward()
                ev[2].record()
                torch.cuda.synchronize()
                return ev[0].elapsed_time(ev[2])

            rms = timed(ref_step, max(2, a.steps // 2), 1)
            print(f"[depth {depth}] oracle under torch.autocast(bf16): {rms:.1f} ms per step -> engine speed-up {rms / ms:.2f}x")
            del sdd
        del prog
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
