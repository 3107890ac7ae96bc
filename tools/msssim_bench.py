"""What the device MS-SSIM loss (models.losses.MS_SSIM_Loss, csrc/msssim.hip) costs, against the same arithmetic as torch runs it
(the fp32 restatement of tests/msssim_restatement.py on the same device -- the reference's class is those torch ops).

  --mode loss   forward (no_grad) and forward + backward of both at (1,1,48,192,192), (1,1,8,192,192), (1,1,48,512,512);
                achieved bytes/s against the algorithmic traffic of the kernel form: per level-0 pixel
                forward 8 B read + 14 B written, backward 21 B read + 4 B written, all levels x 4/3 = 62.7 B; forward alone
                without the gradient's maps (8 + 2) x 4/3 = 13.3 B
  --mode vae    the VAE training step of tools/vae_train_bench.py's thin and thick shapes with (a) MSE only, (b) MSE + the torch
                restatement, (c) MSE + the device loss
  --mode trace  only the device loss, forward + backward --iters times at --shape (default the thin patch): run it under
                `rocprofv3 --kernel-trace --stats -- python tools/msssim_bench.py --mode trace` to count launches and read the
                kernels' own durations, or under `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --` (a run of its own)
The variants are ALTERNATED in one process, HIP events around each, warm, medians over the rounds with the min-max spread.

    python tools/msssim_bench.py --mode loss [--rounds 15] [--warmup 3] >> profiles/msssim_bench.log"""
import argparse
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")     # (as tests/conftest.py: no exhaustive MIOpen search for the baseline)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import formula_input, load_formula          # noqa: E402
from tests.msssim_restatement import msssim_loss, smooth_pair  # noqa: E402

DEV = "cuda:0"
B_FWD_BWD, B_FWD = (8 + 14 + 21 + 4) * 4 / 3, (8 + 2) * 4 / 3


def alternate(variants, rounds, warmup, before=None):
    """variants: [(name, fn)]; returns {name: sorted times in ms}"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in variants]
    times = {name: [] for name, _ in variants}
    for rnd in range(warmup + rounds):
        for i, (_, fn) in enumerate(variants):
            if before:
                before()
            ev[i][0].record()
            fn()
            ev[i][1].record()
        torch.cuda.synchronize()
        if rnd >= warmup:
            for i, (name, _) in enumerate(variants):
                times[name].append(ev[i][0].elapsed_time(ev[i][1]))
    return {k: sorted(v) for k, v in times.items()}


def show(name, ts, extra=""):
    print(f"  ({name:34s}) median {ts[len(ts) // 2]:8.3f} ms   min {ts[0]:8.3f}  max {ts[-1]:8.3f}   {extra}")
    return ts[len(ts) // 2]


def loss_mode(a, losses):
    m = losses.MS_SSIM_Loss()
    for shape in ((1, 1, 48, 192, 192), (1, 1, 8, 192, 192), (1, 1, 48, 512, 512)):
        pred, target = smooth_pair(shape, 0.1, 7, DEV)
        p = pred.clone().requires_grad_(True)
        npx = pred.numel()

        def hip_fwd():
            with torch.no_grad():
                m(pred, target)

        def hip_fb():
            p.grad = None
            m(p, target).backward()

        def torch_fwd():
            with torch.no_grad():
                msssim_loss(pred, target, torch.float32)

        def torch_fb():
            p.grad = None
            msssim_loss(p, target, torch.float32).backward()

        t = alternate([("device loss, forward", hip_fwd), ("torch restatement, forward", torch_fwd),
                       ("device loss, forward + backward", hip_fb), ("torch restatement, forward + backward", torch_fb)],
                      a.rounds, a.warmup)
        print(f"[{'x'.join(map(str, shape))}] {npx / 1e6:.2f} M pixels; {a.rounds} alternated rounds after {a.warmup} warm-up")
        hf = show("device loss, forward", t["device loss, forward"],
                  f"{B_FWD * npx / 1e6:.0f} MB -> {B_FWD * npx / (t['device loss, forward'][len(t['device loss, forward']) // 2] * 1e-3) / 1e12:.2f} TB/s")
        tf = show("torch restatement, forward", t["torch restatement, forward"])
        k = "device loss, forward + backward"
        hb = show(k, t[k], f"{B_FWD_BWD * npx / 1e6:.0f} MB -> {B_FWD_BWD * npx / (t[k][len(t[k]) // 2] * 1e-3) / 1e12:.2f} TB/s")
        tb = show("torch restatement, forward + backward", t["torch restatement, forward + backward"])
        print(f"  forward {tf / hf:.1f}x, forward + backward {tb / hb:.1f}x faster than the torch restatement -> "
              f"{'device loss wins' if hb < tb and hf < tf else 'device loss LOSES'}")


def vae_mode(a, pkg, losses):
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=1.0)
    load_formula(vae, 76)
    vae.train().to(DEV)
    m = losses.MS_SSIM_Loss()
    for depth in (48, 8):
        x = formula_input((1, 1, depth, 192, 192), 45).clamp(-1, 1).to(DEV)

        def step(term):
            def fn():
                recon, _ = vae(x)
                loss = F.mse_loss(recon, x)
                if term is not None:
                    loss = loss + 1.0 * term(recon, x)
                loss.backward()
            return fn

        t = alternate([("a  MSE only", step(None)),
                       ("b  MSE + torch restatement", step(lambda r, y: msssim_loss(r, y, torch.float32))),
                       ("c  MSE + device MS-SSIM loss", step(m))], a.rounds, a.warmup,
                      before=lambda: vae.zero_grad(set_to_none=True))
        print(f"[VAE base 128, latent 16, (1,1,{depth},192,192)] {a.rounds} alternated rounds after {a.warmup} warm-up")
        med = [show(k, v) for k, v in t.items()]
        print(f"  the term adds {med[2] - med[0]:.3f} ms per step on the device ({100 * (med[2] - med[0]) / med[0]:.1f} %), "
              f"{med[1] - med[0]:.3f} ms as torch ops ({100 * (med[1] - med[0]) / med[0]:.1f} %)")


def trace_mode(a, losses):
    m = losses.MS_SSIM_Loss()
    pred, target = smooth_pair(tuple(a.shape), 0.1, 7, DEV)
    p = pred.clone().requires_grad_(True)
    for _ in range(a.iters):
        p.grad = None
        m(p, target).backward()
    torch.cuda.synchronize()
    print(f"{a.iters} forward + backward passes of the device loss at {tuple(a.shape)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loss", "vae", "trace"), default="loss")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=5, default=[1, 1, 48, 192, 192])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_bench.py measures on a ROCm device; none is available")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    losses = importlib.import_module("models.losses")
    print(f"device {torch.cuda.get_device_name(0)}; mode {a.mode}; HIP events, host launch included")
    if a.mode == "loss":
        loss_mode(a, losses)
    elif a.mode == "vae":
        vae_mode(a, pkg, losses)
    else:
        trace_mode(a, losses)


if __name__ == "__main__":
    main()
