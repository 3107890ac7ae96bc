"""What the device VGG-19 perceptual loss (models.losses.VGGPerceptualLoss, vgg_loss_engine.py) costs, forward + backward.

  --mode loss   at (4,1,48,192,192) and (1,1,48,512,512), slice_sample_rate 0.2, ALTERNATED in one process:
                  (a) the engine's loss as planned (the planar (1,3,3) form of the k32 halo-tile kernel where the plan picks it),
                  (b) the same with CTSI_CONV_PLANAR=0: every conv on the gather kernel, ReLU as a pass of its own,
                  (c) the restatement (tests/vgg_restatement.py) as torch ops under bf16 autocast on the device;
                then, per conv launch of (a) and (b) (HIP events around every op, engine.Program.profile_ops): milliseconds,
                TFLOP/s from the algorithmic FLOPs of the layer and the fraction of the 2.5 PFLOP/s bf16 peak.  A layer whose
                planar launch is slower than its gather launch is flagged: the plan should keep it on the gather kernel.
  --mode vae    one VAE training step (base 128, latent 16) at (1,1,48,192,192) and (1,1,8,192,192) with (a) MSE only, (b) MSE +
                0.1 x the torch restatement under autocast, (c) MSE + 0.1 x the device loss -- as tools/msssim_bench.py
                measures its term.
Weights are He-normal random numbers (no trained VGG weights ship with the project; the arithmetic does not depend on them).

    python tools/vgg_bench.py --mode loss [--rounds 9] [--warmup 2] >> profiles/perceptual_bench.log"""
import argparse
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")     # (as tests/conftest.py: no exhaustive MIOpen search for the baseline)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import formula_input, load_formula                                # noqa: E402
from tests.vgg_restatement import Restatement, he_state_dict, smooth_volume         # noqa: E402
from tools.msssim_bench import alternate, show                                       # noqa: E402

DEV = "cuda:0"
PEAK = 2.5e15


def build(losses, sd, planar: bool, pred, target):
    """A loss module whose programs were planned with / without the planar form (the override is read when a plan is made)."""
    old = os.environ.pop("CTSI_CONV_PLANAR", None)
    if not planar:
        os.environ["CTSI_CONV_PLANAR"] = "0"
    try:
        m = losses.VGGPerceptualLoss(weights=sd).to(DEV)
        p = pred.clone().requires_grad_(True)
        m(p, target).backward()              # builds and packs
        torch.cuda.synchronize()
    finally:
        os.environ.pop("CTSI_CONV_PLANAR", None)
        if old is not None:
            os.environ["CTSI_CONV_PLANAR"] = old
    return m


def per_layer(m):
    prog = [p for v in m._ctsi_programs.values() for p in v][0]
    with prog.ctx.scope():
        rows = prog.profile_ops(repeats=5)
    torch.cuda.synchronize()
    return {name: (kernel, flops, ms) for name, kernel, flops, ms in rows}, prog


def loss_mode(a, losses):
    sd = he_state_dict(1234, upto=30)
    for shape in ((4, 1, 48, 192, 192), (1, 1, 48, 512, 512)):
        pred, target = smooth_volume(shape, 7).to(DEV), smooth_volume(shape, 8).to(DEV)
        m_p, m_g = build(losses, sd, True, pred, target), build(losses, sd, False, pred, target)
        r = Restatement(sd, rate=0.2, dtype=torch.float32, device=DEV)
        p = pred.clone().requires_grad_(True)

        def run(m):
            def fn():
                p.grad = None
                m(p, target).backward()
            return fn

        def torch_fb():
            p.grad = None
            r(p, target, autocast=True).backward()

        t = alternate([("a  engine, planar form", run(m_p)), ("b  engine, gather kernel", run(m_g)),
                       ("c  torch ops, bf16 autocast", torch_fb)], a.rounds, a.warmup)
        rows_p, prog = per_layer(m_p)
        rows_g, _ = per_layer(m_g)
        n_img = prog.n_img
        print(f"[{'x'.join(map(str, shape))}] {n_img} sampled slices (2 x {n_img} images through the stack); {a.rounds} alternated "
              f"rounds after {a.warmup} warm-up; forward + backward; conv work {prog.flops / 1e12:.2f} TFLOP")
        med = [show(k, v) for k, v in t.items()]
        print(f"  planar form {med[1] / med[0]:.2f}x the gather kernel's speed, {med[2] / med[0]:.2f}x the torch run's; "
              f"whole loss {prog.flops / (med[0] * 1e-3) / 1e12:.0f} TFLOP/s = {100 * prog.flops / (med[0] * 1e-3) / PEAK:.1f} % of peak")
        print(f"  {'conv launch':18s} {'kernel (a)':26s} {'ms (a)':>8s} {'TFLOP/s':>8s} {'of peak':>8s}   {'kernel (b)':26s} {'ms (b)':>8s}")
        slower = []
        for name, (kernel, flops, ms) in rows_p.items():
            if not kernel.startswith("conv_"):
                continue
            kg, _, msg = rows_g[name]
            # (b) pays its ReLU as a separate pass: count it with the conv it follows
            idx = name.split(".")[1]
            extra = rows_g.get(f"vgg.{int(idx) + 1}.relu", (None, 0, 0.0))[2] if (".dgrad" not in name and f"vgg.{int(idx) + 1}.relu" not in rows_p) else 0.0
            flag = ""
            if kernel.endswith("m9p") and ms > msg + extra:
                flag = "  <-- planar slower"
                slower.append(name)
            print(f"  {name:18s} {kernel:26s} {ms:8.3f} {flops / (ms * 1e-3) / 1e12:8.0f} {100 * flops / (ms * 1e-3) / PEAK:7.1f}%   "
                  f"{kg:26s} {msg + extra:8.3f}{flag}")
        other_p = sum(ms for _, (k, _, ms) in rows_p.items() if not k.startswith("conv_"))
        other_g = sum(ms for _, (k, _, ms) in rows_g.items() if not k.startswith("conv_"))
        print(f"  elementwise passes (prep excluded): {other_p:.3f} ms (a), {other_g:.3f} ms (b)")
        print(f"  layers whose planar launch is slower than the gather launch (+ its ReLU pass): {slower or 'none'}")


def vae_mode(a, pkg, losses):
    sd = he_state_dict(1234, upto=30)
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=1.0)
    load_formula(vae, 76)
    vae.train().to(DEV)
    m = losses.VGGPerceptualLoss(weights=sd).to(DEV)
    r = Restatement(sd, rate=0.2, dtype=torch.float32, device=DEV)
    for depth in (48, 8):
        x = formula_input((1, 1, depth, 192, 192), 45).clamp(-1, 1).to(DEV)

        def step(term):
            def fn():
                recon, _ = vae(x)
                loss = F.mse_loss(recon, x)
                if term is not None:
                    loss = loss + 0.1 * term(recon, x)
                loss.backward()
            return fn

        t = alternate([("a  MSE only", step(None)),
                       ("b  MSE + torch ops, bf16 autocast", step(lambda rc, y: r(rc, y, autocast=True))),
                       ("c  MSE + device perceptual loss", step(m))], a.rounds, a.warmup,
                      before=lambda: vae.zero_grad(set_to_none=True))
        print(f"[VAE base 128, latent 16, (1,1,{depth},192,192)] {a.rounds} alternated rounds after {a.warmup} warm-up")
        med = [show(k, v) for k, v in t.items()]
        print(f"  the term adds {med[2] - med[0]:.3f} ms per step on the device ({100 * (med[2] - med[0]) / med[0]:.1f} %), "
              f"{med[1] - med[0]:.3f} ms as torch ops ({100 * (med[1] - med[0]) / med[0]:.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loss", "vae"), default="loss")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vgg_bench.py measures on a ROCm device; none is available")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    losses = importlib.import_module("models.losses")
    print(f"device {torch.cuda.get_device_name(0)}; mode {a.mode}; HIP events, host launch included")
    if a.mode == "loss":
        loss_mode(a, losses)
    else:
        vae_mode(a, pkg, losses)


if __name__ == "__main__":
    main()
