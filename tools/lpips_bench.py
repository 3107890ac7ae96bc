"""What the device LPIPS distance (models.losses.LPIPS, vgg_loss_engine.py, csrc/lpips.hip) costs.  Everything is ALTERNATED
in one process; medians with their spread (min / max) over the rounds.

  --mode loss     forward + backward of LPIPS against the same arithmetic as torch ops under bf16 autocast
                  (tests/lpips_restatement.py) at (4, 3, 192, 192) -- the VAE trainer's middle slices at batch 4 -- and
                  (1, 3, 512, 512)
  --mode metric   utils.metrics.calculate_lpips on a 48 x 512 x 512 pair
  --mode kernels  ctsi_lpips_dist_fwd / ctsi_lpips_grad_relu_bwd alone on the largest tap tensor (tap 1 of (4, 3, 192, 192): 4
                  images x 36864 positions x 64 channels per half), next to ctsi_feat_loss_fwd / ctsi_feat_grad_relu_bwd on the
                  SAME buffers: bytes moved, TB/s and the time per byte relative to those passes
  --mode vae      one VAE training step (base 128, latent 16) at (1,1,48,192,192) and (1,1,8,192,192) with MSE only, MSE + 0.1 x
                  the torch restatement under autocast, MSE + 0.1 x LPIPS on the middle slice
  --mode vgg19    VGGPerceptualLoss forward + backward at the shapes of tools/vgg_bench.py (run it from two checkouts to
                  compare them; one process cannot load two libraries)
Weights are random (He-normal convs, non-negative heads): no trained weights ship with the project, so image quality is not
measured; the arithmetic does not depend on the values.

    python tools/lpips_bench.py --mode loss [--rounds 9] [--warmup 2] >> profiles/lpips_bench.log"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")     # (as tests/conftest.py: no exhaustive MIOpen search for the baseline)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import formula_input, load_formula                                 # noqa: E402
from tools.msssim_bench import alternate, show                                        # noqa: E402

DEV = "cuda:0"


def _weights():
    from tests.lpips_restatement import he_state_dict, random_heads
    return he_state_dict(1234), random_heads(77)


def _pair(shape, seed):
    from tests.lpips_restatement import make_pair
    return tuple(x.to(DEV) for x in make_pair(shape, seed))


def loss_mode(a, losses):
    from tests.lpips_restatement import Restatement
    sd, heads = _weights()
    m = losses.LPIPS(weights=sd, lin_weights=heads).to(DEV)
    r = Restatement(sd, heads, torch.float32, DEV)
    for shape in ((4, 3, 192, 192), (1, 3, 512, 512)):
        pred, target = _pair(shape, 7)
        p = pred.clone().requires_grad_(True)

        def hip_fb():
            p.grad = None
            m(p, target).mean().backward()

        def torch_fb():
            p.grad = None
            r(p, target, autocast=True).mean().backward()

        def hip_fwd():
            with torch.no_grad():
                m(pred, target)

        t = alternate([("a  engine, forward + backward", hip_fb), ("b  torch ops, bf16 autocast, f + b", torch_fb),
                       ("c  engine, forward only", hip_fwd)], a.rounds, a.warmup)
        prog = [q for v in m._ctsi_programs.values() for q in v if q.h == shape[2]][0]
        print(f"[{'x'.join(map(str, shape))}] {a.rounds} alternated rounds after {a.warmup} warm-up; conv work {prog.flops / 1e12:.2f} TFLOP")
        med = [show(k, v) for k, v in t.items()]
        print(f"  engine {med[1] / med[0]:.2f}x the torch run's speed")
        with prog.ctx.scope():
            rows = prog.profile_ops(repeats=5)
        torch.cuda.synchronize()
        for name, kernel, _, ms in rows:
            if kernel.startswith("lpips"):
                nbytes = prog.op_bytes[[n for n, _, _ in prog.op_meta].index(name)]
                print(f"  {name:22s} {kernel:22s} {ms:8.4f} ms" + (f"  {nbytes / (ms * 1e-3) / 1e12:6.2f} TB/s" if nbytes else ""))
        print(f"  all passes but the convs: {sum(ms for _, k, _, ms in rows if not k.startswith('conv_')):.3f} ms of "
              f"{sum(ms for _, _, _, ms in rows):.3f} ms")


def metric_mode(a, losses):
    metrics = importlib.import_module("utils.metrics")
    sd, heads = _weights()
    m = losses.LPIPS(weights=sd, lin_weights=heads).to(DEV)
    g = torch.Generator().manual_seed(5)
    v2 = torch.rand(1, 1, 48, 512, 512, generator=g)
    v1 = (v2 + 0.1 * torch.randn(v2.shape, generator=g)).clamp(0, 1).to(DEV)
    v2 = v2.to(DEV)
    res = {}

    def run():
        res.update(metrics.calculate_lpips(v1, v2, m))

    t = alternate([("calculate_lpips, 48 x 512 x 512", run)], a.rounds, a.warmup)
    print(f"[calculate_lpips] 48 slices in groups of 8; {a.rounds} rounds after {a.warmup} warm-up; "
          f"value {res['lpips']:.4f} (random weights)")
    med = show("calculate_lpips, 48 x 512 x 512", t["calculate_lpips, 48 x 512 x 512"])
    print(f"  {med / 48:.3f} ms per slice; device memory in use {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB at the peak")


def kernels_mode(a, pkg):
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    ctx = E.Ctx.get(torch.device(DEV))
    lib = ctx.lib
    n, pos, c = 4, 192 * 192, 64
    half = n * pos * c
    g = torch.Generator().manual_seed(3)
    feats = torch.relu(torch.randn(2 * half, generator=g)).to(device=DEV, dtype=torch.bfloat16)
    gin = (torch.randn(half, generator=g) * 1e-3).to(device=DEV, dtype=torch.bfloat16)
    gout = torch.empty_like(gin)
    w = (torch.rand(c, generator=g) * (64.0 / c)).to(DEV)
    go = torch.full((n,), 0.25, device=DEV)
    gl = torch.ones(1, device=DEV)
    part_l = torch.empty(n * lib.lpips_blocks(), dtype=torch.float64, device=DEV)
    part_f = torch.empty(lib.feat_loss_blocks(), dtype=torch.float64, device=DEV)
    yp, tp = C.c_void_p(feats.data_ptr()), C.c_void_p(feats.data_ptr() + 2 * half)
    P = lambda t: C.c_void_p(t.data_ptr())                                                    # noqa: E731
    s = ctx.sptr

    def scoped(fn):
        def run():
            with ctx.scope():
                fn()
        return run

    variants = [("lpips_dist_fwd", scoped(lambda: lib.lpips_dist_fwd(yp, tp, P(w), n, pos, c, P(part_l), s)), 4.0 * half),
                ("feat_loss_fwd (L1)", scoped(lambda: lib.feat_loss_fwd(yp, tp, half, 0, P(part_f), s)), 4.0 * half),
                ("lpips_grad_relu_bwd", scoped(lambda: lib.lpips_grad_relu_bwd(P(gin), yp, tp, P(w), P(gout), n, pos, c, P(go), s)), 8.0 * half),
                ("feat_grad_relu_bwd (L1)", scoped(lambda: lib.feat_grad_relu_bwd(P(gin), yp, tp, P(gout), half, 1e-6, 1, 1, P(gl), s)), 8.0 * half)]
    t = alternate([(k, f) for k, f, _ in variants], a.rounds, a.warmup)
    print(f"[kernels] tap 1 of (4, 3, 192, 192): {n} images x {pos} positions x {c} channels per half ({2 * half / 2 ** 20:.0f} MiB "
          f"each); {a.rounds} alternated rounds after {a.warmup} warm-up; HIP events, host launch included")
    med = {}
    for k, _, nbytes in variants:
        ts = t[k]
        med[k] = ts[len(ts) // 2]
        show(k, ts, f"{nbytes / 2 ** 20:.0f} MiB moved, {nbytes / (med[k] * 1e-3) / 1e12:.2f} TB/s")
    print(f"  time per byte: lpips_dist_fwd {med['lpips_dist_fwd'] / med['feat_loss_fwd (L1)']:.2f}x ctsi_feat_loss_fwd's, "
          f"lpips_grad_relu_bwd {med['lpips_grad_relu_bwd'] / med['feat_grad_relu_bwd (L1)']:.2f}x ctsi_feat_grad_relu_bwd's "
          f"(the same buffers, the same byte counts)")


def vae_mode(a, pkg, losses):
    from tests.lpips_restatement import Restatement, volume_loss
    sd, heads = _weights()
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=1.0)
    load_formula(vae, 76)
    vae.train().to(DEV)
    m = losses.LPIPS(weights=sd, lin_weights=heads).to(DEV)
    r = Restatement(sd, heads, torch.float32, DEV)
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
                       ("b  MSE + torch ops, bf16 autocast", step(lambda rc, y: volume_loss(r, rc.float(), y, [depth // 2], autocast=True))),
                       ("c  MSE + device LPIPS", step(m))], a.rounds, a.warmup,
                      before=lambda: vae.zero_grad(set_to_none=True))
        print(f"[VAE base 128, latent 16, (1,1,{depth},192,192), middle slice] {a.rounds} alternated rounds after {a.warmup} warm-up")
        med = [show(k, v) for k, v in t.items()]
        print(f"  the term adds {med[2] - med[0]:.3f} ms per step on the device ({100 * (med[2] - med[0]) / med[0]:.1f} %), "
              f"{med[1] - med[0]:.3f} ms as torch ops ({100 * (med[1] - med[0]) / med[0]:.1f} %)")


def vgg19_mode(a, losses):
    from tests.vgg_restatement import he_state_dict, smooth_volume
    m = losses.VGGPerceptualLoss(weights=he_state_dict(1234, upto=30)).to(DEV)
    for shape in ((4, 1, 48, 192, 192), (1, 1, 48, 512, 512)):
        pred, target = smooth_volume(shape, 7).to(DEV), smooth_volume(shape, 8).to(DEV)
        p = pred.clone().requires_grad_(True)

        def fb():
            p.grad = None
            m(p, target).backward()

        t = alternate([("VGGPerceptualLoss, forward + backward", fb)], a.rounds, a.warmup)
        print(f"[vgg19 {'x'.join(map(str, shape))}] {a.rounds} rounds after {a.warmup} warm-up; loss {float(m(pred, target)):.6f}")
        show("VGGPerceptualLoss, f + b", t["VGGPerceptualLoss, forward + backward"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("loss", "metric", "kernels", "vae", "vgg19"), default="loss")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench.py measures on a ROCm device; none is available")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    losses = importlib.import_module("models.losses")
    print(f"device {torch.cuda.get_device_name(0)}; mode {a.mode}; HIP events, host launch included")
    {"loss": lambda: loss_mode(a, losses), "metric": lambda: metric_mode(a, losses), "kernels": lambda: kernels_mode(a, pkg),
     "vae": lambda: vae_mode(a, pkg, losses), "vgg19": lambda: vgg19_mode(a, losses)}[a.mode]()


if __name__ == "__main__":
    main()
