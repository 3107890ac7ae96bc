"""What the image-space loss terms of the diffusion stage cost, at BASELINE config 3: B = 4, 8 -> 48 slices of
192 x 192, latent (4, 8, 48, 48, 48), the production model (264.66 M-parameter U-Net, base-128 VAE), random weights.

  --mode step     one training micro-step (model(v_in, v_gt) + backward), variants ALTERNATED in one process:
                    no term; MS-SSIM (CombinedLoss(0, 0.1, ssim_every_n_steps=1)) with 4 / 2 / 1 rows passing the SNR gate
                    (t is injected: 100 passes, 900 does not); the same with ssim_every_n_steps=10 (mean over the rounds: one
                    step in ten carries the term).
  --mode decode   decode_with_grad alone at (1, 8, 48, 48, 48): its forward against engine.VAEDecodeProgram, its backward
                    against VAETrainProgram's backward at the same shape.  That backward is a strict subset of the VAE
                    backward's launches (no encoder, no weight gradients); the per-launch table of both says where the time is.
  --mode kernels  ctsi_z0_pred and ctsi_loss_bwd_z0 beside ctsi_mse_loss_bwd on the same (4, 8, 48, 48, 48) buffers: us, TB/s of
                    the algorithmic bytes (16 / 14 / 10 bytes per element).
  --mode default  the micro-step without the term only; `--root DIR` imports the package from another checkout (a build of the
                    parent commit), so that parent / this / parent runs of this mode bracket the default path.

    python tools/image_loss_bench.py --mode step >> profiles/image_loss_bench.log"""
import argparse
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402

DEV = "cuda:0"
T_IN, T_OUT = 100, 900        # cosine schedule: SNR 33 and 0.02


def _root(argv):
    for i, a in enumerate(argv):
        if a == "--root" and i + 1 < len(argv):
            return os.path.abspath(argv[i + 1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ROOT = _root(sys.argv)
sys.path.insert(0, ROOT)
from tests.helpers import FULL_CFG, formula_input     # noqa: E402


def alternate(variants, rounds, warmup):
    """variants: [(name, fn)] -> {name: times in ms, in round order}"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in variants]
    times = {name: [] for name, _ in variants}
    for rnd in range(warmup + rounds):
        for i, (_, fn) in enumerate(variants):
            ev[i][0].record()
            fn()
            ev[i][1].record()
        torch.cuda.synchronize()
        if rnd >= warmup:
            for i, (name, _) in enumerate(variants):
                times[name].append(ev[i][0].elapsed_time(ev[i][1]))
    return times


def show(name, ts, extra=""):
    s = sorted(ts)
    print(f"  ({name:44s}) median {s[len(s) // 2]:9.3f} ms   mean {sum(s) / len(s):9.3f}   min {s[0]:9.3f}  max {s[-1]:9.3f}   {extra}")
    return s[len(s) // 2]


def _model(pkg):
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).to(DEV)
    model.train()
    return model


def _batch():
    v_in = formula_input((4, 1, 8, 192, 192), 18).clamp(-1, 1).to(DEV)
    v_gt = formula_input((4, 1, 48, 192, 192), 19).clamp(-1, 1).to(DEV)
    noise = torch.randn((4, 8, 48, 48, 48), generator=torch.Generator().manual_seed(3)).to(DEV)
    return v_in, v_gt, noise


def _step(model, v_in, v_gt, noise, t, fn):
    def run():
        model.image_loss = fn
        for p in model.unet.parameters():
            p.grad = None
        total, _ = model(v_in, v_gt, t=t, noise=noise)
        total.backward()
    return run


def step_mode(a, pkg, losses):
    model = _model(pkg)
    v_in, v_gt, noise = _batch()
    t_of = lambda k: torch.tensor([T_IN] * k + [T_OUT] * (4 - k), device=DEV)
    every = lambda n: losses.CombinedLoss(lambda_perceptual=0.0, lambda_ssim=0.1, ssim_every_n_steps=n)
    variants = [("no term", _step(model, v_in, v_gt, noise, t_of(4), None))]
    for k in (4, 2, 1):
        variants.append((f"MS-SSIM every step, {k} active row(s)", _step(model, v_in, v_gt, noise, t_of(k), every(1))))
    variants.append(("MS-SSIM every 10th step, 4 active rows", _step(model, v_in, v_gt, noise, t_of(4), every(10))))
    times = alternate(variants, a.rounds, a.warmup)
    print(f"[micro-step, config 3: B = 4, latent (4,8,48,48,48), 192^2 patches] {a.rounds} alternated rounds after {a.warmup} warm-up; "
          f"forward + backward, both VAE encodes included")
    med = {k: show(k, v) for k, v in times.items()}
    base = med["no term"]
    for k in (4, 2, 1):
        d = med[f"MS-SSIM every step, {k} active row(s)"] - base
        print(f"  the term with {k} active row(s) adds {d:8.1f} ms = {100 * d / base:5.1f} % of the plain micro-step ({d / k:6.1f} ms per row)")
    ts = times["MS-SSIM every 10th step, 4 active rows"]
    print(f"  every 10th step: mean {sum(ts) / len(ts):.1f} ms over {len(ts)} consecutive steps = "
          f"{100 * (sum(ts) / len(ts) - base) / base:.1f} % over the plain micro-step (the term's step: max {max(ts):.1f} ms)")
    print(f"  peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def default_mode(a, pkg):
    model = _model(pkg)
    v_in, v_gt, noise = _batch()
    t = torch.tensor([T_IN] * 4, device=DEV)

    def run():
        for p in model.unet.parameters():
            p.grad = None
        total, _ = model(v_in, v_gt, t=t, noise=noise)
        total.backward()

    times = alternate([("micro-step without the term", run)], a.rounds, a.warmup)
    print(f"[default path, package from {os.path.relpath(ROOT)}] config-3 micro-step, {a.rounds} rounds after {a.warmup} warm-up")
    show("micro-step without the term", times["micro-step without the term"])


def _table(prog, lo, hi, repeats=3):
    with prog.ctx.scope():
        rows = prog.profile_ops(repeats=repeats)
    torch.cuda.synchronize()
    agg = {}
    for name, kernel, flops, ms in rows[lo:hi]:
        last = name.split(".")[-1]
        if "wgrad" in name:
            key = "weight gradients"
        elif last == "bgrad":
            key = "bias sums"
        elif kernel.startswith("conv_"):
            key = "conv data gradients" if last == "dgrad" else "conv " + last
        else:
            key = name
        cnt, tot = agg.get(key, (0, 0.0))
        agg[key] = (cnt + 1, tot + ms)
    return sorted(agg.items(), key=lambda kv: -kv[1][1]), sum(r[3] for r in rows[lo:hi])


def decode_mode(a, pkg):
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    torch.manual_seed(0)
    vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=128, scaling_factor=1.0).to(DEV)
    z = formula_input((1, 8, 48, 48, 48), 61).to(DEV)
    x = formula_input((1, 1, 48, 192, 192), 45).clamp(-1, 1).to(DEV)
    zg = z.clone().requires_grad_(True)
    box = {}

    def dec_plain():
        with torch.no_grad():
            vae._decode(z, "bf16")

    def dec_fwd():
        box["r"] = vae.decode_with_grad(zg)

    def dec_bwd():
        zg.grad = None
        box["r"].backward(box["g"])

    def vae_fwd():
        box["vr"], _ = vae(x)

    def vae_bwd():
        vae.zero_grad(set_to_none=True)
        box["vr"].backward(box["g"])

    dec_fwd()
    box["g"] = torch.ones_like(box["r"]) / box["r"].numel()
    times = alternate([("VAEDecodeProgram forward (no tape)", dec_plain), ("decode_with_grad forward", dec_fwd),
                       ("decode_with_grad backward", dec_bwd), ("VAETrainProgram forward (encode + decode)", vae_fwd),
                       ("VAETrainProgram backward (weight gradients)", vae_bwd)], a.rounds, a.warmup)
    print(f"[decode_with_grad, latent (1,8,48,48,48) -> (1,1,48,192,192), base-128 VAE] {a.rounds} alternated rounds after {a.warmup} warm-up")
    med = {k: show(k, v) for k, v in times.items()}
    b, vb = med["decode_with_grad backward"], med["VAETrainProgram backward (weight gradients)"]
    print(f"  data-gradient backward {b:.1f} ms against {vb:.1f} ms of the VAE training backward at the same shape: "
          f"{'LOWER' if b < vb else 'NOT lower'} ({100 * b / vb:.0f} %)")
    dprog = [p for k, p in vae.decoder.__dict__["_ctsi_programs"].items() if k[0] == "dec-grad"][0]
    tprog = [p for k, p in vae.__dict__["_ctsi_programs"].items() if k[0] == "train"][0]
    for tag, prog in (("decode_with_grad", dprog), ("VAETrainProgram", tprog)):
        rows, total = _table(prog, prog.n_fwd, len(prog.ops))
        print(f"  backward launches of {tag}, eager with HIP events around each (sum {total:.1f} ms, {len(prog.ops) - prog.n_fwd} launches):")
        for key, (cnt, ms) in rows[:8]:
            print(f"      {key:28s} x{cnt:<3d} {ms:9.3f} ms")
    print(f"  activation + gradient buffers of the decode tape: {dprog.pool.total_bytes / 2 ** 30:.1f} GiB")


def kernels_mode(a, pkg):
    lib = pkg.get_lib()
    n, c, d, h, w = 4, 8, 48, 48, 48
    numel = n * c * d * h * w
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    z0, noise, g_z0, pred = rnd(n, c, d, h, w), rnd(n, c, d, h, w), rnd(n, c, d, h, w), rnd(n, d, h, w, c)
    g = pkg.GaussianDiffusion("cosine", 1000)
    sa, s1 = g.sqrt_alphas_cumprod.to(DEV), g.sqrt_one_minus_alphas_cumprod.to(DEV)
    t = torch.tensor([100, 300, 500, 700], dtype=torch.int32, device=DEV)
    act = torch.ones(n, dtype=torch.int32, device=DEV)
    coef, norm, gs = -(s1 / sa)[t.long()].contiguous(), torch.full((n,), 1e-6, device=DEV), torch.ones(1, device=DEV)
    out, dp = torch.empty_like(z0), torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    variants = [
        ("ctsi_z0_pred (epsilon)", lambda: lib.z0_pred(p(z0), p(noise), p(pred), c, p(sa), p(s1), p(t), p(act), 0, n, c, d, h, w, p(out), sp)),
        ("ctsi_z0_pred (v)", lambda: lib.z0_pred(p(z0), p(noise), p(pred), c, p(sa), p(s1), p(t), p(act), 1, n, c, d, h, w, p(out), sp)),
        ("ctsi_loss_bwd_z0", lambda: lib.loss_bwd_z0(p(pred), p(noise), None, p(norm), p(gs), p(g_z0), p(act), p(coef), n, c, d, h, w, p(dp), c, sp)),
        ("ctsi_mse_loss_bwd", lambda: lib.mse_loss_bwd(p(pred), p(noise), None, p(norm), p(gs), n, c, d, h, w, p(dp), c, sp)),
    ]
    nbytes = {"ctsi_z0_pred (epsilon)": 16, "ctsi_z0_pred (v)": 16, "ctsi_loss_bwd_z0": 14, "ctsi_mse_loss_bwd": 10}
    times = alternate(variants, a.rounds, a.warmup)
    print(f"[kernels, (4,8,48,48,48) = {numel / 1e6:.2f} M elements] {a.rounds} alternated rounds after {a.warmup} warm-up; one launch per timing")
    for k, ts in times.items():
        s = sorted(ts)
        print(f"  ({k:26s}) min {1e3 * s[0]:8.1f} us  median {1e3 * s[len(s) // 2]:8.1f} us   {nbytes[k]} B/element = "
              f"{nbytes[k] * numel / 1e6:.0f} MB -> {nbytes[k] * numel / (s[0] * 1e-3) / 1e12:.2f} TB/s at the minimum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "decode", "kernels", "default"), default="step")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=None, help="import the package from this checkout instead of the tool's own")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_loss_bench.py measures on a ROCm device; none is available")
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    print(f"device {torch.cuda.get_device_name(0)}; mode {a.mode}; HIP events, host launch included")
    if a.mode == "step":
        step_mode(a, pkg, importlib.import_module("models.losses"))
    elif a.mode == "default":
        default_mode(a, pkg)
    elif a.mode == "decode":
        decode_mode(a, pkg)
    else:
        kernels_mode(a, pkg)


if __name__ == "__main__":
    main()
