"""GPU: classifier-free guidance on the sampler step graph (csrc/guidance.hip, engine.UNetProgram(guided=True),
sampler.run_sampler(guidance_scale=, guidance_rescale=)) and conditioning dropout in the training forward.

 4. ctsi_cfg_combine / _stats / _mirror against the float64 restatement (tests/cfg_restatement.py);
 5. guided sampling of an analytic model whose eps is affine in the conditioning == unguided sampling on s c;
 6. the engine U-Net per evaluation: the batch-2n program against two runs of the existing batch-n program;
 7. guidance_scale = 1.0 is the unguided path, bit for bit, and builds no guided program;
 8. guidance_scale = 0 == unguided sampling on the zero conditioning;
 9. captured replay == eager; repeated calls; a change of scale reuses the captured graph;
10. a batch of two == two single runs; guided stitching == window by window;
11. generate() at config 1 (one VAE encode); the depth-sharded refusal;
12. conditioning dropout: the mask, the generator, eval mode.
Every measured figure is printed before it is asserted (profiles/cfg_tests.log is that output)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from tests import cfg_restatement as CR
from tests.helpers import TINY_UNET, formula_input, load_formula, rel_l2, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
U24 = 2.0 ** -24
MU, SD, K = 0.5, 1.0, 0.3          # the analytic data model: x0 ~ N(MU + K c, SD^2) per element


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _t_desc(g, n):
    return [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n)]


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


@pytest.fixture(scope="module")
def tiny_unet(pkg):
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    return un.to(DEV)


@pytest.fixture(scope="module")
def full_model(pkg):
    torch.manual_seed(0)
    return pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)


class _precision:
    def __init__(self, unet, p):
        self.unet, self.p = unet, p

    def __enter__(self):
        self.prev = self.unet.inference_precision
        self.unet.inference_precision = self.p

    def __exit__(self, *exc):
        self.unet.inference_precision = self.prev


# ---------------------------------------------------------------------------------------------------------------------
# 4. the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
def _branches(shape, variant, seed):
    """(eps_c, eps_u) as fp32 (n, d, h, w, L) tensors: independent draws, or nearly cancelling branches."""
    n, Lc, d, h, w = shape
    c = _randn((n, d, h, w, Lc), seed)
    if variant == "random":
        u = 0.3 + 0.8 * _randn((n, d, h, w, Lc), seed + 1)
    else:
        u = c * (1.0 + 1e-3 * _randn((n, d, h, w, Lc), seed + 1))
    return c, u


def _device_cfg(lib, ctx, c, u, s, phi, shape):
    """ctsi_cfg_(stats, stats_finalize,) combine on the device; returns (eps rows [0, n), the untouched rows [n, 2n),
    stats or None)."""
    n, Lc, d, h, w = shape
    eps = torch.cat([c, u]).to(DEV).contiguous()
    scale = torch.tensor([[7.0, 0.0], [s, phi]], dtype=torch.float32, device=DEV)     # row 1 is the one in use
    step = torch.ones(1, dtype=torch.int32, device=DEV)
    stats = None
    with ctx.scope():
        if phi > 0:
            part = torch.zeros(n * lib.cfg_stats_blocks(Lc * d * h * w) * 4, dtype=torch.float64, device=DEV)
            stats = torch.zeros((n, 4), dtype=torch.float64, device=DEV)
            lib.cfg_stats(_ptr(eps), _ptr(scale), _ptr(step), _ptr(part), n, Lc, d, h, w, ctx.sptr)
            lib.cfg_stats_finalize(_ptr(part), _ptr(stats), n, Lc, d, h, w, ctx.sptr)
        lib.cfg_combine(_ptr(eps), _ptr(scale), _ptr(step), _ptr(stats), n, Lc, d, h, w, ctx.sptr)
    torch.cuda.synchronize()
    return eps[:n].cpu(), eps[n:].cpu(), None if stats is None else stats.cpu()


@pytest.mark.parametrize("variant", ["random", "cancelling"])
@pytest.mark.parametrize("s", [0.0, 0.5, 1.5, 7.5, -1.0])
@pytest.mark.parametrize("shape", [(2, 8, 4, 8, 8), (1, 3, 5, 7, 9)])      # the second: no 16-byte path
def test_combine_against_float64(shape, s, variant):
    """|got - ref| <= 4 * 2^-24 * (|s| (|eps_c| + |eps_u|) + |eps_u|) elementwise: eps_c - eps_u, the product with s and
    the sum with eps_u are at most three fp32 roundings, each relative to a term of that magnitude."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    c, u = _branches(shape, variant, 100)
    got, tail, _ = _device_cfg(lib, ctx, c, u, s, 0.0, shape)
    ref = CR.cfg_eps(c, u, s, 0.0)
    mag = CR.magnitude(c, u, s)
    used = float(((got.double() - ref).abs() / (4 * U24 * mag).clamp_min(1e-300)).max())
    print(f"combine {shape} s={s} {variant}: worst |err| / bound = {used:.3f}")
    assert torch.equal(tail, u)                                   # rows [n, 2n) are read only
    assert ((got.double() - ref).abs() <= 4 * U24 * mag).all(), used
    if s == 0.0:
        assert torch.equal(got, u)


@pytest.mark.parametrize("variant", ["random", "cancelling"])
@pytest.mark.parametrize("phi", [0.3, 1.0])
@pytest.mark.parametrize("s", [0.0, 0.5, 1.5, 7.5, -1.0])
@pytest.mark.parametrize("shape", [(2, 8, 4, 8, 8), (1, 3, 5, 7, 9)])
def test_rescale_against_float64(shape, s, phi, variant):
    """Both standard deviations within 1e-6 relative of torch.std in float64; the result within 8 * 2^-24 of the
    magnitude term times the factor that multiplies eps_g, m = phi std(eps_c) / std(eps_g) + 1 - phi (the std ratio itself
    at phi = 1): eps_g carries the three roundings above, m one, their product one more.  Two runs: the same bits."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    c, u = _branches(shape, variant, 200)
    got, _, stats = _device_cfg(lib, ctx, c, u, s, phi, shape)
    got2, _, stats2 = _device_cfg(lib, ctx, c, u, s, phi, shape)
    g64 = CR.guide(c, u, s)
    sc, sg = CR.std_b(c), CR.std_b(g64)
    e_c = float(((stats[:, 0] - sc).abs() / sc).max())
    e_g = float(((stats[:, 1] - sg).abs() / sg).max())
    m = (phi * CR.rescale_factor(c, g64) + (1.0 - phi)).reshape(-1, 1, 1, 1, 1)
    ref = CR.cfg_eps(c, u, s, phi)
    bound = 8 * U24 * CR.magnitude(c, u, s) * m
    used = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"rescale {shape} s={s} phi={phi} {variant}: std rel err {e_c:.2e} / {e_g:.2e}, worst |err| / bound = {used:.3f}")
    assert e_c <= 1e-6 and e_g <= 1e-6
    assert float((stats[:, 3] - c[0].numel()).abs().max()) == 0.0
    assert ((got.double() - ref).abs() <= bound).all(), used
    assert torch.equal(got, got2) and torch.equal(stats, stats2)


def test_rescale_of_a_constant_guided_eps_has_factor_one():
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    shape = (2, 8, 4, 8, 8)
    c, u = _branches(shape, "random", 300)
    u[0] = 0.25                          # s = 0: eps_g = eps_u, constant in sample 0
    got, _, stats = _device_cfg(lib, ctx, c, u, 0.0, 1.0, shape)
    assert float(stats[0, 1]) == 0.0 and float(stats[0, 2]) == 1.0
    assert torch.equal(got[0], u[0]) and torch.isfinite(got).all()


@pytest.mark.parametrize("Lc,dtype", [(8, torch.bfloat16), (3, torch.bfloat16), (8, torch.float32), (3, torch.float32),
                                      (2, torch.float32)])
def test_mirror_copies_the_z_half_only(Lc, dtype):
    """rows [0, n) of the z slice -> rows [n, 2n); the conditioning half of a [z | cond] tensor is not touched."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, vox = 2, 4 * 7 * 9
    c_total = 2 * Lc if dtype == torch.bfloat16 else Lc
    x = _randn((2 * n * vox, c_total), 400).to(dtype).to(DEV)
    before = x.clone()
    nbytes = x.element_size()
    with ctx.scope():
        lib.cfg_mirror(_ptr(x), C.c_void_p(x.data_ptr() + n * vox * c_total * nbytes), n * vox, Lc * nbytes,
                       c_total * nbytes, ctx.sptr)
    torch.cuda.synchronize()
    assert torch.equal(x[:n * vox], before[:n * vox])
    assert torch.equal(x[n * vox:, :Lc], before[:n * vox, :Lc])
    assert torch.equal(x[n * vox:, Lc:], before[n * vox:, Lc:])


# ---------------------------------------------------------------------------------------------------------------------
# 5. exact identity on an analytic model through the generic path
# ---------------------------------------------------------------------------------------------------------------------
def _analytic_vp(g):
    """eps*(z, t, c) = sigma (z - alpha (MU + K c)) / (alpha^2 SD^2 + sigma^2): affine in c.  float64 inside."""
    ac = g.alphas_cumprod.double().to(DEV)

    def model(z, t, c):
        ab = ac[t].view(-1, 1, 1, 1, 1)
        a, s = ab.sqrt(), (1 - ab).sqrt()
        return (s * (z.double() - a * (MU + K * c.double())) / (a * a * SD * SD + s * s)).float()
    return model


def _analytic_edm(g):
    """The same data model at the noise level of the (fractional) timestep, as tests/test_gpu_heun_sampler.py writes it."""
    ls = torch.from_numpy(np.log(S.sigma_table(g.alphas_cumprod))).to(DEV)

    def model(z, t, c):
        t = t.double().clamp(0, len(ls) - 1)
        k = t.floor().long().clamp(max=len(ls) - 2)
        s = torch.exp(ls[k] + (t - k) * (ls[k + 1] - ls[k])).view(-1, 1, 1, 1, 1)
        a = (1 + s * s).sqrt()
        return (s * (a * z.double() - (MU + K * c.double())) / (SD * SD + s * s)).float()
    return model


def _restated_unguided(g, kind, z_t, cond, n, noises=None, rows_heun=None):
    """Unguided sampling of the analytic model on conditioning `cond`, float64 (the fp32 rows widened)."""
    ac = g.alphas_cumprod.double()
    mean = MU + K * cond.double()
    z = z_t.double().clone()
    if kind == "heun":
        r = rows_heun
        rows = r.rows.double()
        z = r.init[0] * z
        d1, zin = torch.zeros_like(z), z.clone()
        for e in range(rows.shape[0]):
            s = float(r.sigma_eval[e])
            eps = s * (np.sqrt(1 + s * s) * zin - mean) / (SD * SD + s * s)
            c = rows[e]
            dd = (c[0] * z + c[1] * d1 - c[2] * eps).clamp(-10, 10)
            if c[3] == 0:
                d1, zin = dd, c[4] * z + c[5] * dd
            else:
                z = c[4] * z + c[5] * dd + c[6] * d1
                zin = z
        return z
    t_desc = list(reversed(range(g.timesteps)))[:n] if kind == "ddpm" else _t_desc(g, n)
    if kind == "dpmpp":
        rows, xp = S.dpm_coef_rows(g.alphas_cumprod, t_desc, 2).double(), torch.zeros_like(z)
    elif kind == "ddim":
        rows = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).double()
    else:
        rows = g.ddpm_coef_rows(t_desc).double().cpu()
    for i, t in enumerate(t_desc):
        a, sg = ac[t].sqrt(), (1 - ac[t]).sqrt()
        e = sg * (z - a * mean) / (a * a * SD * SD + sg * sg)
        if kind == "dpmpp":
            x0 = (rows[i, 0] * z - rows[i, 1] * e).clamp(-10, 10)
            z = rows[i, 2] * z + rows[i, 3] * x0 + rows[i, 4] * xp
            xp = x0
        elif kind == "ddim":
            x0 = ((z - rows[i, 0] * e) / rows[i, 1]).clamp(-10, 10)
            z = rows[i, 2] * x0 + rows[i, 3] * e
        else:
            x0 = ((z - rows[i, 0] * e) / rows[i, 1]).clamp(-1, 1)
            z = rows[i, 2] * x0 + rows[i, 3] * z + rows[i, 4] * noises[i].double()
    return z


@pytest.mark.parametrize("s", [0.0, 2.5])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp", "heun", "ddpm"])
def test_guided_analytic_model_equals_unguided_on_scaled_conditioning(pkg, kind, s):
    """eps* is affine in c, so eps_u + s (eps_c - eps_u) is eps* on the conditioning s c, whatever update follows."""
    g = pkg.GaussianDiffusion()
    shape, n = (2, 4, 4, 16, 16), 10
    z_t, cond = _randn(shape, 1), formula_input(shape, 2)
    kw = dict(guidance_scale=s, progress=False)
    if kind == "ddim":
        out = pkg.DDIMSampler(g, _analytic_vp(g)).sample(shape, cond.to(DEV), n, DEV, z_init=z_t.to(DEV), **kw)
        ref = _restated_unguided(g, kind, z_t, s * cond, n)
    elif kind == "dpmpp":
        out = pkg.DPMSolverSampler(g, _analytic_vp(g)).sample(shape, cond.to(DEV), n, DEV, z_init=z_t.to(DEV), **kw)
        ref = _restated_unguided(g, kind, z_t, s * cond, n)
    elif kind == "heun":
        sp = pkg.HeunSampler(g, _analytic_edm(g))
        out = sp.sample(shape, cond.to(DEV), n, DEV, z_init=z_t.to(DEV), **kw)
        ref = _restated_unguided(g, kind, z_t, s * cond, n, rows_heun=sp.coef_rows(n))
    else:
        n = 40
        noises = {i: _randn(shape, 500 + i) for i in range(-1, n)}
        out = pkg.DDPMSampler(g, _analytic_vp(g)).sample(shape, cond.to(DEV), DEV, num_steps=n,
                                                          noise_fn=lambda i, shp: noises[i].to(DEV), **kw)
        ref = _restated_unguided(g, kind, noises[-1], s * cond, n, noises=noises)
    err = rel_l2(out.cpu(), ref)
    print(f"analytic {kind} s={s}: guided(s, c) vs float64 unguided(s c) rel-L2 {err:.3e}")
    assert torch.isfinite(out).all()
    assert err < 2e-3, err


# ---------------------------------------------------------------------------------------------------------------------
# 6. the engine U-Net, per evaluation
# ---------------------------------------------------------------------------------------------------------------------
def _ddim_update(rows, i, z, e):
    x0 = ((z - rows[i, 0] * e) / rows[i, 1]).clamp(-10, 10)
    return rows[i, 2] * x0 + rows[i, 3] * e


def _per_evaluation(g, unet, shape, s, precision, seed, phi=0.0):
    """5 DDIM steps of the guided program.  For every evaluation: the guided eps against the float64 combination of two
    runs of the EXISTING unguided program (unet(z, t, c): batch n) on the recorded input state, then the update."""
    cond = formula_input(shape, seed).to(DEV)
    zeros = torch.zeros_like(cond)
    z_t = _randn(shape, seed + 1)
    t_desc = _t_desc(g, 5)
    traj, eps = [], []
    with _precision(unet, precision):
        out = S.run_sampler(g, unet, shape, cond, DEV, kind="ddim", t_desc=t_desc, progress=False, z_init=z_t.to(DEV),
                            trajectory=traj, eps_trajectory=eps, guidance_scale=s, guidance_rescale=phi)
    assert len(traj) == len(eps) == len(t_desc) and torch.equal(traj[-1], out)
    rows = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).double()
    zs = [z_t] + [t.cpu() for t in traj]
    n = shape[0]
    worst_ratio = 0.0
    for i, t in enumerate(t_desc):
        zi = zs[i].to(DEV)
        tt = torch.full((n,), t, device=DEV, dtype=torch.long)
        with _precision(unet, "fp32"):
            c32, u32 = unet(zi, tt, cond).cpu(), unet(zi, tt, zeros).cpu()
        ref = CR.cfg_eps(c32, u32, s, phi)
        got = eps[i].cpu().double()
        assert torch.isfinite(got).all()
        dist = float((got - ref).norm())
        if precision == "fp32":
            bound = 1e-5 * (abs(s) * float(c32.double().norm()) + abs(1 - s) * float(u32.double().norm()))
            print(f"fp32 {tuple(shape)} s={s} phi={phi} eval {i}: ||got - ref|| {dist:.3e}, bound {bound:.3e} "
                  f"(ratio {dist / bound:.3f})")
        else:
            with _precision(unet, "bf16"):
                c16, u16 = unet(zi, tt, cond).cpu(), unet(zi, tt, zeros).cpu()
            d_c, d_u = float((c16.double() - c32.double()).norm()), float((u16.double() - u32.double()).norm())
            bracket = abs(s) * d_c + abs(1 - s) * d_u
            bound = 1.25 * bracket
            print(f"bf16 {tuple(shape)} s={s} phi={phi} eval {i}: ||got - ref|| {dist:.3e}, D_c {d_c:.3e}, D_u {d_u:.3e}, "
                  f"ratio to |s| D_c + |1 - s| D_u {dist / bracket:.3f}")
        worst_ratio = max(worst_ratio, dist / bound)
        assert dist <= bound, (precision, i, dist, bound)
        err = rel_l2(zs[i + 1], _ddim_update(rows, i, zs[i].double(), got))
        assert err < 1e-4, f"{precision} update {i}: {err:.3g}"
    print(f"{precision} {tuple(shape)} s={s} phi={phi}: worst distance / bound {worst_ratio:.3f}")


@pytest.mark.parametrize("s", [3.0, 0.5, -1.0])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_per_evaluation_tiny(pkg, tiny_unet, precision, s):
    _per_evaluation(pkg.GaussianDiffusion(), tiny_unet, (1, 8, 4, 8, 8), s, precision, 20)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_per_evaluation_config1(pkg, full_model, precision):
    _per_evaluation(full_model.diffusion, full_model.unet, (1, 8, 48, 48, 48), 3.0, precision, 30)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["dpmpp", "heun"])
def test_update_parity_other_samplers(pkg, tiny_unet, kind, precision):
    """The unchanged update, fed the recorded guided eps, against its float64 restatement: < 1e-4 per step."""
    from tests.test_gpu_heun_sampler import _replay_rows
    g = pkg.GaussianDiffusion()
    shape, n = (1, 8, 4, 8, 8), 5
    cond, z_t = formula_input(shape, 60).to(DEV), _randn(shape, 61)
    traj, eps = [], []
    with _precision(tiny_unet, precision):
        if kind == "dpmpp":
            t_desc = _t_desc(g, n)
            S.run_sampler(g, tiny_unet, shape, cond, DEV, kind="dpmpp", t_desc=t_desc, progress=False,
                          z_init=z_t.to(DEV), trajectory=traj, eps_trajectory=eps, guidance_scale=3.0)
        else:
            sp = S.HeunSampler(g, tiny_unet)
            r = sp.coef_rows(n)
            S.run_sampler(g, tiny_unet, shape, cond, DEV, kind="heun", t_desc=list(r.t), progress=False,
                          z_init=z_t.to(DEV), trajectory=traj, eps_trajectory=eps, order=sp.order, heun=r,
                          guidance_scale=3.0)
    worst = 0.0
    if kind == "dpmpp":
        rows = S.dpm_coef_rows(g.alphas_cumprod, t_desc, 2).double()
        zs = [z_t.double()] + [t.cpu().double() for t in traj]
        xp = torch.zeros_like(zs[0])
        for i in range(len(t_desc)):
            e = eps[i].cpu().double()
            x0 = (rows[i, 0] * zs[i] - rows[i, 1] * e).clamp(-10, 10)
            worst = max(worst, rel_l2(zs[i + 1], rows[i, 2] * zs[i] + rows[i, 3] * x0 + rows[i, 4] * xp))
            xp = x0
    else:
        assert len(eps) == r.rows.shape[0] and len(traj) == n
        states = [r.init[0] * z_t.double()] + [t.cpu().double() for t in traj]
        e0 = 0
        for i in range(n):
            k = 2 if i < n - 1 else 1
            sub = S.HeunRows(r.rows[e0:e0 + k], r.t[e0:e0 + k], r.sigma_eval[e0:e0 + k], r.sigmas, r.sigma_hat, r.gammas,
                             r.noise_step[e0:e0 + k], r.closes[e0:e0 + k], r.init)
            (zn,) = _replay_rows(sub, states[i], [x.cpu() for x in eps[e0:e0 + k]], {})
            worst = max(worst, rel_l2(states[i + 1], zn))
            e0 += k
    print(f"{kind} {precision}: worst per-step rel-L2 of the update on the guided eps {worst:.2e}")
    assert worst < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 7. guidance_scale = 1.0 is today's path
# ---------------------------------------------------------------------------------------------------------------------
def _keys(unet):
    return list(getattr(unet, "_ctsi_programs", {}).keys())


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpmpp", "heun"])
def test_scale_one_is_bit_identical_and_builds_no_guided_program(pkg, tiny_unet, kind):
    g = pkg.GaussianDiffusion()
    shape = (1, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 70).to(DEV), _randn(shape, 71).to(DEV)
    nf = lambda i, shp: (z_t if i < 0 else _randn(shp, 800 + i).to(DEV))
    call = {"ddim": lambda **kw: pkg.DDIMSampler(g, tiny_unet).sample(shape, cond, 4, DEV, progress=False, z_init=z_t, **kw),
            "ddpm": lambda **kw: pkg.DDPMSampler(g, tiny_unet).sample(shape, cond, DEV, progress=False, noise_fn=nf,
                                                                      num_steps=4, **kw),
            "dpmpp": lambda **kw: pkg.DPMSolverSampler(g, tiny_unet).sample(shape, cond, 4, DEV, progress=False,
                                                                            z_init=z_t, **kw),
            "heun": lambda **kw: pkg.HeunSampler(g, tiny_unet).sample(shape, cond, 4, DEV, progress=False, z_init=z_t,
                                                                      **kw)}[kind]
    E.invalidate_engine_cache(tiny_unet)
    plain = call()
    keys = _keys(tiny_unet)
    same = call(guidance_scale=1.0)
    also = call(guidance_scale=1.0, guidance_rescale=0.7)      # s = 1: eps_g = eps_c, nothing to rescale
    assert torch.equal(plain, same) and torch.equal(plain, also)
    assert _keys(tiny_unet) == keys and not any(k[0] == "sampler-cfg" for k in keys)
    guided = call(guidance_scale=3.0)
    assert any(k[0] == "sampler-cfg" for k in _keys(tiny_unet))
    assert [k for k in _keys(tiny_unet) if k[0] != "sampler-cfg"] == keys     # unguided keys unchanged
    assert torch.isfinite(guided).all() and not torch.equal(guided, plain)


def test_generate_scale_one_is_bit_identical(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    nf = lambda i, shp: _randn(shp, 900 + i).to(DEV)
    plain = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    keys = _keys(model.unet)
    same = model.generate(v_in, "ddim", 3, 1.0, 4, nf)
    assert torch.equal(plain, same) and _keys(model.unet) == keys
    guided = model.generate(v_in, "ddim", 3, guidance_scale=3.0, target_depth=4, noise_fn=nf)
    assert tuple(guided.shape) == tuple(plain.shape) and torch.isfinite(guided).all()
    assert not torch.equal(guided, plain)


# ---------------------------------------------------------------------------------------------------------------------
# 8. s = 0 is unconditional sampling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpmpp"])
def test_scale_zero_equals_unguided_on_zero_conditioning(pkg, tiny_unet, kind):
    g = pkg.GaussianDiffusion()
    shape = (1, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 80).to(DEV), _randn(shape, 81).to(DEV)
    cls = pkg.DDIMSampler if kind == "ddim" else pkg.DPMSolverSampler
    with _precision(tiny_unet, "fp32"):
        sp = cls(g, tiny_unet)
        a = sp.sample(shape, cond, 5, DEV, progress=False, z_init=z_t, guidance_scale=0.0)
        b = sp.sample(shape, torch.zeros_like(cond), 5, DEV, progress=False, z_init=z_t)
    err = rel_l2(a.cpu(), b.cpu())
    print(f"{kind} fp32: guided s = 0 vs unguided on zeros rel-L2 {err:.3e}")
    assert err < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 9. captured == eager, repeats, one graph for every scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_captured_equals_eager_and_repeats(pkg, tiny_unet, precision, phi):
    g = pkg.GaussianDiffusion()
    shape, n_steps, s = (1, 8, 4, 8, 8), 5, 3.0
    cond, z_t = formula_input(shape, 41).to(DEV), _randn(shape, 43).to(DEV)
    t_desc = _t_desc(g, n_steps)
    with _precision(tiny_unet, precision):
        sp = pkg.DDIMSampler(g, tiny_unet)
        runs = [sp.sample(shape, cond, n_steps, DEV, progress=False, z_init=z_t, guidance_scale=s,
                          guidance_rescale=phi) for _ in range(3)]
        ctx = E.Ctx.get(torch.device(DEV))
        with ctx.scope():       # the same step eagerly: a separately built program, launch by launch (no graph)
            cls = E32.UNetProgramF32 if precision == "fp32" else E.UNetProgram
            prog = cls(ctx, tiny_unet, 1, 4, 8, 8, (g.timesteps + 1) * 2, tiny_unet.attention_mode, guided=True,
                       rescale=phi > 0)
            prog.add_sampler_step("ddim", False)
            added = len(prog.ops) - prog.unet_op_count
            prog.load_latents(z_t, cond)
            prog.set_schedule([t for t in t_desc for _ in range(2)],
                              S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).to(DEV))
            prog.set_guidance(s, phi)
            for _ in t_desc:
                prog.run()
            eager = prog.z_ncdhw()
        torch.cuda.synchronize()
    assert added == (6 if phi > 0 else 4)     # update + advance, plus at most 2 (phi = 0) / 4 (phi > 0) launches
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert torch.equal(eager, runs[0])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_change_of_scale_reuses_the_captured_graph(pkg, tiny_unet, precision):
    g = pkg.GaussianDiffusion()
    shape = (1, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 45).to(DEV), _randn(shape, 46).to(DEV)
    with _precision(tiny_unet, precision):
        sp = pkg.DDIMSampler(g, tiny_unet)
        E.invalidate_engine_cache(tiny_unet)

        def run(s):
            out = sp.sample(shape, cond, 5, DEV, progress=False, z_init=z_t, guidance_scale=s)
            progs = [p for k, p in tiny_unet._ctsi_programs.items() if k[0] == "sampler-cfg"]
            assert len(progs) == 1
            return out, progs[0], progs[0].graph
        a, pa, ga = run(2.0)
        b, pb, gb = run(5.0)
        c, pc, gc = run(2.0)
    assert pa is pb is pc and ga is gb is gc and ga is not None
    assert torch.equal(a, c) and not torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 10. batches and stitching
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_batch_of_two_equals_two_single_guided_runs(pkg, tiny_unet, phi):
    g = pkg.GaussianDiffusion()
    shape = (2, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 50).to(DEV), _randn(shape, 51).to(DEV)
    kw = dict(progress=False, guidance_scale=3.0, guidance_rescale=phi)
    with _precision(tiny_unet, "fp32"):
        sp = pkg.DDIMSampler(g, tiny_unet)
        both = sp.sample(shape, cond, 6, DEV, z_init=z_t, **kw)
        one = [sp.sample((1,) + shape[1:], cond[b:b + 1], 6, DEV, z_init=z_t[b:b + 1], **kw) for b in (0, 1)]
    for b in (0, 1):
        err = rel_l2(both[b:b + 1].cpu(), one[b].cpu())
        print(f"fp32 guided phi={phi}: sample {b} of a batch of two vs alone rel-L2 {err:.3e}")
        assert err < 1e-5


def test_guided_stitching_equals_window_by_window(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v_full = formula_input((1, 1, 4, 16, 24), 17).clamp(-1, 1).to(DEV)            # two windows along w
    sampler = pkg.DDIMSampler(model.diffusion, model.unet)
    kw = dict(patch_size=(4, 16, 16), target_patch_size=(4, 16, 16), stride=(2, 8, 8), device=DEV, progress=False)
    outs = {}
    model.set_inference_precision("fp32")
    try:
        for wb in (1, None):
            torch.manual_seed(123)
            outs[wb] = sampler.sample_with_stitching(v_full, model.vae, 3, window_batch=wb, guidance_scale=3.0, **kw).cpu()
        torch.manual_seed(123)
        plain = sampler.sample_with_stitching(v_full, model.vae, 3, window_batch=None, **kw).cpu()
    finally:
        model.set_inference_precision("bf16")
    err = rel_l2(outs[None], outs[1])
    print(f"fp32 guided stitching: two windows as one batch vs one by one rel-L2 {err:.3e}")
    assert tuple(outs[1].shape) == (1, 1, 4, 16, 24) and torch.isfinite(outs[1]).all()
    assert err < 1e-5
    assert not torch.equal(outs[None], plain)


# ---------------------------------------------------------------------------------------------------------------------
# 11. generate() at config 1; the sharded refusal
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_config1_guided(pkg, full_model, monkeypatch):
    v_in = (torch.rand((1, 1, 8, 192, 192), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    nf = lambda i, s: _randn(s, 900 + i).to(DEV)
    plain = full_model.generate(v_in, 'ddim', 10, target_depth=48, noise_fn=nf)
    vae_keys = _keys(full_model.vae)
    calls = {"encode": 0, "decode": 0}
    enc, dec = full_model.vae.encode, full_model.vae.decode
    monkeypatch.setattr(full_model.vae, "encode", lambda x: (calls.__setitem__("encode", calls["encode"] + 1), enc(x))[1])
    monkeypatch.setattr(full_model.vae, "decode", lambda z: (calls.__setitem__("decode", calls["decode"] + 1), dec(z))[1])
    out = full_model.generate(v_in, 'ddim', 10, guidance_scale=3.0, target_depth=48, noise_fn=nf)
    resc = full_model.generate(v_in, 'ddim', 10, guidance_scale=3.0, target_depth=48, noise_fn=nf, guidance_rescale=0.7)
    torch.cuda.synchronize()
    assert calls == {"encode": 2, "decode": 2}              # once per call: the VAE never sees the doubled batch
    assert _keys(full_model.vae) == vae_keys                # ... and built no program for one
    for o in (out, resc):
        assert tuple(o.shape) == (1, 1, 48, 192, 192)
        assert torch.isfinite(o).all() and float(o.abs().max()) <= 1.0
    d_g, d_r = rel_l2(out.cpu(), plain.cpu()), rel_l2(resc.cpu(), out.cpu())
    print(f"config 1 generate('ddim', 10): guided s=3 vs unguided rel-L2 {d_g:.3e}; phi=0.7 vs phi=0 {d_r:.3e}")
    assert d_g > 0 and d_r > 0
    from inference.generate import generate_batch
    gb = generate_batch(full_model, v_in[:, :, :4, :64, :64].contiguous(), sampler_type='ddim', num_inference_steps=3,
                        device=DEV, noise_fn=nf, guidance_scale=2.0)
    assert torch.isfinite(gb).all()


def test_guidance_refuses_depth_sharding_before_any_launch(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    x = formula_input((1, 8, 4, 8, 8), 3).to(DEV)

    class _Comm:
        world, rank = 2, 0

    model.unet.depth_shard_comm = _Comm()
    drawn = []
    try:
        with pytest.raises(L.CtsiError, match="sharding"):
            pkg.DDIMSampler(model.diffusion, model.unet).sample(
                tuple(x.shape), x, 2, DEV, progress=False, guidance_scale=3.0,
                noise_fn=lambda i, s: drawn.append(i) or torch.zeros(s, device=DEV))
        assert not drawn and not _keys(model.unet)           # refused before the initial noise and before any program
    finally:
        del model.unet.depth_shard_comm


# ---------------------------------------------------------------------------------------------------------------------
# 12. conditioning dropout
# ---------------------------------------------------------------------------------------------------------------------
def _train_step(g, unet, z0, c, t, noise, **kw):
    for p in unet.parameters():
        p.grad = None
    loss, info = g.training_loss(unet, z0, c, t=t, noise=noise, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in unet.named_parameters()}, info


def test_cond_keep_equals_a_zeroed_conditioning(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV).train()
    g, unet = model.diffusion, model.unet
    B, shape = 4, (4, 8, 4, 8, 8)
    z0, c = formula_input(shape, 90).to(DEV), formula_input(shape, 91).to(DEV)
    t = torch.tensor([37, 812, 400, 5], device=DEV)
    noise = _randn(shape, 92).to(DEV)
    keep = torch.tensor([True, False, True, False], device=DEV)
    # is the whole micro-step bit-stable on identical inputs?  (its launches are each tested so; the step as a whole is not)
    l1, g1, info1 = _train_step(g, unet, z0, c, t, noise)
    l2, g2, _ = _train_step(g, unet, z0, c, t, noise)
    stable = torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    print(f"unmasked micro-step twice on identical inputs: {'bit-identical' if stable else 'NOT bit-identical'}")
    assert "cond_dropped" not in info1
    la, ga, info_a = _train_step(g, unet, z0, c, t, noise, cond_keep=keep)
    lb, gb, info_b = _train_step(g, unet, z0, c * keep[:, None, None, None, None], t, noise)
    assert info_a["cond_dropped"] == 2 and "cond_dropped" not in info_b
    assert not torch.equal(la, l1)
    if stable:
        assert torch.equal(la, lb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
    else:
        assert float((la - lb).abs()) <= float((l1 - l2).abs())
        for k in ga:
            assert float((ga[k] - gb[k]).float().norm()) <= float((g1[k] - g2[k]).float().norm()), k


def test_dropout_draws_after_t_and_noise_and_only_when_asked(pkg, monkeypatch):
    from tests.helpers import TINY_CFG
    TE = importlib.import_module("video-to-video-diffusion_amd.train_engine")
    B, latent = 4, (4, 8, 6, 8, 8)
    v_in = formula_input((B, 1, 2, 32, 32), 18).clamp(-1, 1).to(DEV)
    v_gt = formula_input((B, 1, 6, 32, 32), 19).clamp(-1, 1).to(DEV)
    base, _, _ = tiny_model_sd(pkg)

    def build(p):
        m = pkg.VideoToVideoDiffusion(dict(TINY_CFG, cond_drop_prob=p))
        m.load_state_dict(base.state_dict(), strict=True)
        return m.to(DEV).train()

    seen = {}
    real_step = TE.train_step

    def spy(prog, z_0, c, t, noise, norm, m):        # what reaches the engine: the conditioning after the mask
        seen.update(c=c.clone(), t=t.clone(), noise=noise.clone())
        return real_step(prog, z_0, c, t, noise, norm, m)
    monkeypatch.setattr(TE, "train_step", spy)

    def replay(seed):
        """The draws of the parent's forward (randint, then randn_like), the generator state behind them, then the
        mask draw."""
        torch.manual_seed(seed)
        t = torch.randint(0, 1000, (B,), device=DEV, dtype=torch.long)
        nz = torch.randn(latent, device=DEV)
        return t, nz, torch.cuda.get_rng_state(DEV), torch.rand(B, device=DEV) >= 0.5

    seed = next(sd for sd in range(7, 100) if 0 < int((~replay(sd)[3]).sum()) < B)     # a seed whose mask is mixed
    t_ref, n_ref, state_ref, keep_ref = replay(seed)
    # p = 0: nothing beyond t and noise is drawn; the conditioning reaches the engine whole
    m0 = build(0.0)
    torch.manual_seed(seed)
    l0, info0 = m0(v_in, v_gt)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state_ref) and "cond_dropped" not in info0
    c_full = seen["c"]
    assert torch.equal(seen["t"], t_ref) and torch.equal(seen["noise"], n_ref)
    assert all(float(c_full[b].abs().max()) > 0 for b in range(B))
    # p = 0.5: the same t and noise, and the mask is the next draw
    m5 = build(0.5)
    torch.manual_seed(seed)
    l5, info5 = m5(v_in, v_gt)
    assert torch.equal(seen["t"], t_ref) and torch.equal(seen["noise"], n_ref)
    assert info5["cond_dropped"] == int((~keep_ref).sum())
    for b in range(B):
        want = c_full[b] if bool(keep_ref[b]) else torch.zeros_like(c_full[b])
        assert torch.equal(seen["c"][b], want), b
    print(f"seed {seed}: mask {keep_ref.tolist()}, p=0 loss {l0.item():.6f}, p=0.5 loss {l5.item():.6f}, dropped "
          f"{info5['cond_dropped']} of {B}")
    # an injected mask is applied as given, whatever the probability
    _, info_inj = m0(v_in, v_gt, cond_keep=~keep_ref)
    assert info_inj["cond_dropped"] == int(keep_ref.sum())
    assert all(torch.equal(seen["c"][b], torch.zeros_like(c_full[b]) if bool(keep_ref[b]) else c_full[b])
               for b in range(B))
    # training mode at p = 1 drops everything; eval mode never drops and draws nothing more
    m1 = build(1.0)
    torch.manual_seed(seed)
    _, info_tr = m1(v_in, v_gt)
    assert info_tr["cond_dropped"] == B and float(seen["c"].abs().max()) == 0.0
    m1.eval()
    torch.manual_seed(seed)
    _, info_ev = m1(v_in, v_gt)
    assert "cond_dropped" not in info_ev and torch.equal(seen["c"], c_full)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state_ref)
