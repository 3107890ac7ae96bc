"""GPU: the two kernels of csrc/image_loss.hip against their float64 restatement (tests/image_loss_restatement.py).

ctsi_z0_pred      rel-L2 error against float64 at most 2 x that of the same expression in torch fp32
                  (_predict_z_0_from_noise / _predict_z_0_from_v of q_sample: z_t = a z0 + s noise, then (z_t - s eps) / a or
                  a z_t - s v) plus the 2e-7 floor of tests/test_gpu_fp32_mode.py -- the factor 2 is headroom for another
                  association order, the measured ratio is printed; inactive rows are z0 bit for bit; nothing non-finite at
                  t = T - 1; padding channels of the prediction (NaN here) are never read.
ctsi_loss_bwd_z0  every element within one bf16 ulp of float64 (train_audit.cmp_bf16, the bar of tests/fwd_audit.py); with a zero
                  latent gradient the bits of ctsi_mse_loss_bwd; padding channels zero.
Shapes: (2, 8, 4, 8, 8) takes the 16-byte form of ctsi_z0_pred, (1, 3, 5, 7, 9) the element-wise one."""
import ctypes as C

import pytest
import torch

from tests import image_loss_restatement as IR
from tests.helpers import rel_l2
from tests.train_audit import cmp_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2e-7
T = 1000
SHAPES = [(2, 8, 4, 8, 8), (1, 3, 5, 7, 9)]
# (t, active) per batch size: t = 0 and T - 1, every row active / mixed / none
CASES = {2: [([0, T - 1], [1, 1]), ([T - 1, 417], [0, 1]), ([3, 998], [1, 0])],
         1: [([T - 1], [1]), ([0], [1]), ([640], [0])]}


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


@pytest.fixture(scope="module")
def sched(pkg):
    g = pkg.GaussianDiffusion("cosine", T)
    return g.sqrt_alphas_cumprod.clone(), g.sqrt_one_minus_alphas_cumprod.clone()


def _data(shape, seed, c_stride):
    gen = torch.Generator().manual_seed(seed)
    n, c, d, h, w = shape
    z0, noise, pred = (torch.randn(shape, generator=gen) for _ in range(3))
    nd = torch.full((n, d, h, w, c_stride), float("nan"))
    nd[..., :c] = pred.permute(0, 2, 3, 4, 1)
    return z0, noise, pred, nd.contiguous()


@pytest.mark.parametrize("v_pred", [False, True], ids=["eps", "v"])
@pytest.mark.parametrize("pad", [0, 4], ids=["tight", "padded"])
@pytest.mark.parametrize("shape", SHAPES, ids=["vec", "elem"])
def test_z0_pred(pkg, sched, shape, pad, v_pred):
    lib = pkg.get_lib()
    a_tab, s_tab = sched
    n, c, d, h, w = shape
    cs = c + pad + (1 if (c % 4 and pad) else 0)            # (3 -> 8: still no 16-byte form; 8 -> 12: the 16-byte form, strided)
    z0, noise, pred, pred_nd = _data(shape, 5 + pad, cs)
    dev = [x.to(DEV) for x in (z0, noise, pred_nd, a_tab, s_tab)]
    for t_list, act_list in CASES[n]:
        t, act = torch.tensor(t_list), torch.tensor(act_list, dtype=torch.int32)
        out = torch.full(shape, float("nan"), device=DEV)
        t_d, act_d = t.to(DEV, torch.int32), act.to(DEV)
        lib.z0_pred(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), cs, _ptr(dev[3]), _ptr(dev[4]), _ptr(t_d), _ptr(act_d),
                    int(v_pred), n, c, d, h, w, _ptr(out), None)
        torch.cuda.synchronize()
        got = out.cpu()
        ref = IR.z0_pred_f64(z0, noise, pred, a_tab, s_tab, t, act, v_pred)
        assert bool(torch.isfinite(got).all()), (t_list, act_list)
        a, s = (x[t].reshape(-1, 1, 1, 1, 1) for x in (a_tab, s_tab))
        zt = a * z0 + s * noise
        t32 = a * zt - s * pred if v_pred else (zt - s * pred) / a
        for b in range(n):
            if not act_list[b]:
                assert torch.equal(got[b].view(torch.int32), z0[b].view(torch.int32)), (t_list, act_list, b)
                continue
            e_hip, e_t32 = rel_l2(got[b], ref[b]), rel_l2(t32[b], ref[b])
            print(f"  z0_pred {shape} stride {cs} {'v' if v_pred else 'eps'} t={t_list[b]}: hip {e_hip:.3e} torch-fp32 {e_t32:.3e} "
                  f"ratio {e_hip / (2 * e_t32 + FLOOR):.2f}")
            assert e_hip <= 2 * e_t32 + FLOOR, (shape, t_list[b], e_hip, e_t32)


@pytest.mark.parametrize("v_pred", [False, True], ids=["eps", "v"])
@pytest.mark.parametrize("use_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=["c8", "c3"])
def test_loss_bwd_z0(pkg, sched, shape, use_mask, v_pred):
    lib = pkg.get_lib()
    a_tab, s_tab = sched
    n, c, d, h, w = shape
    cs = (c + 7) // 8 * 8 + (8 if use_mask else 0)          # the engine's padded stride, and a wider one
    gen = torch.Generator().manual_seed(11 + c)
    pred, target, g_z0 = (torch.randn(shape, generator=gen) for _ in range(3))
    g_z0 = g_z0 * 1e-3
    mask = (torch.rand(n, c, d, generator=gen) > 0.4).float() if use_mask else None
    norm = torch.rand(n, generator=gen) * 1e-3 + 1e-4
    gscale = torch.tensor([0.75])
    pred_nd = pred.permute(0, 2, 3, 4, 1).contiguous()
    dv = lambda x: None if x is None else x.to(DEV)
    p_d, t_d, m_d, n_d, gs_d, g_d = (dv(x) for x in (pred_nd, target, mask, norm, gscale, g_z0))
    base = torch.full((n, d, h, w, cs), 7.0, dtype=torch.bfloat16, device=DEV)
    lib.mse_loss_bwd(_ptr(p_d), _ptr(t_d), _ptr(m_d), _ptr(n_d), _ptr(gs_d), n, c, d, h, w, _ptr(base), cs, None)
    for t_list, act_list in CASES[n]:
        t, act = torch.tensor(t_list), torch.tensor(act_list, dtype=torch.int32)
        coef = IR.z0_coef_f64(a_tab, s_tab, t, act, v_pred).float()
        out = torch.full((n, d, h, w, cs), 7.0, dtype=torch.bfloat16, device=DEV)
        act_d, coef_d = act.to(DEV), coef.to(DEV)
        lib.loss_bwd_z0(_ptr(p_d), _ptr(t_d), _ptr(m_d), _ptr(n_d), _ptr(gs_d), _ptr(g_d), _ptr(act_d), _ptr(coef_d), n, c, d, h,
                        w, _ptr(out), cs, None)
        torch.cuda.synchronize()
        got = out.cpu()
        assert bool((got[..., c:] == 0).all())
        ref = IR.loss_bwd_z0_f64(pred, target, mask, norm, 0.75, g_z0, act, coef)
        r = cmp_bf16(got[..., :c].float().permute(0, 4, 1, 2, 3), ref)
        print(f"  loss_bwd_z0 {shape} stride {cs} t={t_list} active={act_list}: {r['ulps']:.3f} ulp, rel-L2 {r['rel_l2']:.2e}")
        assert r["ok"], r
        # inactive rows: the plain loss gradient, whatever g_z0 holds
        for b in range(n):
            if not act_list[b]:
                assert torch.equal(got[b].view(torch.int16), base[b].cpu().view(torch.int16))
        # a zero latent gradient: ctsi_mse_loss_bwd's bits (its -0 of masked elements included)
        zero = torch.zeros(shape, device=DEV)
        out0 = torch.full((n, d, h, w, cs), 7.0, dtype=torch.bfloat16, device=DEV)
        lib.loss_bwd_z0(_ptr(p_d), _ptr(t_d), _ptr(m_d), _ptr(n_d), _ptr(gs_d), _ptr(zero), _ptr(act_d), _ptr(coef_d), n, c, d, h,
                        w, _ptr(out0), cs, None)
        torch.cuda.synchronize()
        assert torch.equal(out0.view(torch.int16), base.view(torch.int16))
