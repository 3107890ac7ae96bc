"""DDPM / DDIM samplers (mirror of reference inference/sampler.py) on the HIP engine, plus DPM-Solver++(2M)
(DPMSolverSampler) and EDM Heun / Euler on Karras sigmas (HeunSampler), both additive: not in the reference.

One denoising step = one replay of a captured hipGraph holding every kernel of a U-Net evaluation,
the elementwise x_{t-1} update (the sampler's engine.SAMPLER_STEPS entry: ctsi_ddim_step / ctsi_ddpm_step /
ctsi_dpm_step / ctsi_heun_step) and the increment of the device-side step counter.  Per-step scalars (timestep
embedding rows, update coefficients) come from device tables indexed by that counter, so the same graph serves all
steps and the host never synchronises inside the loop.  The reference's five isnan/isinf host checks per step are
folded into the update kernel as unconditional nan_to_num (identity on finite values).

The sampler kinds are data: _step_plan turns a kind and its settings into a StepPlan (coefficient rows, timesteps, noise
index and trajectory flag per U-Net evaluation, cache key, initial state), which the captured, depth-sharded and
generic-callable loops read.  Adding a sampler = one _step_plan branch + one engine.SAMPLER_STEPS row (and its kernel).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import logging
import math
import threading
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .consistency import check_data_consistency, refuse_depth_sharding
from .engine import (Ctx, UNetProgram, _ptr, check_attention_mode, check_device_errors,
                     check_resblock_options_unsharded, nan_to_num_, sampler_step_launcher, sampler_step_row, trilinear_depth)
from .engine_f32 import check_precision
from .engine_x3 import ACT_BYTES, unet_program
from .learned_sigma import check_learn_sigma_unsharded, check_pairing, check_var_type, respaced_ddpm_rows
from .lib import CtsiError
from .window_fuse import check_fusion, fused_program, stitch_geometry
from .x0_form import check_eps_form_timesteps, check_update_form, x0_coef_rows, x0_step_launcher

logger = logging.getLogger(__name__)

try:  # progress bars are cosmetic
    from tqdm import tqdm
except Exception:  # pragma: no cover
    tqdm = None


def _is_engine_unet(model) -> bool:
    return type(model).__name__ == "UNet3D" and hasattr(model, "program")


def _log_nonfinite(table: torch.Tensor, steps: int, max_rows: int):
    """What the reference's five NaN/Inf checkpoints log (inference/sampler.py:268-275, 288-292, 307-311, 331-334), from
    the device-side counters the update kernel keeps: one host read after the loop instead of five syncs per step."""
    t = table.cpu()
    if not bool(t.any()):
        return
    init, cond = t[max_rows], t[max_rows + 1]
    if int(init[0]) or int(init[1]):
        logger.error(f"NaN/Inf in initial noise z! NaN: {int(init[0])}, Inf: {int(init[1])}")
    if int(cond[0]) or int(cond[1]):
        logger.error(f"NaN/Inf in conditioning! NaN: {int(cond[0])}, Inf: {int(cond[1])}")
    for i in range(steps):
        r = [int(v) for v in t[i]]
        if r[0] or r[1]:
            logger.error(f"[Step {i}/{steps}] NaN/Inf in noise_pred! NaN: {r[0]}, Inf: {r[1]}")
        if r[2] or r[3]:
            logger.error(f"[Step {i}/{steps}] NaN/Inf in z_0_pred! NaN: {r[2]}, Inf: {r[3]}")
        if r[4] or r[5]:
            logger.error(f"[Step {i}/{steps}] NaN/Inf in z after update! NaN: {r[4]}, Inf: {r[5]}")


def _check_eps(eps, shape):
    if not (torch.is_tensor(eps) and tuple(eps.shape) == tuple(shape) and eps.is_cuda):
        raise CtsiError("the model callable must return a ROCm tensor of the latent's shape "
                        f"{tuple(shape)}, got {type(eps).__name__} {tuple(getattr(eps, 'shape', ()))}")


def check_guidance(guidance_scale, guidance_rescale) -> Tuple[float, float]:
    """Validate the classifier-free guidance arguments (before any launch): a finite scale (0 and negatives included; 0
    is unconditional sampling, 1 the unguided path) and a rescale phi in [0, 1].  Returns them as floats."""
    try:
        s, phi = float(guidance_scale), float(guidance_rescale)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_scale / guidance_rescale must be numbers, got {guidance_scale!r}, "
                         f"{guidance_rescale!r}") from None
    if not math.isfinite(s):
        raise ValueError(f"guidance_scale must be finite, got {guidance_scale!r}")
    if not 0.0 <= phi <= 1.0:     # (a NaN fails both comparisons)
        raise ValueError(f"guidance_rescale must lie in [0, 1], got {guidance_rescale!r}")
    return s, phi


_MEASUREMENT = threading.local()


@contextlib.contextmanager
def measurement_scope(measurement):
    """Hand a bound measurement (MeasurementGuidance.bind(y, vae), or None) to the next run_sampler call of this thread.
    run_sampler's parameter list is part of the pinned public surface and stays as it is; the call takes the value once on
    entry, so a nested or a later run is not guided by it; leaving the scope puts back what an enclosing scope had set.
    sample(measurement=None) opens no scope and so leaves an enclosing one alone."""
    outer = getattr(_MEASUREMENT, "value", None)
    _MEASUREMENT.value = measurement
    try:
        yield
    finally:
        _MEASUREMENT.value = outer


def _take_measurement():
    value = getattr(_MEASUREMENT, "value", None)
    _MEASUREMENT.value = None
    return value


def _draw_noise(noise_fn, i, shape, dev) -> torch.Tensor:
    return (noise_fn(i, tuple(shape)) if noise_fn is not None
            else torch.randn(tuple(shape), device=dev)).to(dev, torch.float32)


def ddim_coef_rows(alphas_cumprod: torch.Tensor, timesteps: Sequence[int], eta: float) -> torch.Tensor:
    """Coefficient rows for ctsi_ddim_step, computed with fp32 torch ops in the reference's order
    (sampler.py:295-325): [sqrt(1-a+1e-8), sqrt(a+1e-8)+1e-8, sqrt(a'+1e-8), sqrt(1-a'+1e-8), sigma]."""
    ac = alphas_cumprod.detach().float().cpu()
    n = len(timesteps)
    rows = torch.zeros(n, 8, dtype=torch.float32)
    for i, t_idx in enumerate(timesteps):
        a = ac[int(t_idx)]
        a_prev = ac[int(timesteps[i + 1])] if i < n - 1 else torch.tensor(1.0)
        rows[i, 0] = torch.sqrt(1 - a + 1e-8)
        rows[i, 1] = torch.sqrt(a + 1e-8) + 1e-8
        rows[i, 2] = torch.sqrt(a_prev + 1e-8)
        rows[i, 3] = torch.sqrt(1 - a_prev + 1e-8)
        if eta > 0:
            rows[i, 4] = eta * torch.sqrt((1 - a_prev + 1e-8) / (1 - a + 1e-8) * (1 - a / (a_prev + 1e-8)))
    return rows


def dpm_coef_rows(alphas_cumprod: torch.Tensor, t_desc: Sequence[int], order: int = 2,
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Coefficient rows for ctsi_dpm_step: multistep DPM-Solver++ in data prediction (Lu et al. 2022, "DPM-Solver++",
    Algorithm 2) on the timestep list `t_desc`, the last target being abar = 1 as in the reference DDIM.

    With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log alpha - log sigma and h_i = lambda_{i+1} - lambda_i,
    step i maps z_i to z_{i+1} = a_i z_i + b_i x0_i + c_i x0_{i-1}, x0_i = clamp(nan_to_num((z_i - sigma_i eps_i) /
    alpha_i), -10, 10):
      first order (step 0, order=1):  a = sigma_{i+1}/sigma_i,  b = alpha_{i+1} (1 - e^-h),  c = 0  (= DDIM, eta 0)
      second order:  r = h_{i-1}/h_i,  b = alpha_{i+1} (1 - e^-h) (1 + 1/2r),  c = -alpha_{i+1} (1 - e^-h) / 2r
      final step (sigma = 0, lambda = +inf): first order, exactly a = 0, b = 1, c = 0.
    Rows [1/alpha_i, sigma_i/alpha_i, a_i, b_i, c_i, 0, 0, 0], computed in float64 and rounded once to fp32 (`dtype`
    = torch.float64 returns them unrounded)."""
    if order not in (1, 2):
        raise ValueError(f"DPM-Solver++ order must be 1 or 2, got {order}")
    ac = alphas_cumprod.detach().double().cpu().numpy()
    n = len(t_desc)
    abar = np.array([ac[int(t)] for t in t_desc], dtype=np.float64)
    alpha, sigma = np.sqrt(abar), np.sqrt(1.0 - abar)
    lam = np.log(alpha) - np.log(sigma)
    rows = np.zeros((n, 8), dtype=np.float64)
    rows[:, 0] = 1.0 / alpha
    rows[:, 1] = sigma / alpha
    h_prev = None
    for i in range(n):
        if i == n - 1:
            rows[i, 2:5] = (0.0, 1.0, 0.0)
            break
        h = lam[i + 1] - lam[i]
        phi = -np.expm1(-h)                         # 1 - e^{-h}
        rows[i, 2] = sigma[i + 1] / sigma[i]
        if order == 1 or h_prev is None:
            rows[i, 3] = alpha[i + 1] * phi
        else:
            r = h_prev / h
            rows[i, 3] = alpha[i + 1] * phi * (1.0 + 0.5 / r)
            rows[i, 4] = -alpha[i + 1] * phi * (0.5 / r)
        h_prev = h
    return torch.from_numpy(rows).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# EDM (Karras et al. 2022, Algorithm 2) on the VP model: sigma = sqrt((1 - abar) / abar), x = z * a(sigma),
# a(sigma) = sqrt(1 + sigma^2).  Host side in float64; the device update is ctsi_heun_step.
# ---------------------------------------------------------------------------------------------------------------------
def sigma_table(alphas_cumprod: torch.Tensor) -> np.ndarray:
    """sigma_k = sqrt((1 - abar_k) / abar_k), k = 0..T-1, float64 (increasing; the last is inf on a zero-terminal-SNR
    schedule, abar_{T-1} = 0)."""
    ac = alphas_cumprod.detach().double().cpu().numpy()
    with np.errstate(divide="ignore"):
        return np.sqrt((1.0 - ac) / ac)


def karras_sigmas(n: int, sigma_min: float, sigma_max: float, rho: float = 7.0) -> np.ndarray:
    """The rho-schedule (Karras et al. 2022, eq. 5): sigma_i = (sigma_max^(1/rho) + i/(n-1) (sigma_min^(1/rho) -
    sigma_max^(1/rho)))^rho for i < n, then sigma_n = 0; n = 1 gives [sigma_max, 0].  float64, n + 1 entries."""
    n = int(n)
    if n < 1:
        raise ValueError(f"the EDM schedule needs at least one step, got {n}")
    if not (0.0 < sigma_min <= sigma_max and math.isfinite(sigma_max)):
        raise ValueError(f"need 0 < sigma_min <= sigma_max < inf, got {sigma_min}, {sigma_max}")
    if not rho > 0:
        raise ValueError(f"rho must be positive, got {rho}")
    if n == 1:
        return np.array([float(sigma_max), 0.0])
    lo, hi = float(sigma_min) ** (1.0 / rho), float(sigma_max) ** (1.0 / rho)
    s = (hi + np.arange(n, dtype=np.float64) / (n - 1) * (lo - hi)) ** rho
    s[0], s[-1] = sigma_max, sigma_min            # the endpoints exactly (pow(pow(x, 1/rho), rho) rounds)
    return np.append(s, 0.0)


def sigma_to_t(sigma, alphas_cumprod: torch.Tensor):
    """The (fractional) timestep of a noise level: for sigma_k <= sigma <= sigma_{k+1},
    t = k + (ln sigma - ln sigma_k) / (ln sigma_{k+1} - ln sigma_k), clamped to [0, T-1].  Exactly k at a table value.
    Scalar in, float out; array in, float64 array out."""
    table = sigma_table(alphas_cumprod)
    table = table[np.isfinite(table)]      # a zero-terminal-SNR schedule ends in sigma = inf: t then lies in [0, T-2]
    T = len(table)
    sig = np.asarray(sigma, dtype=np.float64)
    k = np.clip(np.searchsorted(table, sig, side="right") - 1, 0, T - 2)
    ls = np.log(table)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = k + (np.log(np.maximum(sig, table[0])) - ls[k]) / (ls[k + 1] - ls[k])
    t = np.where(sig <= table[0], 0.0, np.where(sig >= table[-1], float(T - 1), t))
    t = np.clip(t, 0.0, float(T - 1))
    return float(t) if t.ndim == 0 else t


class HeunRows(NamedTuple):
    """What ctsi_heun_step needs for one sampling run (sampler.heun_coef_rows)."""
    rows: torch.Tensor            # (E, 8) coefficient rows, one per U-Net evaluation (fp32 unless asked otherwise)
    t: np.ndarray                 # (E,) float64 timestep of every evaluation
    sigma_eval: np.ndarray        # (E,) float64 noise level of every evaluation
    sigmas: np.ndarray            # (N + 1,) the schedule, ending in 0
    sigma_hat: np.ndarray         # (N,) sigma_i (1 + gamma_i)
    gammas: np.ndarray            # (N,)
    noise_step: List[int]         # (E,) step i whose churn noise eps_i the row consumes, or -1
    closes: List[bool]            # (E,) True for the row that completes a step
    init: Tuple[float, float]     # zhat_0 = init[0] eps + init[1] eps_0 (eps_0: step 0's churn noise)


def heun_coef_rows(alphas_cumprod: torch.Tensor, sigmas: Sequence[float], order: int = 2, s_churn: float = 0.0,
                   s_tmin: float = 0.0, s_tmax: float = float("inf"), s_noise: float = 1.0,
                   dtype: torch.dtype = torch.float32) -> HeunRows:
    """Coefficient rows for ctsi_heun_step: EDM (Karras et al. 2022, Algorithm 2) on the descending noise levels
    `sigmas` (a trailing 0 is appended when missing), with the denoiser D(x, sigma) = clamp(nan_to_num(x - sigma
    eps(x / a(sigma), t(sigma))), -10, 10) of the reference DDIM.

    Step i: gamma_i = min(S_churn / N, sqrt 2 - 1) on S_tmin <= sigma_i <= S_tmax (else 0), sigma_hat = sigma_i (1 +
    gamma_i), xhat = x_i + S_noise sqrt(sigma_hat^2 - sigma_i^2) eps_i; Euler predictor x' = xhat + (sigma_{i+1} -
    sigma_hat) (xhat - D1) / sigma_hat; at order 2 with sigma_{i+1} > 0 the corrector averages the two slopes.

    The device state is zhat = xhat / a(sigma_hat), so with A = a(sigma_hat), p = A sigma_{i+1} / sigma_hat,
    q = 1 - sigma_{i+1} / sigma_hat, a' = a(sigma_{i+1}), A' = a(sigma_hat_{i+1}) and k' = S_noise sqrt(sigma_hat_{i+1}^2 -
    sigma_{i+1}^2) / A' (the next step's churn, fused into this step's closing row):
      predictor  [A, 0, sigma_hat, 0, p/a', q/a', 0, 0]              zin = z' = x'/a'
      corrector  [p, q, sigma_{i+1}, 1, p/A', -h/(2 sigma_{i+1} A'), h (1/sigma_{i+1} - 2/sigma_hat) / (2 A'), k']
                 with h = sigma_{i+1} - sigma_hat  (x' = p zhat + q D1 is recomputed, not stored)
      Euler      [A, 0, sigma_hat, 1, p/A', q/A', 0, k']
      final      [A, 0, sigma_hat, 1, 0, 1, 0, 0]                      (sigma_{i+1} = 0: x_N = D1 exactly)
    Order 2 costs 2N - 1 evaluations, order 1 N.  Computed in float64, rounded once to `dtype`."""
    if order not in (1, 2):
        raise ValueError(f"the EDM sampler's order must be 1 (Euler) or 2 (Heun), got {order}")
    sig = np.asarray([float(v) for v in sigmas], dtype=np.float64)
    if sig.ndim != 1 or len(sig) == 0 or not np.isfinite(sig).all():
        raise ValueError("sigmas must be a non-empty list of finite noise levels")
    if sig[-1] != 0.0:
        sig = np.append(sig, 0.0)
    if len(sig) < 2 or not (sig[:-1] > 0).all() or not (np.diff(sig) < 0).all():
        raise ValueError(f"sigmas must be strictly descending and positive (then 0), got {sig.tolist()}")
    if not (s_churn >= 0 and s_noise >= 0 and s_tmin <= s_tmax):
        raise ValueError(f"bad churn settings: s_churn={s_churn}, s_noise={s_noise}, s_tmin={s_tmin}, s_tmax={s_tmax}")
    T = int(alphas_cumprod.shape[0])
    N = len(sig) - 1
    evals = 2 * N - 1 if order == 2 else N
    if evals > T + 1:
        raise ValueError(f"{N} EDM steps of order {order} need {evals} U-Net evaluations; at most T + 1 = {T + 1}")
    a = lambda v: math.sqrt(1.0 + v * v)
    gam = np.array([min(s_churn / N, math.sqrt(2.0) - 1.0) if (s_tmin <= sig[i] <= s_tmax and s_churn > 0) else 0.0
                    for i in range(N)])
    sh = sig[:N] * (1.0 + gam)
    churn = np.array([s_noise * math.sqrt(max(sh[i] ** 2 - sig[i] ** 2, 0.0)) if gam[i] > 0 else 0.0
                      for i in range(N)])
    rows, sev, noise_step, closes = [], [], [], []
    for i in range(N):
        s_hat, s1, A = sh[i], sig[i + 1], a(sh[i])
        if s1 == 0.0:
            rows.append([A, 0.0, s_hat, 1.0, 0.0, 1.0, 0.0, 0.0])
            sev.append(s_hat), noise_step.append(-1), closes.append(True)
            continue
        p, q = A * s1 / s_hat, 1.0 - s1 / s_hat
        A_next = a(sh[i + 1])
        k_next = churn[i + 1] / A_next
        nxt = i + 1 if gam[i + 1] > 0 else -1
        if order == 1:
            rows.append([A, 0.0, s_hat, 1.0, p / A_next, q / A_next, 0.0, k_next])
            sev.append(s_hat), noise_step.append(nxt), closes.append(True)
            continue
        a1, hh = a(s1), s1 - s_hat
        rows.append([A, 0.0, s_hat, 0.0, p / a1, q / a1, 0.0, 0.0])
        sev.append(s_hat), noise_step.append(-1), closes.append(False)
        rows.append([p, q, s1, 1.0, p / A_next, -hh / (2.0 * s1) / A_next,
                     0.5 * hh * (1.0 / s1 - 2.0 / s_hat) / A_next, k_next])
        sev.append(s1), noise_step.append(nxt), closes.append(True)
    sev = np.asarray(sev)
    A0 = a(sh[0])
    return HeunRows(rows=torch.from_numpy(np.asarray(rows, dtype=np.float64)).to(dtype),
                    t=np.asarray(sigma_to_t(sev, alphas_cumprod), dtype=np.float64).reshape(-1),
                    sigma_eval=sev, sigmas=sig, sigma_hat=sh, gammas=gam, noise_step=noise_step, closes=closes,
                    init=(sig[0] / A0, churn[0] / A0))


def heun_pred_rows(heun: HeunRows, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """ctsi_pred_to_eps rows {a, b0, b1, 0} for the evaluations of an EDM run under v-prediction.  At
    the noise level sigma = sigma_eval[e] the VP coefficients are alpha = 1 / sqrt(1 + sigma^2), beta = sigma alpha, and
    eps = alpha v + beta zin with zin the network's input.  A predictor, Euler or final row evaluates the network on the state
    zhat itself: {alpha, beta, 0}.  A corrector row evaluates it on z' = c4 zhat + c5 D1 (c4 = p / a', c5 = q / a' of the
    preceding predictor row), which the engine recomputes instead of storing: {alpha, beta c4, beta c5} with the D1 buffer
    as `hist`.  float64, rounded once to `dtype`."""
    E = len(heun.sigma_eval)
    rows = np.zeros((E, 4), dtype=np.float64)
    a = lambda v: math.sqrt(1.0 + v * v)
    step = 0
    for e in range(E):
        sg = float(heun.sigma_eval[e])
        alpha = 1.0 / a(sg)
        beta = sg * alpha
        if e > 0 and not heun.closes[e - 1]:            # the corrector of step `step`: sigma_eval[e] = sigma_{step+1}
            s_hat, s1 = float(heun.sigma_hat[step]), float(heun.sigmas[step + 1])
            c4 = a(s_hat) * s1 / s_hat / a(s1)
            c5 = (1.0 - s1 / s_hat) / a(s1)
            rows[e] = (alpha, beta * c4, beta * c5, 0.0)
        else:
            rows[e] = (alpha, beta, 0.0, 0.0)
        if heun.closes[e]:
            step += 1
    return torch.from_numpy(rows).to(dtype)


class LvRows(NamedTuple):
    """What kind 'ddpm_lv' needs for one sampling run (sampler.lv_rows)."""
    rows: torch.Tensor            # (N, 8) ctsi_ddpm_lv_step rows of the whole chain (learned_sigma.respaced_ddpm_rows)
    chain: Tuple[int, ...]        # (N,) its descending timesteps
    learned: bool                 # the step reads the model's variance channels (var_type 'learned_range')


def lv_rows(diffusion, chain: Sequence[int], clip: bool = True) -> LvRows:
    learned = check_var_type(getattr(diffusion, "var_type", "fixed_small")) == "learned_range"
    return LvRows(respaced_ddpm_rows(diffusion, chain, clip), tuple(int(t) for t in chain), learned)


class StepPlan(NamedTuple):
    """One sampling run as data, per U-Net evaluation e (E = len(t)).  run_sampler, run_sampler_sharded and the
    generic-callable loop read it and never test the sampler kind; only _step_plan builds one."""
    kind: str                       # the engine.SAMPLER_STEPS row of the update (and the progress-bar label)
    coef: torch.Tensor              # (E, 8) update coefficient rows
    t: tuple                        # (E,) timestep: int (ddim, ddpm, dpmpp) or float (heun)
    t_dtype: torch.dtype            # the generic callable's t: torch.long, or torch.float32 (heun, integral or not)
    noise_step: Tuple[int, ...]     # (E,) the noise_fn index consumed before evaluation e's update, or -1
    closes: Tuple[bool, ...]        # (E,) evaluation e completes a step (gets a trajectory entry)
    with_noise: bool                # the step program holds a noise buffer
    logs_nonfinite: bool            # the reference logs NaN / Inf for this sampler (its DDPM loop does not)
    key: tuple                      # (kind, with_noise): the sampler's part of the program cache keys ...
    key_order: tuple                # ... and their last element: (order,) for dpmpp / heun, else ()
    init: Optional[Tuple[float, float]] = None     # z_0 = init[0] eps + init[1] eps_0; None: z_0 = eps
    init_noise: bool = False                       # eps_0 = noise_fn(0, shape) is drawn (step 0 churns)
    pred: Optional[torch.Tensor] = None            # (E, 4) ctsi_pred_to_eps rows under 'v_prediction'; None: the output is eps
    x0: bool = False                               # update_form 'x0': coef holds ctsi_x0_step rows, the update reads the raw v
    learned: bool = False                          # the update reads the variance channels of a learn_sigma model (section 24)

    def initial_state(self, z0: torch.Tensor, noise_fn, shape, dev) -> torch.Tensor:
        """The loop's start from the initial draw eps = z0 (Heun's zhat_0 is formed in float64)."""
        if self.init is None:
            return z0
        zh = self.init[0] * z0.to(dev, torch.float64)
        if self.init_noise:
            zh += self.init[1] * _draw_noise(noise_fn, 0, shape, dev).double()
        return zh.float()


def _step_plan(diffusion, kind: str, t_desc: Sequence, eta: float, order: int,
               rows: "Optional[HeunRows | LvRows]") -> StepPlan:
    """The only place that branches on the sampler kind.  A new sampler adds one branch here and one row to
    engine.SAMPLER_STEPS (its update entry and operands).  `rows`: the host rows of the kinds that bring their own -- 'heun'
    takes HeunRows (t_desc = rows.t); 'ddpm_lv'  takes LvRows, the respaced rows of a chain of which t_desc
    is a prefix, and reads the learned variance when they say so (diffusion.var_type 'learned_range').  run_sampler and
    run_sampler_sharded hand over what they receive as `heun=`, the name that slot had while Heun was its only user and
    that their parameter lists keep."""
    heun = rows if isinstance(rows, HeunRows) else None
    lv = rows if isinstance(rows, LvRows) else None
    E = len(t_desc)
    # v-prediction: the conversion rows, and the prediction type in the program cache keys (the epsilon keys stay as they are)
    v_pred = getattr(diffusion, "prediction_type", "epsilon") == "v_prediction"
    vkey = ("v_prediction",) if v_pred else ()
    # the x0 form of the three integer-timestep samplers; Heun evaluates finite noise levels only and
    # keeps its eps-form rows
    x0 = check_update_form(getattr(diffusion, "update_form", "eps"),
                           getattr(diffusion, "prediction_type", "epsilon")) == "x0"
    if kind == "heun":
        if heun is None or len(heun.t) != E:
            raise ValueError("kind='heun' needs the rows of heun_coef_rows(...) (heun=) and t_desc = heun.t")
        with_noise = bool((heun.gammas > 0).any())        # churn on
        return StepPlan(kind, heun.rows, tuple(float(t) for t in t_desc), torch.float32, tuple(heun.noise_step),
                        tuple(heun.closes), with_noise, True, (kind, with_noise) + vkey, (order,), init=heun.init,
                        init_noise=bool(heun.gammas[0] > 0), pred=heun_pred_rows(heun) if v_pred else None)
    if kind == "ddpm_lv":
        learned = lv is not None and lv.learned
        if x0:
            raise CtsiError("update_form='x0' does not support the strided ancestral sampler or a learned reverse variance: "
                            "the x0-form DDPM row carries one scalar noise scale; sample with 'ddpm' on fixed_small, a "
                            "deterministic sampler, or update_form='eps'")
        if lv is None or [int(t) for t in t_desc] != list(lv.chain[:E]):
            raise ValueError("kind='ddpm_lv' needs the rows of lv_rows(...) (rows=; heun= of run_sampler) and t_desc = a prefix "
                             "of their chain")
        check_eps_form_timesteps(diffusion.alphas_cumprod, t_desc)
        return StepPlan(kind, lv.rows[:E], tuple(int(t) for t in t_desc), torch.long,
                        tuple(range(E)), (True,) * E, True, False, (kind, True) + vkey + (("learned",) if learned else ()), (),
                        pred=diffusion.pred_to_eps_rows(t_desc) if v_pred else None, learned=learned)
    if kind not in ("ddim", "ddpm", "dpmpp"):
        raise ValueError(f"unknown sampler kind {kind!r}: expected 'ddim', 'ddpm', 'ddpm_lv', 'dpmpp' or 'heun'")
    if x0:
        coef = x0_coef_rows(diffusion, kind, t_desc, eta, order)
    elif kind == "ddim":
        check_eps_form_timesteps(diffusion.alphas_cumprod, t_desc)
        coef = ddim_coef_rows(diffusion.alphas_cumprod, t_desc, eta)
    elif kind == "ddpm":
        check_eps_form_timesteps(diffusion.alphas_cumprod, t_desc)
        coef = diffusion.ddpm_coef_rows(t_desc)
    else:
        check_eps_form_timesteps(diffusion.alphas_cumprod, t_desc)
        coef = dpm_coef_rows(diffusion.alphas_cumprod, t_desc, order)
    with_noise = kind == "ddpm" or eta > 0
    return StepPlan(kind, coef, tuple(int(t) for t in t_desc), torch.long,
                    tuple(range(E)) if with_noise else (-1,) * E, (True,) * E, with_noise, kind != "ddpm",
                    (kind, with_noise) + vkey + (("x0",) if x0 else ()), (order,) if kind == "dpmpp" else (),
                    pred=diffusion.pred_to_eps_rows(t_desc) if v_pred and not x0 else None, x0=x0)


def _progress(plan: StepPlan, progress: bool):
    it = range(len(plan.t))
    if progress and tqdm is not None:
        it = tqdm(it, desc=f"{plan.kind.upper()} Sampling", total=len(plan.t))
    return it


def _replay(plan: StepPlan, evals, load_noise, launch):
    """The per-evaluation body of the step-program loops (run_sampler, run_sampler_sharded): the noise the update
    consumes is loaded first (load_noise(noise_fn index)), then one launch.  Yields closes[e]: the caller records a
    trajectory entry on the evaluations that complete a step."""
    for e in evals:
        if plan.noise_step[e] >= 0:
            load_noise(plan.noise_step[e])
        launch()
        yield plan.closes[e]


def _run_generic(plan: StepPlan, model, shape, conditioning, ctx, z0, *, noise_fn, progress, trajectory,
                 eps_trajectory, guidance: Optional[Tuple[float, float]] = None):
    """Reverse loop over an ARBITRARY `model(z, t, c) -> eps` callable (the reference's samplers accept any,
    inference/sampler.py:211-219): the network evaluation is the caller's (any torch code on the ROCm device), the
    update with its guards is the engine's `_f32` entry of the plan's kind, once per evaluation.  Not captured: the
    callable is opaque.  The engine's own UNet3D takes the hipGraph path in run_sampler instead.
    The model sees t as plan.t_dtype (Heun's fractional timesteps as fp32, as the reference embeds t) and as z the
    input the update writes to `zin`: the new state, or after a Heun predictor row the corrector's z' (z keeps zhat).
    Under 'v_prediction' (plan.pred) the callable returns v: ctsi_pred_to_eps turns the evaluation's rows into eps before
    the guidance and the update, as in the step programs; eps_trajectory holds that eps.  Under update_form 'x0' (plan.x0)
    there is no conversion: the guidance and ctsi_x0_step_f32 read the raw v, and eps_trajectory holds it.
    `guidance` = (s, phi): classifier-free guidance -- two calls per evaluation, model(z, t, c) and model(z, t,
    zeros_like(c)), combined by ctsi_cfg_combine (the entry of the guided step program); eps_trajectory then holds the
    guided eps."""
    if plan.learned:
        raise CtsiError("the generic model(z, t, c) callable path does not support a learned reverse variance (a 2L-channel "
                        "output): pass the engine's UNet3D(learn_sigma=True), or set var_type='fixed_small'")
    lib, sptr = ctx.lib, ctx.sptr
    n, L, d, h, w = [int(v) for v in shape]
    evals = len(plan.t)
    dev = ctx.device
    step = x0_step_launcher(lib, True) if plan.x0 else sampler_step_launcher(lib, plan.kind, f32=True)
    coef = plan.coef.to(dev, torch.float32).contiguous()
    z_nd = torch.empty((n, d, h, w, L), dtype=torch.float32, device=dev)
    zin_nd = torch.empty_like(z_nd)
    eps_nd = torch.empty(((2 if guidance else 1) * n, d, h, w, L), dtype=torch.float32, device=dev)
    hist = torch.zeros_like(z_nd) if sampler_step_row(plan.kind).hist else None
    pred = None
    if plan.pred is not None:
        if hist is None and bool((plan.pred[:, 2] != 0).any()):
            raise CtsiError("internal: a conversion row reads the history buffer but the sampler kind has none")
        pred = plan.pred.to(dev, torch.float32).contiguous()
    step_ptr = torch.zeros(1, dtype=torch.int32, device=dev)
    nonfinite = torch.zeros((evals + 2, 6), dtype=torch.int32, device=dev)
    cond = conditioning.to(dev)
    z = z0.to(dev, torch.float32).contiguous()
    if guidance:
        null_cond = torch.zeros_like(cond)
        cfg_scale = torch.tensor([guidance], dtype=torch.float32, device=dev)
        cfg_stats = cfg_partials = None
        if guidance[1] > 0.0:
            cfg_partials = torch.zeros(n * lib.cfg_stats_blocks(L * d * h * w) * 4, dtype=torch.float64, device=dev)
            cfg_stats = torch.zeros((n, 4), dtype=torch.float64, device=dev)
        eps_u_nd = eps_nd[n:]
    with ctx.scope():
        lib.count_nonfinite_f32(_ptr(z), z.numel(), 1, C.c_void_p(nonfinite.data_ptr() + evals * 24), sptr)
        cf = cond.float().contiguous()
        lib.count_nonfinite_f32(_ptr(cf), cf.numel(), 0, C.c_void_p(nonfinite.data_ptr() + (evals + 1) * 24), sptr)
        lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), _ptr(z_nd), n, L, d, h, w, sptr)
    for e in _progress(plan, progress):
        t = torch.full((n,), plan.t[e], device=dev, dtype=plan.t_dtype)
        eps = model(z, t, cond)
        _check_eps(eps, shape)
        eps = eps.detach().to(torch.float32).contiguous()
        if guidance:
            eps_u = model(z, t, null_cond)
            _check_eps(eps_u, shape)
            eps_u = eps_u.detach().to(torch.float32).contiguous()
        elif eps_trajectory is not None and pred is None:
            eps_trajectory.append(eps.clone())
        noise = None
        if plan.noise_step[e] >= 0:
            noise = _draw_noise(noise_fn, plan.noise_step[e], shape, dev).contiguous()
        with ctx.scope():
            lib.ncdhw_f32_to_ndhwc_f32(_ptr(eps), _ptr(eps_nd), n, L, d, h, w, sptr)
            if guidance:
                lib.ncdhw_f32_to_ndhwc_f32(_ptr(eps_u), _ptr(eps_u_nd), n, L, d, h, w, sptr)
            if pred is not None:
                lib.pred_to_eps(_ptr(eps_nd), _ptr(z_nd), _ptr(hist), _ptr(pred), _ptr(step_ptr), 1, eps_nd.shape[0], n,
                                L * d * h * w, sptr)
                if not guidance and eps_trajectory is not None:
                    eps_c = torch.empty((n, L, d, h, w), dtype=torch.float32, device=dev)
                    lib.ndhwc_f32_to_ncdhw_f32(_ptr(eps_nd), _ptr(eps_c), n, L, d, h, w, sptr)
                    eps_trajectory.append(eps_c)
            if guidance:
                if cfg_stats is not None:
                    lib.cfg_stats(_ptr(eps_nd), _ptr(cfg_scale), None, _ptr(cfg_partials), n, L, d, h, w, sptr)
                    lib.cfg_stats_finalize(_ptr(cfg_partials), _ptr(cfg_stats), n, L, d, h, w, sptr)
                lib.cfg_combine(_ptr(eps_nd), _ptr(cfg_scale), None, _ptr(cfg_stats), n, L, d, h, w, sptr)
                if eps_trajectory is not None:
                    eps_g = torch.empty((n, L, d, h, w), dtype=torch.float32, device=dev)
                    lib.ndhwc_f32_to_ncdhw_f32(_ptr(eps_nd), _ptr(eps_g), n, L, d, h, w, sptr)
                    eps_trajectory.append(eps_g)
            step(_ptr(z_nd), _ptr(eps_nd), _ptr(hist), _ptr(noise), _ptr(zin_nd), L, _ptr(coef), _ptr(step_ptr), n, L,
                 d, h, w, _ptr(nonfinite), sptr)
            lib.step_advance(_ptr(step_ptr), sptr)
            z = torch.empty((n, L, d, h, w), dtype=torch.float32, device=dev)
            lib.ndhwc_f32_to_ncdhw_f32(_ptr(zin_nd), _ptr(z), n, L, d, h, w, sptr)
        if trajectory is not None and plan.closes[e]:
            trajectory.append(z.clone())
    if plan.logs_nonfinite:
        _log_nonfinite(nonfinite, evals, evals)
    return z


def run_sampler_sharded(diffusion, unet, shape, conditioning, ctx, z0, *, kind, t_desc, eta, noise_fn, comm,
                        trajectory=None, order=2, heun=None):
    """Depth-sharded reverse loop: this process owns depth slab `comm.rank` of the volume (parallel.RcclComm: RCCL
    issued by libctsi on the engine stream; parallel.DistComm under the gloo tests).  Every rank passes the full
    conditioning / initial noise and gets the full result back (all-gather along depth).  A batch runs volume by
    volume through the one-volume sharded program (every rank holds 1/world of ONE volume at a time).
    With a capture-safe transport and CTSI_SHARD_CAPTURE=1 the step -- kernels AND collectives -- is replayed as one
    hipGraph, like the single-GPU step.
    DPM-Solver++ ('dpmpp'): the update is elementwise over the rank's own slab (its history buffer too), and step 0's
    row (c = 0) overwrites that history, so volume b + 1 starts clean.
    Heun ('heun', rows `heun`): one launch per evaluation, elementwise over the slab; D1 is written by every predictor
    before its corrector reads it, and the churn noise slab is copied only before the rows that consume it."""
    import os
    from .engine import cached_program
    from .parallel import ShardSpec
    plan = _step_plan(diffusion, kind, t_desc, eta, order, heun)
    n, L, d, h, w = [int(v) for v in shape]
    spec = ShardSpec(comm.rank, comm.world, comm, d)
    dl, lo = spec.depth_local, spec.depth_start
    capture = bool(getattr(comm, "capturable", False)) and os.environ.get("CTSI_SHARD_CAPTURE") == "1"
    outs, trajs = [], [[] for _ in range(sum(plan.closes))]
    with ctx.scope():
        key = ("sampler-shard", ctx.device.index, 1, d, h, w, comm.rank, comm.world) + plan.key + plan.key_order

        def build():
            v_out = plan.pred is not None or plan.x0
            kw = dict(prediction="v_prediction") if v_out else {}                   # elementwise on the rank's slab
            prog = UNetProgram(ctx, unet, 1, dl, h, w, diffusion.timesteps + 1, "fast", shard=spec, **kw)
            prog.add_sampler_step(plan.kind, plan.with_noise, **(dict(update_form="x0") if plan.x0 else {}))
            return prog

        prog = cached_program(unet, key, build)
        noises = {}
        for b in range(n):
            def load_noise(i, b=b):
                if i not in noises:   # one draw per step for the whole batch, as the unsharded loop makes it
                    noises[i] = (noise_fn(i, tuple(shape)) if noise_fn is not None
                                 else torch.randn(tuple(shape), device=ctx.device))
                prog.noise.copy_(noises[i][b:b + 1, :, lo:lo + dl].to(ctx.device, torch.float32))

            prog.load_latents(z0[b:b + 1], conditioning[b:b + 1])
            prog.set_schedule(list(plan.t), plan.coef.to(ctx.device), plan.pred)
            if capture and prog.graph is None:
                prog.capture()
                prog.step_ptr.zero_()
            done = 0
            for closes in _replay(plan, range(len(plan.t)), load_noise, prog.launch if capture else prog.run):
                if trajectory is not None and closes:
                    trajs[done].append(comm.gather_depth(comm.rank, prog.z_ncdhw(), counts=spec.depth_counts))
                    done += 1
            outs.append(comm.gather_depth(comm.rank, prog.z_ncdhw(), counts=spec.depth_counts))
        if trajectory is not None:
            trajectory.extend(torch.cat(t, dim=0) for t in trajs)
        res = torch.cat(outs, dim=0)
        torch.cuda.current_stream(ctx.device).synchronize()
        check_device_errors(ctx)
        return res


def _run_step_program(prog: UNetProgram, plan: StepPlan, ctx, shape, conditioning, z0, nb: int, *, noise_fn, progress,
                      guidance: Optional[Tuple[float, float]], trajectory, eps_trajectory, guide=None):
    """The reverse loop on a step program (inside ctx.scope()): run_sampler's on the latent `shape`, run_sampler_fused's on the
    full latent's with the windows' conditioning.  `nb`: network rows of one evaluation (timestep rows per evaluation);
    `shape`: the state's, which the noise draws and both trajectories have.  Returns the final state, fp32 NCDHW.
    `guide` (a measurement_guidance.GuideRun): its guided evaluations save the state before the replay of the
    unchanged captured step and issue the correction eagerly behind it; the trajectory entries hold the corrected state."""
    prog.load_latents(z0, conditioning)
    prog.nonfinite.zero_()
    nf_tail = prog.nonfinite.data_ptr() + prog.max_rows * 24
    # sampler.py:268-275: checkpoint 1 sanitises the initial noise (identity on finite values), checkpoint 2 only
    # reports on the conditioning; both are counted on device and logged after the loop
    ctx.lib.count_nonfinite_f32(_ptr(prog.z), prog.z.numel(), 1, C.c_void_p(nf_tail), ctx.sptr)
    cnd = conditioning.detach().to(ctx.device, torch.float32).contiguous()
    ctx.lib.count_nonfinite_f32(_ptr(cnd), cnd.numel(), 0, C.c_void_p(nf_tail + 24), ctx.sptr)
    cnd.record_stream(ctx.stream)
    prog.set_schedule([t for t in plan.t for _ in range(nb)], plan.coef.to(ctx.device), plan.pred)
    if guidance is not None:
        prog.set_guidance(*guidance)     # a device write: the same captured graph serves every scale
    if prog.graph is None:
        # one eager warm-up step is not needed: capture records launches without executing them
        prog.capture()
        prog.step_ptr.zero_()

    def load_noise(i):
        if noise_fn is not None:
            prog.noise.copy_(noise_fn(i, tuple(shape)).to(ctx.device, torch.float32))
        else:
            prog.noise.normal_()

    launch = prog.launch
    if guide is not None and guide.evals:
        done = [0]

        def launch():
            e, done[0] = done[0], done[0] + 1
            if e not in guide.slot:
                return prog.launch()
            guide.save_state(prog)
            prog.launch()
            guide.correct(prog, e)

    for closes in _replay(plan, _progress(plan, progress), load_noise, launch):
        if trajectory is not None and closes:
            trajectory.append(prog.z_ncdhw())
        if eps_trajectory is not None:
            eps_trajectory.append(prog.eps_ncdhw())
    out = prog.z_ncdhw()
    if plan.logs_nonfinite:     # (one host read: the loop itself never synchronises)
        _log_nonfinite(prog.nonfinite, len(plan.t), prog.max_rows)
    check_device_errors(ctx)
    return out


def run_sampler(diffusion, model, shape, conditioning, device, *, kind: str, t_desc: Sequence[int],
                progress: bool, eta: float = 0.0, noise_fn=None, z_init: Optional[torch.Tensor] = None,
                trajectory: Optional[list] = None, order: int = 2, eps_trajectory: Optional[list] = None,
                heun: "Optional[HeunRows | LvRows]" = None, guidance_scale: float = 1.0, guidance_rescale: float = 0.0):
    """Shared reverse loop.  kind: 'ddim' | 'ddpm' | 'dpmpp' (DPM-Solver++ of `order` 1 or 2) | 'heun' (EDM of `order` 1
    or 2 on the rows `heun` = heun_coef_rows(...), t_desc = heun.t) | 'ddpm_lv' (the ancestral step on the respaced rows
    `heun` = lv_rows(...) -- the slot takes the host rows of either kind and keeps its first user's name -- t_desc a prefix
    of their chain; under diffusion.var_type == 'learned_range' the step reads the
    variance channels of the UNet3D(learn_sigma=True) -- taken from the conditional rows under guidance -- DESIGN section 24);
    t_desc: descending timestep list.
    `eps_trajectory` (unsharded runs only): receives the noise prediction of every U-Net evaluation, fp32 NCDHW.
    'heun': `trajectory` receives the state after every completed step (the VP latent zhat_{i+1}, which already holds
    step i+1's churn; the output last); the initial draw eps becomes zhat_0 = (sigma_0 eps + churn_0 eps_0) / a(sigma_hat_0),
    eps_0 = noise_fn(0, shape) drawn only when step 0 churns.
    `guidance_scale` s, `guidance_rescale` phi: classifier-free guidance.  s == 1.0 is the unguided
    path, untouched.  Any other finite s evaluates the U-Net on the conditioning and on the null conditioning (the
    all-zero latent) as ONE batch-2n evaluation inside the captured step, and feeds eps = m (eps_u + s (eps_c - eps_u)),
    m = phi std(eps_c) / std(eps_g) + 1 - phi per sample, to the unchanged update; trajectories and nonfinite counters
    report on that eps.  Not available with depth sharding (CtsiError).
    `diffusion.prediction_type == 'v_prediction'`: the model's output is v; one ctsi_pred_to_eps launch
    per evaluation turns it into eps ahead of the guidance and the update, so everything above holds as written.
    `diffusion.update_form == 'x0'` ('ddim', 'ddpm', 'dpmpp' of a v model): no conversion launch; the
    update is ctsi_x0_step on the raw v, which divides by nothing, so a zero-terminal-SNR schedule can be sampled.  The
    guidance then combines -- and its rescale takes the statistics of -- the raw v rows (with phi = 0 algebraically the
    guided eps; with phi > 0 the statistics of the model output, as Lin et al. define the rescale: a difference from the
    eps statistics of section 18), and `eps_trajectory` receives the (guided) raw v.  'heun' is not affected.
    Inside `with measurement_scope(MeasurementGuidance.bind(y, vae)):` (additive; the samplers'
    sample(measurement=) does it) the run is steered toward the thick volume y on the guidance's evaluations: 'ddim', 'ddpm',
    'dpmpp' on the engine's UNet3D in bf16, unsharded (CtsiError otherwise, before anything is drawn or built).  No scope, or
    a guidance of scale 0, leaves every launch as it is."""
    s_cfg, phi_cfg = check_guidance(guidance_scale, guidance_rescale)
    guided = s_cfg != 1.0
    measurement = _take_measurement()
    if measurement is not None and measurement.guidance.scale == 0.0:
        measurement = None
    if measurement is not None:
        from .measurement_guidance import refuse_unguidable_run
        refuse_unguidable_run(model, measurement.vae, getattr(model, "inference_precision", "bf16"), kind,
                              getattr(heun, "learned", False))
    plan = _step_plan(diffusion, kind, t_desc, eta, order, heun)
    if not _is_engine_unet(model) and not callable(model):
        raise CtsiError(f"the samplers need a model(z, t, c) callable; got {type(model).__name__}")
    unet = model
    if _is_engine_unet(model):
        check_attention_mode(unet.attention_mode)     # an unknown mode is an error before anything is drawn or built
        check_pairing(diffusion, unet)                # var_type and learn_sigma belong together
    device = torch.device(device)
    ctx = Ctx.get(device if device.type == "cuda" else conditioning.device)
    n, L, d, h, w = [int(v) for v in shape]
    nb = 2 * n if guided else n                 # rows of one U-Net evaluation
    max_rows = (diffusion.timesteps + 1) * nb
    comm = getattr(unet, "depth_shard_comm", None) if _is_engine_unet(model) else None
    if guided and comm is not None and comm.world > 1:
        raise CtsiError("classifier-free guidance (guidance_scale != 1.0) does not support depth sharding "
                        "(unet.depth_shard_comm): the sharded program holds one volume per rank and the rescale "
                        "statistics would need a collective; drop the communicator or sample unguided")
    # initial noise is drawn exactly where the reference draws it (on the caller's stream/generator)
    if z_init is not None:
        z0 = z_init
    elif noise_fn is not None:
        z0 = noise_fn(-1, tuple(shape)).to(ctx.device)
    else:
        z0 = torch.randn(tuple(shape), device=ctx.device)
    z0 = plan.initial_state(z0, noise_fn, shape, ctx.device)
    if not _is_engine_unet(model):
        return _run_generic(plan, model, shape, conditioning, ctx, z0, noise_fn=noise_fn, progress=progress,
                            trajectory=trajectory, eps_trajectory=eps_trajectory,
                            guidance=(s_cfg, phi_cfg) if guided else None)
    precision = check_precision(getattr(unet, "inference_precision", "bf16"))
    if comm is not None and comm.world > 1:
        check_resblock_options_unsharded(unet, True)
        check_learn_sigma_unsharded(unet, True)
        if precision != "bf16":
            raise CtsiError(f"the {precision} inference mode does not support depth sharding (unet.depth_shard_comm); "
                            "set inference_precision='bf16' or drop the communicator")
        if eps_trajectory is not None:
            raise CtsiError("eps_trajectory is not recorded by the depth-sharded sampler")
        return run_sampler_sharded(diffusion, unet, shape, conditioning, ctx, z0, kind=kind, t_desc=t_desc, eta=eta,
                                   noise_fn=noise_fn, comm=comm, trajectory=trajectory, order=order, heun=heun)
    with ctx.scope():
        # the unguided key is what it always was; a guided program (with or without the rescale statistics) has its own
        head = ("sampler-cfg", ctx.device.index, n, d, h, w, max_rows, phi_cfg > 0.0) if guided else (
            "sampler", ctx.device.index, n, d, h, w, max_rows)
        key = head + plan.key + (unet.attention_mode, precision) + plan.key_order
        from .engine import cached_program

        def build():
            cls = unet_program(precision)
            kw = dict(guided=True, rescale=phi_cfg > 0.0) if guided else {}
            if plan.pred is not None or plan.x0:
                kw["prediction"] = "v_prediction"
            prog = cls(ctx, unet, n, d, h, w, max_rows, unet.attention_mode, **kw)
            prog.add_sampler_step(plan.kind, plan.with_noise, **(dict(update_form="x0") if plan.x0 else {}),
                                  **(dict(learned_variance=True) if plan.learned else {}))
            return prog

        prog: UNetProgram = cached_program(unet, key, build)
        guide = None
        if measurement is not None:
            from .measurement_guidance import GuideRun
            guide = GuideRun(measurement, diffusion, plan, order, ctx, shape)
        return _run_step_program(prog, plan, ctx, shape, conditioning, z0, nb, noise_fn=noise_fn, progress=progress,
                                 guidance=(s_cfg, phi_cfg) if guided else None, trajectory=trajectory,
                                 eps_trajectory=eps_trajectory, guide=guide)


def check_fusable(diffusion, model, kind: str = "ddim", dp_group=None):
    """What latent window fusion refuses, before anything is drawn or built (CtsiError, each naming the alternative)."""
    if dp_group is not None and dp_group is not False:
        raise CtsiError("fusion='latent' does not support window data parallelism (dp_group=): every window is a row of one "
                        "network batch on one device; use fusion='pixel' to split the windows over ranks")
    if not _is_engine_unet(model):
        raise CtsiError("fusion='latent' needs the engine's UNet3D: the blend and the cut run inside its captured step; a "
                        "generic model(z, t, c) callable can be stitched with fusion='pixel'")
    comm = getattr(model, "depth_shard_comm", None)
    if comm is not None and getattr(comm, "world", 1) > 1:
        raise CtsiError("fusion='latent' does not support depth sharding (unet.depth_shard_comm): drop the communicator, or "
                        "use fusion='pixel'")
    learned = check_var_type(getattr(diffusion, "var_type", "fixed_small")) == "learned_range"
    if getattr(model, "learn_sigma", False) or learned or kind == "ddpm_lv":
        raise CtsiError("fusion='latent' does not support a learn_sigma model, var_type='learned_range' or the strided ancestral "
                        "sampler ('ddpm_spaced'): use the full-length DDPMSampler on a fixed_small model, DDIM, DPM-Solver++ "
                        "or Heun, or fusion='pixel'")


def run_sampler_fused(diffusion, unet, full_shape, cond_windows, win_shape, starts, device, *, kind: str, t_desc: Sequence,
                      eta: float = 0.0, noise_fn=None, order: int = 2, heun: Optional[HeunRows] = None,
                      guidance_scale: float = 1.0, guidance_rescale: float = 0.0, trajectory: Optional[list] = None,
                      eps_trajectory: Optional[list] = None, progress: bool = False):
    """run_sampler with latent window fusion: ONE latent of `full_shape` (B, L, D, H, W) for the whole
    volume; every U-Net evaluation runs on all windows -- `starts`: their latent (d, h, w) starts, a product grid in that
    order; `win_shape` (td, lh, lw); `cond_windows` (nw B, L, td, lh, lw): their conditioning latents, window-major, never
    blended -- as one batch (2 nw B rows when guided), the raw outputs are blended into a full-size prediction
    (ctsi_window_blend) and everything run_sampler puts behind the network -- ctsi_pred_to_eps, the guidance (its rescale
    statistics per full volume), the kind's update or ctsi_x0_step, the nonfinite counters -- runs unchanged at the full
    shape; ctsi_window_gather then cuts the new network input back into the windows.  One captured hipGraph per step.
    Noise: one draw of the full shape, noise_fn(-1, full_shape) / torch.randn for the start and noise_fn(i, full_shape) per
    noisy step.  Kinds 'ddim', 'ddpm', 'dpmpp', 'heun'.  `trajectory` / `eps_trajectory` receive full-shape fp32 NCDHW tensors,
    as in run_sampler.  Returns the full latent."""
    s_cfg, phi_cfg = check_guidance(guidance_scale, guidance_rescale)
    guided = s_cfg != 1.0
    check_fusable(diffusion, unet, kind)
    plan = _step_plan(diffusion, kind, t_desc, eta, order, heun)
    check_attention_mode(unet.attention_mode)
    check_pairing(diffusion, unet)
    precision = check_precision(getattr(unet, "inference_precision", "bf16"))
    ctx = Ctx.get(torch.device(device))
    n, L, D, H, W = [int(v) for v in full_shape]
    win = tuple(int(v) for v in win_shape)
    starts = [tuple(int(v) for v in s) for s in starts]
    nb_net = len(starts) * n * (2 if guided else 1)          # rows of one U-Net evaluation
    max_rows = (diffusion.timesteps + 1) * nb_net
    z0 = noise_fn(-1, tuple(full_shape)).to(ctx.device) if noise_fn is not None else torch.randn(tuple(full_shape),
                                                                                                  device=ctx.device)
    z0 = plan.initial_state(z0, noise_fn, full_shape, ctx.device)
    with ctx.scope():
        from .engine import cached_program
        key = ("sampler-fused", ctx.device.index, n, D, H, W, win, tuple(starts), max_rows, guided,
               phi_cfg > 0.0) + plan.key + (unet.attention_mode, precision) + plan.key_order

        def build():
            kw = dict(guided=True, rescale=phi_cfg > 0.0) if guided else {}
            if plan.pred is not None or plan.x0:
                kw["prediction"] = "v_prediction"
            prog = fused_program(precision)(ctx, unet, n, (D, H, W), win, starts, max_rows, unet.attention_mode, **kw)
            prog.add_sampler_step(plan.kind, plan.with_noise, **(dict(update_form="x0") if plan.x0 else {}))
            return prog

        prog = cached_program(unet, key, build)
        return _run_step_program(prog, plan, ctx, full_shape, cond_windows, z0, nb_net, noise_fn=noise_fn, progress=progress,
                                 guidance=(s_cfg, phi_cfg) if guided else None, trajectory=trajectory,
                                 eps_trajectory=eps_trajectory)


class _Sampler:
    """What the samplers share: the model pair, the DDIM timestep list, the blend window and the stitching driver."""

    def __init__(self, diffusion, model):
        self.diffusion = diffusion
        self.model = model
        self.timesteps = diffusion.timesteps
        # plain attribute: None or a consistency.DataConsistency; sample_with_stitching then projects the
        # full blended volume onto `v_thick_full` once (blending overlapping windows does not keep per-window consistency)
        self.data_consistency = None

    def _get_timesteps(self, num_inference_steps):
        """arange(0, T, T // N) plus T-1 when the stride misses it, descending — N+1 entries whenever
        T % N == 0 and N < T (sampler.py:221-239)."""
        stride = self.timesteps // num_inference_steps
        ts = np.arange(0, self.timesteps, stride)
        if ts[-1] != self.timesteps - 1:
            ts = np.append(ts, self.timesteps - 1)
        return ts[::-1]

    def _create_gaussian_weight(self, d, h, w):
        return gaussian_weight(d, h, w)

    def _stitch(self, v_thick_full, vae, num_inference_steps, patch_size, target_patch_size, stride, device, progress,
                window_batch, dp_group, batchable, fusion="pixel", decode=None, **kw):
        """sample_with_stitching on `num_inference_steps` steps (`kw`: more sample() arguments).  Windows are batched
        (up to `window_batch`; None / 0: as many as the device memory holds, see _stitched) only when `batchable`, i.e.
        when the sampler draws no noise after the initial latent.
        `fusion` 'latent' (`decode` 'full' | 'windows'): _stitched_fused on the run `_fused_plan` describes; there
        `window_batch` batches the window decode only."""
        fusion, decode = check_fusion(fusion, decode)
        s_cfg, phi_cfg = check_guidance(kw.get("guidance_scale", 1.0), kw.get("guidance_rescale", 0.0))
        if fusion == "latent":
            plan_kw = {k: v for k, v in kw.items() if k not in ("guidance_scale", "guidance_rescale")}
            return _stitched_fused(self, v_thick_full, vae, patch_size, target_patch_size, stride, device, progress,
                                   self._fused_plan(num_inference_steps, **plan_kw), decode, window_batch, dp_group,
                                   (s_cfg, phi_cfg))

        def sample(shp, cond, z_init=None):
            return self.sample(shp, cond, num_inference_steps, device, progress=False, z_init=z_init, **kw)

        if window_batch is None:
            window_batch = 0
        return _stitched(self, v_thick_full, vae, patch_size, target_patch_size, stride, device, progress, sample,
                         batched_fn=sample if batchable and window_batch != 1 else None, window_batch=window_batch,
                         dp_group=dp_group, guided=s_cfg != 1.0)


class DDPMSampler(_Sampler):
    """Ancestral sampling over all `diffusion.timesteps` steps (reference sampler.py:17-61), or -- additive, DESIGN section 24 --
    over the strided subset DDIMSampler walks (`num_inference_steps`), on the respaced chain of Improved DDPM."""

    def chain(self, num_inference_steps=None, clip_denoised=True):
        """(kind, timesteps) of a run: ('ddpm', T-1 .. 0), the reference's loop and rows, when the chain is full-length, clips
        and the variance is fixed-small; ('ddpm_lv', DDIM's timesteps) otherwise -- ctsi_ddpm_lv_step on respaced rows."""
        T = self.timesteps
        if num_inference_steps is not None and not 1 <= int(num_inference_steps) <= T:
            raise ValueError(f"num_inference_steps must lie in [1, {T}], got {num_inference_steps!r}")
        full = num_inference_steps is None or int(num_inference_steps) == T
        learned = check_var_type(getattr(self.diffusion, "var_type", "fixed_small")) == "learned_range"
        t_desc = list(reversed(range(T))) if full else [int(t) for t in self._get_timesteps(int(num_inference_steps))]
        return ("ddpm" if full and clip_denoised and not learned else "ddpm_lv"), t_desc

    def _fused_plan(self, num_inference_steps=None, clip_denoised=True) -> dict:
        kind, chain = self.chain(num_inference_steps, clip_denoised)
        return dict(kind=kind, t_desc=chain)

    def coef_rows(self, num_inference_steps=None, clip_denoised=True) -> torch.Tensor:
        """The update's coefficient rows for such a run (what the step program reads)."""
        kind, t_desc = self.chain(num_inference_steps, clip_denoised)
        rows = lv_rows(self.diffusion, t_desc, clip_denoised) if kind == "ddpm_lv" else None
        return _step_plan(self.diffusion, kind, t_desc, 0.0, 2, rows).coef

    @torch.no_grad()
    def sample(self, shape, conditioning, device, progress=True, noise_fn=None, num_steps=None,
               trajectory=None, guidance_scale=1.0, guidance_rescale=0.0, num_inference_steps=None, clip_denoised=True,
               measurement=None):
        """`num_inference_steps` N (additive; None or T: every step, as ever): the N-step strided ancestral sampler.  The
        timesteps are DDIMSampler's for N; the network is evaluated at the original timesteps and the update runs on the
        respaced chain beta'_i = 1 - abar_{S_i} / abar_{S_{i-1}} with its own posterior coefficients and variances
        (learned_sigma.respaced_ddpm_rows) -- the fixed-small beta~' or, under var_type='learned_range', the model's.
        `clip_denoised=False` (additive) drops the clamp of the predicted z_0 to [-1, 1].  `num_steps`: a prefix (test hook)."""
        kind, chain = self.chain(num_inference_steps, clip_denoised)
        rows = dict(heun=lv_rows(self.diffusion, chain, clip_denoised)) if kind == "ddpm_lv" else {}
        with measurement_scope(measurement) if measurement is not None else contextlib.nullcontext():
            return run_sampler(self.diffusion, self.model, shape, conditioning, device, kind=kind, t_desc=chain[:num_steps],
                               progress=progress, noise_fn=noise_fn, trajectory=trajectory,
                               guidance_scale=guidance_scale, guidance_rescale=guidance_rescale, **rows)

    @torch.no_grad()
    def sample_with_stitching(self, v_thick_full, vae, patch_size=(8, 192, 192),
                              target_patch_size=(48, 192, 192), stride=(4, 96, 96), device='cuda',
                              progress=True, dp_group=None, guidance_scale=1.0, guidance_rescale=0.0,
                              num_inference_steps=None, clip_denoised=True, fusion='pixel', decode=None):
        """`fusion`, `decode`: as in DDIMSampler.sample_with_stitching; fusion='latent' runs the full-length chain of a
        fixed_small model only (the strided / learned-variance step 'ddpm_lv' is refused)."""
        fusion, decode = check_fusion(fusion, decode)
        s_cfg, phi_cfg = check_guidance(guidance_scale, guidance_rescale)
        if fusion == "latent":
            return _stitched_fused(self, v_thick_full, vae, patch_size, target_patch_size, stride, device, progress,
                                   self._fused_plan(num_inference_steps, clip_denoised=clip_denoised), decode, 0, dp_group,
                                   (s_cfg, phi_cfg))
        kw = {} if num_inference_steps is None and clip_denoised else dict(num_inference_steps=num_inference_steps,
                                                                          clip_denoised=clip_denoised)
        return _stitched(self, v_thick_full, vae, patch_size, target_patch_size, stride, device, progress,
                         lambda shp, cond: self.sample(shp, cond, device, progress=False,
                                                       guidance_scale=guidance_scale,
                                                       guidance_rescale=guidance_rescale, **kw), dp_group=dp_group)


class DDIMSampler(_Sampler):
    """Deterministic (eta = 0) or stochastic DDIM over a strided timestep subset (sampler.py:201-336)."""

    @torch.no_grad()
    def sample(self, shape, conditioning, num_inference_steps, device, eta=0.0, progress=True, noise_fn=None,
               trajectory=None, z_init=None, guidance_scale=1.0, guidance_rescale=0.0, measurement=None):
        t_desc = [int(t) for t in self._get_timesteps(num_inference_steps)]
        with measurement_scope(measurement) if measurement is not None else contextlib.nullcontext():
            return run_sampler(self.diffusion, self.model, shape, conditioning, device, kind="ddim", t_desc=t_desc,
                               progress=progress, eta=float(eta), noise_fn=noise_fn, trajectory=trajectory, z_init=z_init,
                               guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)

    @torch.no_grad()
    def sample_with_stitching(self, v_thick_full, vae, num_inference_steps=20, patch_size=(8, 192, 192),
                              target_patch_size=(48, 192, 192), stride=(4, 96, 96), device='cuda', eta=0.0,
                              progress=True, window_batch=None, dp_group=None, guidance_scale=1.0,
                              guidance_rescale=0.0, fusion='pixel', decode=None):
        """`dp_group` (additive kwarg, default None = every window on this process, as in the reference): a
        torch.distributed process group (or True for the default group) over which the windows are split; every rank
        of the group must make the call with the SAME volume.
        `window_batch` (additive kwarg): windows are independent, so for the deterministic sampler (eta == 0) up to
        that many are encoded / sampled / decoded as one batch -- a single 192x192 patch leaves most of an MI355X
        idle (its coarsest level has 28 conv tiles for 256 CUs).  None / 0 (default): as many as a fifth of the device
        memory holds (13 windows of 48 x 192 x 192 on a 288 GB part); 1: one by one, like the reference.  The initial noise of every window is still drawn
        with its own `torch.randn` call in window order, exactly as the reference's one-by-one loop draws it.
        `guidance_scale`, `guidance_rescale` (additive kwargs): classifier-free guidance of every window (run_sampler); a
        guided window counts as two in the automatic `window_batch`.
        `fusion` (additive kwarg): 'pixel' (default) is the path described above, every window an independent sample whose
        decoded pixels are blended.  'latent'  keeps ONE latent for the whole volume: every U-Net evaluation
        runs on all windows as one batch and their outputs are blended in latent space before the sampler update, so the
        windows share one trajectory and the result is one coherent sample; noise is drawn once at the full latent's shape.
        `decode` (with fusion='latent' only): 'full' (default) decodes the fused latent in one piece; 'windows' decodes its
        windows in batches of `window_batch` and blends the pixels, for a VAE that should only see training-size inputs.
        fusion='latent' refuses (CtsiError) dp_group, depth sharding, a learn_sigma model and a generic model callable."""
        return self._stitch(v_thick_full, vae, num_inference_steps, patch_size, target_patch_size, stride, device,
                            progress, window_batch, dp_group, float(eta) == 0.0, fusion, decode, eta=eta,
                            guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)

    def _fused_plan(self, num_inference_steps, eta=0.0) -> dict:
        return dict(kind="ddim", t_desc=[int(t) for t in self._get_timesteps(num_inference_steps)], eta=float(eta))


class DPMSolverSampler(_Sampler):
    """DPM-Solver++(2M) (Lu et al. 2022): the training-free multistep ODE solver in data prediction, on the DDIM
    timestep list (N steps = the same N + 1 U-Net evaluations as DDIM-N).  Additive: the reference has no such sampler.
    order=1 is the DDIM (eta = 0) update written in data-prediction form.  Deterministic: no noise is drawn after the
    initial latent."""

    def __init__(self, diffusion, model, order=2):
        if order not in (1, 2):
            raise ValueError(f"DPM-Solver++ order must be 1 or 2, got {order}")
        super().__init__(diffusion, model)
        self.order = int(order)

    @torch.no_grad()
    def sample(self, shape, conditioning, num_inference_steps, device, progress=True, noise_fn=None, trajectory=None,
               z_init=None, guidance_scale=1.0, guidance_rescale=0.0, measurement=None):
        t_desc = [int(t) for t in self._get_timesteps(num_inference_steps)]
        with measurement_scope(measurement) if measurement is not None else contextlib.nullcontext():
            return run_sampler(self.diffusion, self.model, shape, conditioning, device, kind="dpmpp", t_desc=t_desc,
                               progress=progress, noise_fn=noise_fn, trajectory=trajectory, z_init=z_init,
                               order=self.order, guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)

    @torch.no_grad()
    def sample_with_stitching(self, v_thick_full, vae, num_inference_steps=20, patch_size=(8, 192, 192),
                              target_patch_size=(48, 192, 192), stride=(4, 96, 96), device='cuda', progress=True,
                              window_batch=None, dp_group=None, guidance_scale=1.0, guidance_rescale=0.0,
                              fusion='pixel', decode=None):
        """DDIMSampler.sample_with_stitching without `eta`: the same windows, blend, `window_batch`, `dp_group`, guidance,
        `fusion` and `decode` behaviour (the solver is deterministic, so windows are always batchable)."""
        return self._stitch(v_thick_full, vae, num_inference_steps, patch_size, target_patch_size, stride, device,
                            progress, window_batch, dp_group, True, fusion, decode, guidance_scale=guidance_scale,
                            guidance_rescale=guidance_rescale)

    def _fused_plan(self, num_inference_steps) -> dict:
        return dict(kind="dpmpp", t_desc=[int(t) for t in self._get_timesteps(num_inference_steps)], order=self.order)


class HeunSampler(_Sampler):
    """EDM sampling (Karras et al. 2022, Algorithm 2): second-order Heun (order=2, 2N - 1 U-Net evaluations) or Euler
    (order=1, N evaluations) steps on freely chosen noise levels -- by default the rho-schedule between sigma_min and
    sigma_max -- with optional stochastic churn.  The U-Net sees the VP latent x / a(sigma) at the fractional timestep
    t(sigma) (sigma_to_t).  Additive: the reference's EDMSampler is an unimplemented stub (kept as is).
    Defaults follow the paper clamped to the model's range: sigma_min = max(0.002, sigma_0), sigma_max = min(80,
    sigma_{T-1}), rho = 7.  Noise: eps from z_init / noise_fn(-1, shape) / torch.randn, then eps_i = noise_fn(i, shape)
    (else torch.randn) only for the steps that churn (gamma_i > 0).
    `diffusion.update_form` does not affect this sampler: it evaluates finite noise levels only, so its eps-form rows and
    kernels stay.  On a zero-terminal-SNR schedule (sigma_{T-1} = inf) the default sigma_max is the largest finite table
    entry, sigma_{T-2}, and t(sigma) lies in [0, T-2]; an explicit infinite sigma_max is a ValueError as before."""

    def __init__(self, diffusion, model, order=2, sigma_min=None, sigma_max=None, rho=7.0, s_churn=0.0, s_tmin=0.0,
                 s_tmax=float("inf"), s_noise=1.0):
        if order not in (1, 2):
            raise ValueError(f"the EDM sampler's order must be 1 (Euler) or 2 (Heun), got {order}")
        super().__init__(diffusion, model)
        self.order = int(order)
        table = sigma_table(diffusion.alphas_cumprod)
        self.sigma_min = float(max(0.002, table[0]) if sigma_min is None else sigma_min)
        if sigma_max is None and not np.isfinite(table[-1]):      # a zero-terminal-SNR schedule: the largest finite level
            sigma_max = table[-2]
        self.sigma_max = float(min(80.0, table[-1]) if sigma_max is None else sigma_max)
        self.rho = float(rho)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = float(s_churn), float(s_tmin), float(s_tmax), float(s_noise)

    def sigmas(self, num_inference_steps) -> np.ndarray:
        """The default schedule: N levels from sigma_max down to sigma_min, then 0 (float64)."""
        return karras_sigmas(num_inference_steps, self.sigma_min, self.sigma_max, self.rho)

    def coef_rows(self, num_inference_steps=None, sigmas=None) -> HeunRows:
        if sigmas is None:
            if num_inference_steps is None:
                raise ValueError("give num_inference_steps or sigmas")
            sigmas = self.sigmas(num_inference_steps)
        return heun_coef_rows(self.diffusion.alphas_cumprod, sigmas, self.order, self.s_churn, self.s_tmin, self.s_tmax,
                              self.s_noise)

    @torch.no_grad()
    def sample(self, shape, conditioning, num_inference_steps, device, progress=True, noise_fn=None, trajectory=None,
               z_init=None, sigmas=None, guidance_scale=1.0, guidance_rescale=0.0):
        """`sigmas` (optional): explicit descending noise levels (a trailing 0 is appended when missing); they override
        the schedule and num_inference_steps."""
        rows = self.coef_rows(num_inference_steps, sigmas)
        return run_sampler(self.diffusion, self.model, shape, conditioning, device, kind="heun", t_desc=list(rows.t),
                           progress=progress, noise_fn=noise_fn, trajectory=trajectory, z_init=z_init,
                           order=self.order, heun=rows, guidance_scale=guidance_scale,
                           guidance_rescale=guidance_rescale)

    @torch.no_grad()
    def sample_with_stitching(self, v_thick_full, vae, num_inference_steps=20, patch_size=(8, 192, 192),
                              target_patch_size=(48, 192, 192), stride=(4, 96, 96), device='cuda', progress=True,
                              window_batch=None, dp_group=None, guidance_scale=1.0, guidance_rescale=0.0,
                              fusion='pixel', decode=None):
        """DDIMSampler.sample_with_stitching without `eta`: windows are batched when s_churn == 0 and run one by one
        otherwise (each window then draws its own churn noise, as stochastic DDIM does).  `fusion`, `decode`: as there (the
        churn noise of a fused run is one draw of the full latent's shape per churning step)."""
        return self._stitch(v_thick_full, vae, num_inference_steps, patch_size, target_patch_size, stride, device,
                            progress, window_batch, dp_group, self.s_churn == 0.0, fusion, decode,
                            guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)

    def _fused_plan(self, num_inference_steps) -> dict:
        rows = self.coef_rows(num_inference_steps)
        return dict(kind="heun", t_desc=list(rows.t), order=self.order, heun=rows)


# generate() / generate_batch() sampler names -> how each samples a latent: (diffusion, model, shape, conditioning,
# num_inference_steps, device, **sample kwargs).  'ddpm' runs all T steps: it ignores the step count; 'ddpm_spaced' honours it.
SAMPLERS = {
    'ddim': lambda df, m, shape, c, n, dev, **kw: DDIMSampler(df, m).sample(shape, c, n, dev, **kw),
    'ddpm': lambda df, m, shape, c, n, dev, **kw: DDPMSampler(df, m).sample(shape, c, dev, **kw),
    'ddpm_spaced': lambda df, m, shape, c, n, dev, **kw: DDPMSampler(df, m).sample(shape, c, dev, num_inference_steps=n, **kw),
    'dpmpp_2m': lambda df, m, shape, c, n, dev, **kw: DPMSolverSampler(df, m, order=2).sample(shape, c, n, dev, **kw),
    'heun': lambda df, m, shape, c, n, dev, **kw: HeunSampler(df, m).sample(shape, c, n, dev, **kw),
}


def gaussian_weight(d: int, h: int, w: int) -> torch.Tensor:
    """Separable blend window, sigma = size/6, centred at (n-1)/2 (sampler.py:174-198)."""
    return _axis_window(d)[:, None, None] * _axis_window(h)[None, :, None] * _axis_window(w)[None, None, :]


def _window_starts(full: int, size: int, step: int):
    return sorted(set(list(range(0, full - size + 1, step)) + [max(0, full - size)]))


def _axis_window(n: int) -> torch.Tensor:
    x = torch.arange(n).float() - (n - 1) / 2
    return torch.exp(-(x ** 2) / (2 * (n / 6) ** 2))


def _window_partition(windows, dp_group, sampler):
    """Which windows this process computes: all of them unless `dp_group` opts in to window data parallelism.
    Returns (my_windows, world, group)."""
    rank, world, group = 0, 1, None
    if dp_group is not None and dp_group is not False:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise CtsiError("sample_with_stitching(dp_group=...) needs an initialised torch.distributed process group")
        comm = getattr(getattr(sampler, "model", None), "depth_shard_comm", None)
        if comm is not None and getattr(comm, "world", 1) > 1:
            raise CtsiError("window data parallelism (dp_group=) cannot be combined with depth sharding "
                            "(unet.depth_shard_comm): depth-sharded ranks must all run the same window")
        group = None if dp_group is True else dp_group
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    from .parallel import shard_units
    return [windows[i] for i in shard_units(len(windows), rank, world)], world, group


def _auto_window_batch(ctx, vae, b, td, th, tw, nwin, guided=False) -> int:
    """sample_with_stitching's window batch when the caller names none."""
    # as many windows per batch as a fifth of the DEVICE memory holds: the VAE decoder is the largest program, ~2.5 KB of
    # activations per output voxel (30 GB for a 48 x 512 x 512 volume, 4.4 GB per 48 x 192 x 192 window: 13 windows on a
    # 288 GB part).  Measured on 25 windows: 13 per batch 1.69 s, all 25 at once 1.72 s, 5 per batch 1.98 s -- past a dozen
    # windows the levels are full and more only costs memory.  The TOTAL memory (not the free memory of the moment) keeps
    # the batch shape, and with it the cached programs, the same from call to call.
    try:
        total = torch.cuda.get_device_properties(ctx.device).total_memory
    except Exception:
        total = 64 << 30
    per_window = 2500.0 * b * td * th * tw
    # fp32 activations (the fp32 and bf16x3 modes): twice the bytes per voxel
    per_window *= ACT_BYTES.get(getattr(vae, "inference_precision", "bf16"), 2) / 2.0
    if guided:
        per_window *= 2.0         # a guided window is two rows of the U-Net's batch
    return max(1, min(nwin, int(0.2 * total / per_window)))


def _stitch_consistency(sampler, vae, patch_size, target_patch_size):
    """The sampler's `data_consistency` attribute, checked before anything is sampled: ValueError for a wrong type or a target
    patch shallower than the thick one, CtsiError under depth sharding."""
    dc = check_data_consistency(getattr(sampler, "data_consistency", None))
    if dc is not None:
        refuse_depth_sharding(getattr(sampler, "model", None), vae)
        if target_patch_size[0] < patch_size[0]:
            raise ValueError(f"data_consistency: target patch depth {target_patch_size[0]} is below the thick patch depth "
                             f"{patch_size[0]}; a slice profile maps thin slices onto fewer thick ones")
    return dc


def _consistent(sampler, dc, volume: torch.Tensor, v_thick_full: torch.Tensor) -> torch.Tensor:
    """The full stitched volume projected once onto the thick volume, with the profile of the full depths."""
    if dc is None:
        return volume
    if volume.shape[2] == v_thick_full.shape[2]:
        if not getattr(sampler, "_consistency_warned", False):      # once per sampler object, as generate() does per model
            sampler._consistency_warned = True
            logger.warning("data_consistency is set but the stitched volume keeps the depth (%d slices): there is nothing "
                           "to project, the attribute has no effect", int(volume.shape[2]))
        return volume
    return dc.project_(volume.contiguous(), v_thick_full.float())


def _stitched(sampler, v_thick_full, vae, patch_size, target_patch_size, stride, device, progress, sample_fn,
              batched_fn=None, window_batch=1, dp_group=None, guided=False):
    """Sliding-window inference (sampler.py:63-172, 338-453): per window encode -> sample -> decode on the
    engine, Gaussian-weighted accumulation (ctsi_blend_accumulate) and final normalisation
    (ctsi_blend_normalize) on device.

    depth_ratio == 1 reproduces the reference exactly (pinned by tests/golden 'stitch.tiny.out').  For
    depth_ratio != 1 the reference samples the latent at the *thick* patch depth and then fails with a shape
    mismatch when it adds the decoded patch to the thin accumulator; here the window's
    conditioning latent is upsampled along depth to the target depth first, exactly as
    VideoToVideoDiffusion.generate does for a whole volume (models/model.py:284-289), so every window
    produces a (target_d, h, w) patch that lands at depth int(d_start * depth_ratio).
    Window data parallelism is OPT-IN (`dp_group=`): by default every window is computed by the calling process,
    whatever the state of torch.distributed -- the reference's behaviour, and the only safe one when ranks validate
    different volumes or only rank 0 calls.  With `dp_group` (a process group, or True for the default group) the
    windows are data-parallel units (parallel.shard_units): every rank of the group must call with the same volume,
    blends its share, and the accumulators are all-reduced over that group before normalisation.  It cannot be
    combined with depth sharding (`unet.depth_shard_comm`): there every rank must run the same window."""
    dc = _stitch_consistency(sampler, vae, patch_size, target_patch_size)
    b, c, d_thick, hf, wf = v_thick_full.shape
    pd, ph, pw = patch_size
    td, th, tw = target_patch_size
    if (th, tw) != (ph, pw):
        raise CtsiError(f"sample_with_stitching: target patch (h, w)=({th},{tw}) must equal the thick patch "
                        f"(h, w)=({ph},{pw}); only depth is interpolated")
    ratio = td / pd
    d_thin = int(d_thick * ratio)
    dev = torch.device(device)
    ctx = Ctx.get(dev)
    lib, sptr = ctx.lib, ctx.sptr
    acc = torch.zeros(b, c, d_thin, hf, wf, device=ctx.device)
    wsum = torch.zeros(b, c, d_thin, hf, wf, device=ctx.device)
    wd, wh, ww = (_axis_window(n).to(ctx.device) for n in (td, th, tw))
    windows = [(ds, hs, ws) for ds in _window_starts(d_thick, pd, stride[0])
               for hs in _window_starts(hf, ph, stride[1]) for ws in _window_starts(wf, pw, stride[2])]
    mine, world, pg = _window_partition(windows, dp_group, sampler)
    it = None
    if progress and tqdm is not None:
        it = tqdm(desc="Patch-based inference", total=len(mine))
    group = 1
    if batched_fn is not None:
        group = int(window_batch)
        if group <= 0:
            group = _auto_window_batch(ctx, vae, b, td, th, tw, len(mine), guided)
    ngroups = max(1, -(-len(mine) // group))            # balanced groups: 25 windows, window_batch 8 -> 7 + 6 + 6 + 6
    bounds = [round(i * len(mine) / ngroups) for i in range(ngroups + 1)]
    for gi in range(ngroups):
        wins = mine[bounds[gi]:bounds[gi + 1]]
        if not wins:
            continue
        patch = torch.cat([v_thick_full[:, :, ds:ds + pd, hs:hs + ph, ws:ws + pw] for (ds, hs, ws) in wins], dim=0)
        z_cond = vae.encode(patch.to(ctx.device).contiguous())
        if td != pd:
            with ctx.scope():
                z_cond = trilinear_depth(ctx, z_cond, td)
        if len(wins) == 1 or batched_fn is None:
            z = sample_fn(tuple(z_cond.shape), z_cond)
        else:   # one torch.randn per window, in window order (the reference's RNG stream)
            one = (b,) + tuple(z_cond.shape[1:])
            z_init = torch.cat([torch.randn(one, device=ctx.device) for _ in wins], dim=0)
            z = batched_fn(tuple(z_cond.shape), z_cond, z_init)
        out = vae.decode(z).contiguous()
        with ctx.scope():
            for k, (ds, hs, ws) in enumerate(wins):
                ok = out[k * b:(k + 1) * b]
                lib.blend_accumulate(_ptr(acc), _ptr(wsum), _ptr(ok), _ptr(wd), _ptr(wh), _ptr(ww), b * c, td, th, tw,
                                     d_thin, hf, wf, int(ds * ratio), hs, ws, sptr)
        if progress and tqdm is not None:
            it.update(len(wins))
    if it is not None:
        it.close()
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(acc, group=pg)
        dist.all_reduce(wsum, group=pg)
    with ctx.scope():
        lib.blend_normalize(_ptr(acc), _ptr(wsum), acc.numel(), sptr)
    return _consistent(sampler, dc, acc, v_thick_full)


def _stitched_fused(sampler, v_thick_full, vae, patch_size, target_patch_size, stride, device, progress, plan_args, decode,
                    window_batch=0, dp_group=None, guidance=(1.0, 0.0)):
    """sample_with_stitching(fusion='latent'): the windows of _stitched, fused in latent space.  Every thick
    window is encoded on its own, in window batches, and depth-upsampled exactly as _stitched does it; run_sampler_fused then
    samples ONE latent of the whole target volume with `plan_args` (the sampler's kind, timesteps and settings).
    `decode` 'full': one vae.decode of that latent; 'windows': its windows are decoded in batches of `window_batch` (None / 0:
    automatic, as in _stitched) and the pixels blended with ctsi_blend_accumulate / ctsi_blend_normalize, for VAEs that
    should only ever see training-size inputs.  All windows are one network batch: there is no chunking, and a volume whose
    window batch does not fit raises torch's out-of-memory error."""
    check_fusable(sampler.diffusion, sampler.model, plan_args["kind"], dp_group)
    dc = _stitch_consistency(sampler, vae, patch_size, target_patch_size)
    window_batch = int(window_batch or 0)
    if decode == "full" and window_batch != 0:
        raise CtsiError(f"window_batch={window_batch} with decode='full': the fused latent is decoded in one piece and all "
                        "windows are one network batch; drop window_batch, or pass decode='windows' to decode window by window")
    b, c, d_thick, hf, wf = v_thick_full.shape
    pd, ph, pw = patch_size
    td, th, tw = target_patch_size
    if (th, tw) != (ph, pw):
        raise CtsiError(f"sample_with_stitching: target patch (h, w)=({th},{tw}) must equal the thick patch "
                        f"(h, w)=({ph},{pw}); only depth is interpolated")
    geo = stitch_geometry(vae, v_thick_full.shape, patch_size, target_patch_size, stride)
    ctx = Ctx.get(torch.device(device))
    nwin = len(geo.pixel_windows)
    auto = _auto_window_batch(ctx, vae, b, td, th, tw, nwin)
    conds = []
    for lo in range(0, nwin, auto):
        wins = geo.pixel_windows[lo:lo + auto]
        patch = torch.cat([v_thick_full[:, :, ds:ds + pd, hs:hs + ph, ws:ws + pw] for (ds, hs, ws) in wins], dim=0)
        z_cond = vae.encode(patch.to(ctx.device).contiguous())
        if td != pd:
            with ctx.scope():
                z_cond = trilinear_depth(ctx, z_cond, td)
        conds.append(z_cond)
    cond = conds[0] if len(conds) == 1 else torch.cat(conds, dim=0)
    L = int(cond.shape[1])
    z = run_sampler_fused(sampler.diffusion, sampler.model, (b, L) + geo.full, cond, geo.win, geo.starts, ctx.device,
                          guidance_scale=guidance[0], guidance_rescale=guidance[1], progress=progress, **plan_args)
    if decode == "full":
        return _consistent(sampler, dc, vae.decode(z), v_thick_full)
    lib, sptr = ctx.lib, ctx.sptr
    d_thin = geo.full[0]
    acc = torch.zeros(b, c, d_thin, hf, wf, device=ctx.device)
    wsum = torch.zeros(b, c, d_thin, hf, wf, device=ctx.device)
    wd, wh, ww = (_axis_window(n).to(ctx.device) for n in (td, th, tw))
    group = window_batch if window_batch > 0 else auto
    f, (ld, lh, lw) = geo.factor, geo.win
    for lo in range(0, nwin, group):
        sts = geo.starts[lo:lo + group]
        out = vae.decode(torch.cat([z[:, :, sd:sd + ld, sh:sh + lh, sw:sw + lw] for (sd, sh, sw) in sts], dim=0)
                         .contiguous()).contiguous()
        with ctx.scope():
            for k, (sd, sh, sw) in enumerate(sts):
                ok = out[k * b:(k + 1) * b]
                lib.blend_accumulate(_ptr(acc), _ptr(wsum), _ptr(ok), _ptr(wd), _ptr(wh), _ptr(ww), b * c, td, th, tw,
                                     d_thin, hf, wf, sd, sh * f, sw * f, sptr)
    with ctx.scope():
        lib.blend_normalize(_ptr(acc), _ptr(wsum), acc.numel(), sptr)
    return _consistent(sampler, dc, acc, v_thick_full)


class EDMSampler:
    def __init__(self, diffusion, model):
        self.diffusion = diffusion
        self.model = model
        raise NotImplementedError("EDM sampler not yet implemented")
