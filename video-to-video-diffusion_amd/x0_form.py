"""x0-form sampler updates and the zero-terminal-SNR schedule (Lin et al. 2024, "Common diffusion noise
schedules and sample steps are flawed").

An eps-form update recovers z_0 = (z - sigma eps) / alpha, alpha = sqrt(abar): at the first step of the default cosine
schedule alpha = 1.6e-5, so the division multiplies every rounding of the network output by 6e4, and at alpha = 0 -- the last
step of a zero-terminal-SNR schedule -- it has no value at all.  A v-prediction model needs no division:

    z_0 = alpha z - sigma v,        z' = (sigma'/sigma) z + (alpha' - alpha sigma'/sigma) z_0.

This module holds the switches' validation (GaussianDiffusion.update_form, .loss_weighting), the schedule rescale in
float64, the coefficient rows of the three x0-form updates, and the one launch an x0 step program adds, ctsi_x0_step
(csrc/x0_step.hip), which reads the network's raw v: such a program has no ctsi_pred_to_eps launch."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Sequence

import numpy as np
import torch

UPDATE_FORMS = ("eps", "x0")
LOSS_WEIGHTINGS = ("min_snr", "uniform")
BUFFERS = ("betas", "alphas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
           "sqrt_one_minus_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1",
           "posterior_mean_coef2")


def check_update_form(form, prediction_type) -> str:
    """Validate an update_form value ('eps' | 'x0') against the prediction type: an epsilon output cannot give z_0 without
    the division, so 'x0' needs 'v_prediction'.  Raises ValueError otherwise."""
    if not isinstance(form, str) or form not in UPDATE_FORMS:
        raise ValueError(f"unknown update_form {form!r}: expected one of {UPDATE_FORMS}")
    if form == "x0" and prediction_type != "v_prediction":
        raise ValueError(f"update_form 'x0' requires prediction_type 'v_prediction', got {prediction_type!r}: an "
                         "'epsilon' output gives z_0 only through the division by sqrt(alphas_cumprod)")
    return form


def check_loss_weighting(w) -> str:
    """Validate a loss_weighting value ('min_snr' | 'uniform'); raises ValueError otherwise."""
    if not isinstance(w, str) or w not in LOSS_WEIGHTINGS:
        raise ValueError(f"unknown loss_weighting {w!r}: expected one of {LOSS_WEIGHTINGS}")
    return w


def check_eps_form_timesteps(alphas_cumprod: torch.Tensor, timesteps: Sequence[int]):
    """The guard of every 'eps'-form evaluation: a timestep whose alphas_cumprod is 0 (the last one of a zero-terminal-SNR
    schedule) has no eps-form update -- a ValueError that names it, never a NaN."""
    idx = torch.as_tensor([int(t) for t in timesteps], dtype=torch.long)
    bad = idx[alphas_cumprod.detach().cpu()[idx] == 0]
    if bad.numel():
        raise ValueError(f"timestep {int(bad[0])} has alphas_cumprod == 0 (a zero-terminal-SNR schedule): the 'eps' update "
                         "form divides by sqrt(alphas_cumprod) there; set update_form='x0' (it needs "
                         "prediction_type='v_prediction') or call rescale_zero_terminal_snr()")


def rescaled_schedule(alphas_cumprod: torch.Tensor) -> dict:
    """Algorithm 1 of Lin et al. on the schedule `alphas_cumprod`, in float64: s = sqrt(abar), s <- (s - s_T) s_0 / (s_0 -
    s_T), abar = s^2, alpha_t = abar_t / abar_{t-1}, beta = 1 - alpha (no clip: beta_{T-1} = 1), and the ten buffers of
    GaussianDiffusion recomputed from them.  Returns name -> float64 tensor."""
    ab0 = alphas_cumprod.detach().double().cpu().numpy()
    s = np.sqrt(ab0)
    s0, sT = s[0], s[-1]
    s = (s - sT) * s0 / (s0 - sT)
    abar = s * s
    abar_prev = np.concatenate([[1.0], abar[:-1]])
    alphas = abar / abar_prev
    betas = 1.0 - alphas
    post_var = betas * (1.0 - abar_prev) / (1.0 - abar)
    out = dict(betas=betas, alphas=alphas, alphas_cumprod=abar, alphas_cumprod_prev=abar_prev,
               sqrt_alphas_cumprod=np.sqrt(abar), sqrt_one_minus_alphas_cumprod=np.sqrt(1.0 - abar),
               posterior_variance=post_var, posterior_log_variance_clipped=np.log(np.maximum(post_var, 1e-20)),
               posterior_mean_coef1=betas * np.sqrt(abar_prev) / (1.0 - abar),
               posterior_mean_coef2=(1.0 - abar_prev) * np.sqrt(alphas) / (1.0 - abar))
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def x0_coef_rows(diffusion, kind: str, t_desc: Sequence[int], eta: float = 0.0, order: int = 2,
                 dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Coefficient rows {alpha, sigma, a, b, c, s, clip, 0} of ctsi_x0_step for sampler `kind` on the timestep list `t_desc`,
    in float64 from `alphas_cumprod`, rounded once to `dtype`.  With alpha, sigma at t and alpha', sigma' at the next
    timestep (1, 0 after the last):
      'ddim'   a = sigma'/sigma,  b = alpha' - alpha a,  s = eta sqrt((1 - abar')/(1 - abar) (1 - abar/abar')),  clip 10
               (the reference's update without its 1e-8 terms, which guard divisions this form does not have; as there, the
               direction term is not reduced by s^2)
      'ddpm'   a = posterior_mean_coef2,  b = posterior_mean_coef1,  s = [t != 0] exp(logvar / 2),  clip 1   (the buffers)
      'dpmpp'  a, b, c = columns 2..4 of sampler.dpm_coef_rows,  clip 10,  hist = the previous data prediction."""
    from .sampler import dpm_coef_rows
    idx = [int(t) for t in t_desc]
    n = len(idx)
    ac = diffusion.alphas_cumprod.detach().double().cpu().numpy()
    abar = ac[idx]
    rows = np.zeros((n, 8), dtype=np.float64)
    rows[:, 0], rows[:, 1] = np.sqrt(abar), np.sqrt(1.0 - abar)
    if kind == "ddim":
        abar_n = np.append(abar[1:], 1.0)
        a = np.sqrt(1.0 - abar_n) / rows[:, 1]
        rows[:, 2] = a
        rows[:, 3] = np.sqrt(abar_n) - rows[:, 0] * a
        if eta > 0:
            rows[:, 5] = eta * np.sqrt((1.0 - abar_n) / (1.0 - abar) * (1.0 - abar / abar_n))
        rows[:, 6] = 10.0
    elif kind == "ddpm":
        buf = lambda name: getattr(diffusion, name).detach().double().cpu().numpy()[idx]
        rows[:, 2] = buf("posterior_mean_coef2")
        rows[:, 3] = buf("posterior_mean_coef1")
        rows[:, 5] = (np.asarray(idx) != 0) * np.exp(0.5 * buf("posterior_log_variance_clipped"))
        rows[:, 6] = 1.0
    elif kind == "dpmpp":
        with np.errstate(divide="ignore", invalid="ignore"):     # lambda = -inf at abar = 0: only the unused columns are inf
            rows[:, 2:5] = dpm_coef_rows(diffusion.alphas_cumprod, idx, order, torch.float64)[:, 2:5].numpy()
        rows[:, 6] = 10.0
    else:
        raise ValueError(f"no x0-form update for sampler kind {kind!r}: expected 'ddim', 'ddpm' or 'dpmpp'")
    return torch.from_numpy(rows).to(dtype)


def x0_step_launcher(lib, f32: bool) -> Callable:
    """ctsi_x0_step / ctsi_x0_step_f32 behind the argument list of engine.sampler_step_launcher."""
    fn = lib.x0_step_f32 if f32 else lib.x0_step

    def launch(z, v, hist, noise, zin, c_total, coef, step_ptr, n, L, d, h, w, nonfinite, stream):
        fn(z, v, hist, noise, zin, c_total, 0, coef, step_ptr, n, L, d, h, w, nonfinite, stream)
    return launch


def add_x0_step(prog, kind: str, with_noise: bool):
    """Append ctsi_x0_step to the step program `prog` (engine.UNetProgram.add_sampler_step under update_form 'x0', in the
    place of the eps-form update): `prog.eps` holds the network's raw v -- rows [0, n) after the guidance in a guided
    program -- and `prog.hist` the previous data prediction where the kind has one ('dpmpp')."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, L, d, h, w = prog.n, prog.L, prog.d, prog.h, prog.w
    xp, c_total, zin_bytes, f32 = prog._sampler_zin()
    step = x0_step_launcher(lib, f32)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    noise = prog.noise if with_noise else None
    zp, vp, hp, npz, cp, sp, nfp = (p(t) for t in (prog.z, prog.eps, prog.hist, noise, prog.coef, prog.step_ptr,
                                                   prog.nonfinite))
    xin = prog.xin

    def run_step():
        step(zp, vp, hp, npz, xp, c_total, cp, sp, n, L, d, h, w, nfp, sptr)
        if not f32:
            xin.dirty = True

    nbytes = (4 + 4 + 4 + zin_bytes + (4 if with_noise else 0) + (8 if prog.hist is not None else 0)) * float(
        n * L * d * h * w)
    prog._emit(run_step, "sampler.step", nbytes=nbytes,
               audit=dict(kind="x0_step", sampler=kind, z=prog.z, v=prog.eps, hist=prog.hist, noise=noise, zin=prog._zin_act(),
                          coef=prog.coef, step_ptr=prog.step_ptr, nonfinite=prog.nonfinite, n=n, L=L))
