"""Learned reverse variance and the strided ancestral sampler (Nichol & Dhariwal 2021, "Improved DDPM").

`UNet3D(learn_sigma=True)` ends in a head of 2L channels -- [0, L) the prediction (eps or v), [L, 2L) the raw variance channels
v -- and a diffusion whose attribute `var_type` is 'learned_range' reads them: the reverse log-variance of a step is f log(beta) + (1 - f)
log(beta~), f = (v + 1) / 2.  This module holds the validation of the two settings, the host tables (float64, rounded once) and
the launches the programs add (csrc/learned_sigma.hip):

  respaced_ddpm_rows   the coefficient rows of ctsi_ddpm_lv_step for a descending timestep subset (Improved-DDPM respacing)
  loss_schedule_rows   the per-timestep rows of ctsi_hybrid_loss_fwd / _bwd and of the single-step API
  add_sigma_split      ctsi_sigma_split behind the 2L-channel head of a step program: everything downstream reads the packed eps
  hybrid_norms         the per-sample factors of L_simple + lambda L_vb
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from .lib import CtsiError

VAR_TYPES = ("fixed_small", "learned_range")


def check_var_type(v) -> str:
    """Validate a var_type value ('fixed_small' | 'learned_range'); raises ValueError otherwise."""
    if not isinstance(v, str) or v not in VAR_TYPES:
        raise ValueError(f"unknown var_type {v!r}: expected one of {VAR_TYPES}")
    return v


def pairing_error(var_type, learn_sigma) -> str:
    """'' when the diffusion's var_type and the U-Net's learn_sigma belong together, else the sentence that says why not."""
    learned = check_var_type(var_type) == "learned_range"
    if learned and not learn_sigma:
        return ("diffusion.var_type = 'learned_range' (config key var_type) needs a U-Net built with learn_sigma=True (config "
                "key unet_learn_sigma): the model has no variance channels")
    if learn_sigma and not learned:
        return ("a U-Net built with learn_sigma=True needs the attribute diffusion.var_type = 'learned_range' (config key "
                "var_type): under 'fixed_small' its variance channels would never be trained or read")
    return ""


def check_pairing(diffusion, model):
    """CtsiError at first use when var_type and learn_sigma do not belong together (an engine UNet3D only: any other
    callable has no such attribute and must return L channels)."""
    if not hasattr(model, "learn_sigma"):
        return
    msg = pairing_error(getattr(diffusion, "var_type", "fixed_small"), bool(model.learn_sigma))
    if msg:
        raise CtsiError(msg)


def check_learn_sigma_unsharded(unet, sharded: bool):
    if sharded and getattr(unet, "learn_sigma", False):
        raise CtsiError("learn_sigma=True does not support depth sharding (unet.depth_shard_comm): the sharded step program "
                        "has no split launch; drop the communicator")


def _clipped_log_posterior(post_var: np.ndarray, last: int) -> np.ndarray:
    """log of the posterior variances of a chain whose entry `last` is the final step (variance 0): that entry takes its
    neighbour's value, the clip of Improved DDPM (a one-step chain has no neighbour: log(1e-20), the reference's clamp)."""
    out = np.empty_like(post_var)
    n = len(post_var)
    for i in range(n):
        out[i] = math.log(post_var[i]) if post_var[i] > 0 else float("nan")
    nb = last - 1 if last == n - 1 else last + 1
    out[last] = out[nb] if 0 <= nb < n and not math.isnan(out[nb]) else math.log(1e-20)
    if np.isnan(out).any():
        raise CtsiError("the timestep list repeats a timestep or is not descending: a respaced step has no variance")
    return out


def respaced_ddpm_rows(diffusion, t_desc: Sequence[int], clip: bool = True, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Coefficient rows of ctsi_ddpm_lv_step for the DESCENDING timestep list `t_desc` (row j serves loop position j):
    {sqrt(1 - abar), sqrt(abar), coef1', coef2', log beta', log beta~' clipped, s, clip} with s = [j is not the last row]
    exp(log beta~' / 2), the fixed-small noise scale (the learned scale is s exp(f (c4 - c5) / 2); the issue's row has the
    bare flag there: carrying the scale keeps every exp of a uniform value on the host).

    Improved-DDPM respacing, in float64 from `alphas_cumprod`, rounded once to `dtype`: with a = abar_{t_j} and a' the abar of
    the next list entry (1 behind the last),  beta' = 1 - a / a',  coef1' = beta' sqrt(a') / (1 - a),  coef2' = (1 - a')
    sqrt(1 - beta') / (1 - a),  beta~' = beta' (1 - a') / (1 - a); the last row's log beta~' takes its neighbour's value.

    The full chain T-1 .. 0 is not respaced: its rows are read from the registered buffers, where ctsi_ddpm_step's rows come
    from (columns 0-3 are ddpm_coef_rows' bit for bit and column 6 is its column 4: with no variance channels the step has
    ctsi_ddpm_step's bits on every row), with log beta in float64 from `betas`; entry t = 0 of the clipped log-variance takes entry 1's value there too.  `clip`: 1.0 (clamp z_0 to [-1, 1]) or 0."""
    t_list = [int(t) for t in t_desc]
    n = len(t_list)
    if n == 0:
        raise ValueError("the timestep list is empty")
    T = int(diffusion.timesteps)
    if any(not 0 <= t < T for t in t_list) or any(a <= b for a, b in zip(t_list, t_list[1:])):
        raise ValueError(f"t_desc must be strictly descending timesteps in [0, {T}), got {t_list[:4]}...")
    rows = torch.zeros(n, 8, dtype=torch.float64)
    if t_list == list(range(T - 1, -1, -1)) and T > 1:
        idx = torch.as_tensor(t_list, dtype=torch.long)
        buf = lambda name: getattr(diffusion, name).detach().cpu()[idx].double()
        rows[:, 0] = buf("sqrt_one_minus_alphas_cumprod")
        rows[:, 1] = buf("sqrt_alphas_cumprod")
        rows[:, 2] = buf("posterior_mean_coef1")
        rows[:, 3] = buf("posterior_mean_coef2")
        rows[:, 4] = torch.log(buf("betas"))
        plv = buf("posterior_log_variance_clipped")
        plv[-1] = plv[-2]
        rows[:, 5] = plv
        rows[:, 6] = diffusion.ddpm_coef_rows(t_list)[:, 4].detach().cpu().double()
    else:
        ac = diffusion.alphas_cumprod.detach().double().cpu().numpy()
        a = ac[t_list]
        a_prev = np.append(a[1:], 1.0)
        beta = 1.0 - a / a_prev
        post = beta * (1.0 - a_prev) / (1.0 - a)
        with np.errstate(divide="ignore"):
            log_beta = np.log(beta)
        if not np.isfinite(log_beta).all() or not np.isfinite(1.0 / a).all():
            raise CtsiError("the respaced chain has a step with abar = 0 or beta' = 0: the eps-form ancestral update cannot "
                            "take it (a zero-terminal-SNR schedule needs update_form='x0', which has no strided ancestral form)")
        rows[:, 0] = torch.from_numpy(np.sqrt(1.0 - a))
        rows[:, 1] = torch.from_numpy(np.sqrt(a))
        rows[:, 2] = torch.from_numpy(beta * np.sqrt(a_prev) / (1.0 - a))
        rows[:, 3] = torch.from_numpy((1.0 - a_prev) * np.sqrt(1.0 - beta) / (1.0 - a))
        rows[:, 4] = torch.from_numpy(log_beta)
        rows[:, 5] = torch.from_numpy(_clipped_log_posterior(post, n - 1))
        rows[:-1, 6] = torch.exp(0.5 * rows[:-1, 5])
    rows[:, 7] = 1.0 if clip else 0.0
    return rows.to(dtype)


def loss_schedule_rows(diffusion, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One row per TIMESTEP for ctsi_hybrid_loss_fwd / _bwd: {sqrt(abar), sqrt(1 - abar), coef1, coef2, log beta, log beta~
    clipped, log beta - log beta~, 0} (the difference in float64, rounded once: at large t the two logs agree to a few 1e-3 and
    the bound's terms are of that order).  Columns 0-3 and 5 are the registered buffers (what q_sample and the samplers read), log beta is float64 of
    `betas`; entry 0 of the clipped log-variance takes entry 1's value (Improved DDPM's clip: the reference's clamp leaves
    log(1e-20) there, which as an end of the learned range would make f meaningless at t = 0)."""
    T = int(diffusion.timesteps)
    buf = lambda name: getattr(diffusion, name).detach().cpu().double()
    rows = torch.zeros(T, 8, dtype=torch.float64)
    rows[:, 0] = buf("sqrt_alphas_cumprod")
    rows[:, 1] = buf("sqrt_one_minus_alphas_cumprod")
    rows[:, 2] = buf("posterior_mean_coef1")
    rows[:, 3] = buf("posterior_mean_coef2")
    rows[:, 4] = torch.log(buf("betas"))
    plv = buf("posterior_log_variance_clipped").clone()
    if T > 1:
        plv[0] = plv[1]
    rows[:, 5] = plv
    rows[:, 6] = rows[:, 4] - rows[:, 5]
    return rows.to(dtype)


def step_rows_per_sample(diffusion, t, with_noise: bool, clip: bool) -> torch.Tensor:
    """One ctsi_ddpm_posterior_lv row per SAMPLE for the single-step API (p_mean_variance / p_sample under 'learned_range'):
    the full chain's row of each sample's timestep."""
    sched = loss_schedule_rows(diffusion, torch.float64)
    idx = t.reshape(-1).detach().cpu().long()
    rows = torch.zeros(len(idx), 8, dtype=torch.float64)
    rows[:, 0], rows[:, 1] = sched[idx, 1], sched[idx, 0]
    rows[:, 2:6] = sched[idx, 2:6]
    if with_noise:      # the scale ctsi_ddpm_posterior reads: [t != 0] exp(posterior_log_variance_clipped / 2) in fp32
        rows[:, 6] = diffusion.ddpm_coef_rows(idx.tolist())[:, 4].detach().cpu().double()
    rows[:, 7] = 1.0 if clip else 0.0
    return rows.float()


def hybrid_norms(snr_weight: torch.Tensor, count_norm: torch.Tensor, timesteps: int):
    """(norm, norm_vb) of ctsi_hybrid_loss_*: `count_norm`[b] is the batch / element-count normalisation the MSE term uses
    (without its loss weight); the bound takes the same one, times lambda / ln 2 with lambda = timesteps / 1000 (the rescaled
    hybrid objective of Improved DDPM, in bits per dimension)."""
    lam = float(timesteps) / 1000.0
    return snr_weight * count_norm, count_norm * (lam / math.log(2.0))


def add_sigma_split(prog):
    """Append ctsi_sigma_split to the U-Net program `prog` right behind its 2L-channel head: `out2` -> the packed `eps` of all
    network rows (what ctsi_pred_to_eps, the guidance, every update and the counters read, unchanged) and, once a step that
    reads them has allocated `vraw`, the variance channels of rows [0, n) -- under guidance the conditional half."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, nb, L, d, h, w = prog.n, prog.nb, prog.L, prog.d, prog.h, prog.w
    op, ep = C.c_void_p(prog.out2.data_ptr()), C.c_void_p(prog.eps.data_ptr())

    def run():
        vp = C.c_void_p(0 if prog.vraw is None else prog.vraw.data_ptr())
        lib.sigma_split(op, ep, vp, nb, n, L, d, h, w, sptr)

    # read 2L channels of nb rows; written: L of nb rows, and L of n rows once a step reads the variance channels
    prog._emit(run, "sigma.split", nbytes=4.0 * (3 * nb + n) * L * d * h * w,
               audit=dict(kind="sigma_split", out2=prog.out2, eps=prog.eps, vraw=lambda: prog.vraw, n=nb, n_keep=n, L=L))


def emit_hybrid_loss(prog, backward: bool):
    """The loss launch of a learn_sigma train program (train_engine.UNetTrainProgram): ctsi_hybrid_loss_fwd in place of
    ctsi_mse_loss_fwd, ctsi_hybrid_loss_bwd in place of ctsi_mse_loss_bwd.  `prog.eps` is the 2L-channel head output, `prog.d_eps`
    its bf16 gradient (Lp channels), `prog.lv_sched` / `prog.norm_vb` are set per forward."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, L, d, h, w = prog.n, prog.L, prog.d, prog.h, prog.w
    v_pred = int(prog.prediction == "v_prediction")
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())

    def args():
        return (p(prog.eps), p(prog.z0), p(prog.noise), p(prog.t_rows), p(prog.lv_sched), int(prog.lv_sched.shape[0]), v_pred,
                p(prog.mask if prog.use_mask else None), p(prog.norm), p(prog.norm_vb))

    record = dict(pred2=prog.eps, z0=prog.z0, noise=prog.noise, t_rows=prog.t_rows, sched=lambda: prog.lv_sched, v_pred=v_pred,
                  mask=lambda: prog.mask if prog.use_mask else None, norm=prog.norm, norm_vb=prog.norm_vb)
    if backward:
        prog._emit(lambda: lib.hybrid_loss_bwd(*args(), p(prog.gscale), n, L, d, h, w, prog.d_eps.ip, prog.Lp, sptr),
                   "loss.bwd", audit=dict(kind="hybrid_loss_bwd", gscale=prog.gscale, out=prog.d_eps, **record))
    else:
        prog._emit(lambda: lib.hybrid_loss_fwd(*args(), n, L, d, h, w, p(prog.loss_ws), p(prog.loss_out), sptr),
                   "loss.fwd", audit=dict(kind="hybrid_loss.fwd", out=prog.loss_out, **record))
