"""GaussianDiffusion — schedules and DDPM sampling (mirror of reference models/diffusion.py).

The ten (timesteps,) fp32 buffers are built with the same torch ops, in the same order, as the
reference (diffusion.py:27-79) so they are bit-identical and checkpoint-compatible.  The reverse
process runs on the HIP engine: `p_sample_loop` drives a captured U-Net step graph and the
ctsi_ddpm_step kernel; single steps with per-sample timesteps (`p_mean_variance`, `p_sample`,
`_predict_z_0_from_noise`) use ctsi_ddpm_posterior.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .lib import CtsiError


class GaussianDiffusion(nn.Module):
    def __init__(self, noise_schedule='cosine', timesteps=1000, beta_start=0.0001, beta_end=0.02,
                 prediction_type='epsilon'):
        """`prediction_type` (additive): what the U-Net's output means -- 'epsilon' (default, the reference) or
        'v_prediction', v = sqrt(abar) eps - sqrt(1 - abar) z_0 (Salimans & Ho 2022).  A plain attribute:
        no buffer is registered for it, the coefficients come from `alphas_cumprod`."""
        super().__init__()
        from .prediction import check_prediction_type
        self.prediction_type = check_prediction_type(prediction_type)
        # a plain attribute like update_form (the config key `var_type` sets it): 'fixed_small' (the reference:
        # the reverse variance is the posterior beta~_t) or 'learned_range' (Nichol & Dhariwal 2021) -- the model, a
        # UNet3D(learn_sigma=True), emits L more channels v, the reverse log-variance is f log beta_t + (1 - f) log beta~_t with
        # f = (v + 1) / 2, and training_loss adds the variational-bound term that trains them.  Validated where it is read.
        self.var_type = "fixed_small"
        # plain attributes like prediction_type (no parameter, no buffer): the form of the sampler updates
        # ('eps' | 'x0'), whether rescale_zero_terminal_snr() has rewritten the schedule, and the training loss weight
        # ('min_snr' | 'uniform')
        self.update_form = "eps"
        self.zero_terminal_snr = False
        self.loss_weighting = "min_snr"
        self.timesteps = timesteps
        self.noise_schedule = noise_schedule
        if noise_schedule == 'linear':
            betas = self._linear_beta_schedule(timesteps, beta_start, beta_end)
        elif noise_schedule == 'cosine':
            betas = self._cosine_beta_schedule(timesteps)
        else:
            raise ValueError(f"Unknown noise schedule: {noise_schedule}")

        alphas = 1.0 - betas
        abar = torch.cumprod(alphas, dim=0)
        abar_prev = F.pad(abar[:-1], (1, 0), value=1.0)
        post_var = betas * (1.0 - abar_prev) / (1.0 - abar)
        for name, value in (
            ('betas', betas),
            ('alphas', alphas),
            ('alphas_cumprod', abar),
            ('alphas_cumprod_prev', abar_prev),
            ('sqrt_alphas_cumprod', torch.sqrt(abar)),
            ('sqrt_one_minus_alphas_cumprod', torch.sqrt(1.0 - abar)),
            ('posterior_variance', post_var),
            ('posterior_log_variance_clipped', torch.log(torch.clamp(post_var, min=1e-20))),
            ('posterior_mean_coef1', betas * torch.sqrt(abar_prev) / (1.0 - abar)),
            ('posterior_mean_coef2', (1.0 - abar_prev) * torch.sqrt(alphas) / (1.0 - abar)),
        ):
            self.register_buffer(name, value)

    def _linear_beta_schedule(self, timesteps, beta_start, beta_end):
        return torch.linspace(beta_start, beta_end, timesteps)

    def _cosine_beta_schedule(self, timesteps, s=0.008):
        # abar(x) = cos^2(((x/T) + s)/(1+s) * pi/2), normalised by abar(0); beta clipped to [1e-4, 0.9999]
        grid = torch.linspace(0, timesteps, timesteps + 1)
        abar = torch.cos(((grid / timesteps) + s) / (1 + s) * math.pi * 0.5) ** 2
        abar = abar / abar[0]
        return torch.clip(1 - (abar[1:] / abar[:-1]), 0.0001, 0.9999)

    def _extract(self, a, t, x_shape):
        out = a.gather(-1, t).float()
        return out.reshape(t.shape[0], *((1,) * (len(x_shape) - 1)))

    # ---- forward process (elementwise, torch ops on whatever device the tensors live) --------------
    def q_sample(self, z_0, t, noise=None):
        if noise is None:
            noise = torch.randn_like(z_0)
        z_t = (self._extract(self.sqrt_alphas_cumprod, t, z_0.shape) * z_0 +
               self._extract(self.sqrt_one_minus_alphas_cumprod, t, z_0.shape) * noise)
        return z_t, noise

    # ---- zero terminal SNR and the x0 form ------------------------------------------------------
    def rescale_zero_terminal_snr(self):
        """Rewrite the ten buffers in place to the zero-terminal-SNR schedule of Lin et al. 2024 (Algorithm 1):
        sqrt(abar) is shifted and scaled so that abar_{T-1} = 0 exactly and abar_0 stays, in float64, every buffer recomputed
        from that and rounded once to fp32; beta_{T-1} = 1 (no 0.9999 clip).  All buffers stay finite (coef1 = sqrt(abar_{T-2}),
        coef2 = 0 at T-1).  Needs 'v_prediction' (ValueError otherwise): at abar = 0 an epsilon output says nothing about
        z_0.  Sets `zero_terminal_snr = True` and `update_form = 'x0'`, the only form that can evaluate T-1.  Idempotent: a
        schedule that already ends in abar = 0 is left as it is.  Buffer names and the state dict keys do not change, so a
        checkpoint of the rescaled model loads under the old names (its config carries `zero_terminal_snr: true`)."""
        from .x0_form import BUFFERS, check_update_form, rescaled_schedule
        check_update_form("x0", self.prediction_type)
        if float(self.alphas_cumprod[-1]) != 0.0:
            with torch.no_grad():
                for name, value in rescaled_schedule(self.alphas_cumprod).items():
                    buf = getattr(self, name)
                    buf.copy_(value.to(buf.dtype))
            assert set(BUFFERS) == set(dict(self.named_buffers()))
        self.zero_terminal_snr = True
        self.update_form = "x0"
        return self

    def _x0_form(self) -> bool:
        from .x0_form import check_update_form
        return check_update_form(self.update_form, self.prediction_type) == "x0"

    def _x0_rows(self, t, with_noise, clip):
        """One ctsi_x0_step row per SAMPLE for the single-step API: sampler.x0_coef_rows 'ddpm' at the sample's timestep,
        s only with a noise tensor, clip 1 or none."""
        from .x0_form import x0_coef_rows
        rows = x0_coef_rows(self, "ddpm", t.reshape(-1).tolist(), dtype=torch.float64)
        if not with_noise:
            rows[:, 5] = 0.0
        rows[:, 6] = 1.0 if clip else 0.0
        return rows.float()

    def _x0_posterior(self, z_t, t, v, noise, clip):
        """The posterior mean (plus noise) of p_mean_variance / p_sample under update_form 'x0': ctsi_x0_step_f32 on each
        sample's contiguous elements (c = per_sample, d = h = w = 1, where NCDHW and NDHWC coincide; no input slice), one row
        per sample.  No division: per-sample timesteps may include T-1 of a zero-terminal-SNR schedule."""
        from .engine import Ctx, _ptr
        if not (z_t.is_cuda and v.is_cuda):
            raise CtsiError("the reverse-process arithmetic runs on the HIP engine: move the tensors to a ROCm device "
                            "(there is no CPU path)")
        if tuple(v.shape) != tuple(z_t.shape) or t.reshape(-1).shape[0] != z_t.shape[0]:
            raise ValueError(f"expected a model output of shape {tuple(z_t.shape)} and one timestep per sample, got "
                             f"{tuple(v.shape)} and t of shape {tuple(t.shape)}")
        ctx = Ctx.get(z_t.device)
        n = int(z_t.shape[0])
        per = z_t.numel() // n
        out = z_t.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
        vv = v.detach().to(torch.float32).contiguous()
        nz = None if noise is None else noise.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
        coef = self._x0_rows(t, nz is not None, clip).to(ctx.device).contiguous()
        at = lambda tns, b, width: C.c_void_p(0 if tns is None else tns.data_ptr() + 4 * b * width)
        with ctx.scope():
            for b in range(n):
                ctx.lib.x0_step_f32(at(out, b, per), at(vv, b, per), None, at(nz, b, per), None, 0, 0, at(coef, b, 8), None,
                                    1, per, 1, 1, 1, None, ctx.sptr)
            for tns in (out, vv, nz, coef):
                if tns is not None:
                    tns.record_stream(ctx.stream)
        return out

    def _check_eps_form(self, t):
        from .x0_form import check_eps_form_timesteps
        check_eps_form_timesteps(self.alphas_cumprod, t.reshape(-1).tolist())

    # ---- v-prediction ---------------------------------------------------------------------------
    def v_target(self, z_0, t, noise):
        """The training target of 'v_prediction': v = sqrt(abar_t) noise - sqrt(1 - abar_t) z_0 (elementwise torch ops on
        whatever device the tensors live, from the two buffers q_sample reads; the training step forms it in
        ctsi_q_sample_v from the same buffers)."""
        return (self._extract(self.sqrt_alphas_cumprod, t, z_0.shape) * noise -
                self._extract(self.sqrt_one_minus_alphas_cumprod, t, z_0.shape) * z_0)

    def pred_to_eps_rows(self, t_desc, dtype=torch.float32):
        """Rows {sqrt(abar_t), sqrt(1 - abar_t), 0, 0} of ctsi_pred_to_eps for the integer timesteps `t_desc`: eps =
        sqrt(abar) v + sqrt(1 - abar) z_t.  float64 from `alphas_cumprod`, rounded once to `dtype`."""
        idx = torch.as_tensor([int(v) for v in t_desc], dtype=torch.long)
        ab = self.alphas_cumprod.detach().double().cpu()[idx]
        rows = torch.zeros(len(idx), 4, dtype=torch.float64)
        rows[:, 0] = torch.sqrt(ab)
        rows[:, 1] = torch.sqrt(1.0 - ab)
        return rows.to(dtype)

    @torch.no_grad()
    def model_output_to_eps(self, z_t, t, out):
        """The noise prediction a model output stands for, per-sample t: `out` itself under 'epsilon'; under
        'v_prediction' eps = sqrt(abar_t) out + sqrt(1 - abar_t) z_t -- one ctsi_pred_to_eps launch with one row per sample
        on ROCm tensors (fp32 result), the same formula in torch on host tensors (their dtype)."""
        return out if self.prediction_type == "epsilon" else self._from_v(z_t, t, out, False)

    @torch.no_grad()
    def _predict_z_0_from_v(self, z_t, t, v):
        """z_0 = sqrt(abar_t) z_t - sqrt(1 - abar_t) v, per-sample t: no division, so it stays exact where abar_t is tiny.
        The same launch as model_output_to_eps with the rows {-sqrt(1 - abar), sqrt(abar), 0}."""
        return self._from_v(z_t, t, v, True)

    def _from_v(self, z_t, t, v, want_z0):
        """a v + b z_t per sample: (a, b) = (sqrt(abar), sqrt(1 - abar)) for eps, (-sqrt(1 - abar), sqrt(abar)) for z_0."""
        if tuple(v.shape) != tuple(z_t.shape) or t.reshape(-1).shape[0] != z_t.shape[0]:
            raise ValueError(f"expected a model output of shape {tuple(z_t.shape)} and one timestep per sample, got "
                             f"{tuple(v.shape)} and t of shape {tuple(t.shape)}")
        rows = self.pred_to_eps_rows(t.reshape(-1).tolist(), torch.float64)
        if want_z0:
            rows = torch.stack([-rows[:, 1], rows[:, 0], rows[:, 2], rows[:, 3]], dim=1)
        if not (z_t.is_cuda and v.is_cuda):
            a, b = (rows[:, k].to(v.dtype).reshape(-1, *((1,) * (v.dim() - 1))) for k in (0, 1))
            return a * v + b * z_t
        from .engine import Ctx, _ptr
        ctx = Ctx.get(z_t.device)
        n = int(z_t.shape[0])
        z = z_t.detach().to(torch.float32).contiguous()
        out = v.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
        rows = rows.to(ctx.device, torch.float32).contiguous()
        with ctx.scope():
            ctx.lib.pred_to_eps(_ptr(out), _ptr(z), None, _ptr(rows), None, n, n, n, z.numel() // n, ctx.sptr)
            for tns in (z, out, rows):
                tns.record_stream(ctx.stream)
        return out

    # ---- DDPM reverse process on the HIP engine -------------------------------------------------------
    def ddpm_coef_rows(self, t_desc):
        """Per-step coefficient rows for ctsi_ddpm_step, fp32 values taken from the registered buffers
        exactly as p_mean_variance / p_sample read them (diffusion.py:290-336)."""
        idx = torch.as_tensor(list(t_desc), dtype=torch.long, device=self.betas.device)
        rows = torch.zeros(len(idx), 8, dtype=torch.float32, device=self.betas.device)
        rows[:, 0] = self.sqrt_one_minus_alphas_cumprod[idx]
        rows[:, 1] = self.sqrt_alphas_cumprod[idx]
        rows[:, 2] = self.posterior_mean_coef1[idx]
        rows[:, 3] = self.posterior_mean_coef2[idx]
        rows[:, 4] = (idx != 0).float() * torch.exp(0.5 * self.posterior_log_variance_clipped[idx])
        return rows

    @torch.no_grad()
    def p_sample_loop(self, model, shape, c, device, progress=True, noise_fn=None, num_steps=None, guidance_scale=1.0,
                      guidance_rescale=0.0):
        """z_T ~ N(0, I); for t = T-1..0: one U-Net evaluation + ctsi_ddpm_step (clip to [-1, 1]).

        `noise_fn(i, shape)` (optional, additive kwarg) supplies the initial noise (i = -1) and the
        per-step noise tensors instead of torch.randn; `num_steps` truncates the loop to its first
        steps (both are test hooks; defaults reproduce the reference).  `guidance_scale` / `guidance_rescale`
        (additive): classifier-free guidance, see sampler.run_sampler."""
        from .sampler import DDPMSampler  # local import: sampler imports this module
        return DDPMSampler(self, model).sample(shape, c, device, progress=progress, noise_fn=noise_fn, num_steps=num_steps,
                                               guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)

    # ---- single reverse steps with per-sample timesteps (diffusion.py:249-338) -------------------------------------
    def _posterior_rows(self, t):
        """One coefficient row per SAMPLE for ctsi_ddpm_posterior, read from the registered buffers exactly where
        _predict_z_0_from_noise / p_mean_variance / p_sample read them."""
        idx = t.reshape(-1).to(device=self.betas.device, dtype=torch.long)
        return self.ddpm_coef_rows(idx.tolist())

    def _posterior(self, z_t, t, eps, noise, clip, want_z0, want_out):
        from .engine import Ctx, _ptr
        if not (z_t.is_cuda and eps.is_cuda):
            raise CtsiError("the reverse-process arithmetic runs on the HIP engine: move the tensors to a ROCm device "
                            "(there is no CPU path)")
        if tuple(eps.shape) != tuple(z_t.shape) or t.reshape(-1).shape[0] != z_t.shape[0]:
            raise ValueError(f"expected noise_pred of shape {tuple(z_t.shape)} and one timestep per sample, got "
                             f"{tuple(eps.shape)} and t of shape {tuple(t.shape)}")
        ctx = Ctx.get(z_t.device)
        n = int(z_t.shape[0])
        z = z_t.detach().to(torch.float32).contiguous()
        e = eps.detach().to(torch.float32).contiguous()
        nz = None if noise is None else noise.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
        coef = self._posterior_rows(t).to(ctx.device, torch.float32).contiguous()
        z0 = torch.empty_like(z) if want_z0 else None
        out = torch.empty_like(z) if want_out else None
        with ctx.scope():
            ctx.lib.ddpm_posterior(_ptr(z), _ptr(e), _ptr(nz), _ptr(z0), _ptr(out), _ptr(coef), n, z.numel() // n,
                                   int(bool(clip)), ctx.sptr)
            for tns in (z, e, nz, coef):
                if tns is not None:
                    tns.record_stream(ctx.stream)
        return z0, out

    def _learned(self) -> bool:
        from .learned_sigma import check_var_type
        return check_var_type(self.var_type) == "learned_range"

    def _split_output(self, out, z_t):
        """(prediction, variance channels) of a learn_sigma model's 2L-channel output (views; CtsiError on another shape)."""
        L = int(z_t.shape[1])
        if not torch.is_tensor(out) or tuple(out.shape) != (z_t.shape[0], 2 * L) + tuple(z_t.shape[2:]):
            raise CtsiError(f"var_type='learned_range' needs a model output of 2 x {L} channels (UNet3D(learn_sigma=True)), got "
                            f"shape {tuple(getattr(out, 'shape', ()))}")
        return out[:, :L], out[:, L:]

    def _posterior_lv(self, z_t, t, eps, vraw, noise, clip, want_logvar):
        """(sample or mean, log-variance per element) under 'learned_range': one ctsi_ddpm_posterior_lv launch, fp32 NCDHW, one
        full-chain row per sample (learned_sigma.step_rows_per_sample)."""
        from .engine import Ctx, _ptr
        from .learned_sigma import step_rows_per_sample
        if not (z_t.is_cuda and eps.is_cuda):
            raise CtsiError("the reverse-process arithmetic runs on the HIP engine: move the tensors to a ROCm device "
                            "(there is no CPU path)")
        ctx = Ctx.get(z_t.device)
        n = int(z_t.shape[0])
        z = z_t.detach().to(torch.float32).contiguous()
        e = eps.detach().to(torch.float32).contiguous()
        vr = vraw.detach().to(torch.float32).contiguous()
        nz = None if noise is None else noise.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
        coef = step_rows_per_sample(self, t, nz is not None, clip).to(ctx.device).contiguous()
        out = torch.empty_like(z)
        logvar = torch.empty_like(z) if want_logvar else None
        with ctx.scope():
            ctx.lib.ddpm_posterior_lv(_ptr(z), _ptr(e), _ptr(vr), _ptr(nz), _ptr(out), _ptr(logvar), _ptr(coef), n,
                                      z.numel() // n, ctx.sptr)
            for tns in (z, e, vr, nz, coef):
                if tns is not None:
                    tns.record_stream(ctx.stream)
        return out, logvar

    @torch.no_grad()
    def _predict_z_0_from_noise(self, z_t, t, noise_pred):
        """z_0 = (z_t - sqrt(1 - abar_t) * noise_pred) / sqrt(abar_t), per-sample t (diffusion.py:249-268)."""
        return self._posterior(z_t, t, noise_pred, None, False, True, False)[0]

    @torch.no_grad()
    def p_mean_variance(self, model, z_t, t, c, clip_denoised=True):
        """(mean, variance, log_variance) of q(z_{t-1} | z_t, z_0_pred) (diffusion.py:270-308).  `model` is any
        `model(z, t, c) -> eps` callable on the ROCm device (the engine's UNet3D evaluates per-sample timesteps); the
        posterior mean is one ctsi_ddpm_posterior launch.  variance / log_variance are the (B,1,1,1,1) buffer gathers
        the reference returns.  Under 'v_prediction' the model returns v (model_output_to_eps converts it); under
        update_form 'x0' the mean comes from the raw v without a division (_x0_posterior).  Under var_type='learned_range'
         the model returns 2L channels and variance / log_variance are per element, of z_t's shape: the
        learned exp(lv) and lv = f log beta_t + (1 - f) log beta~_t."""
        if self._learned():
            if self._x0_form():
                raise CtsiError("update_form='x0' does not support a learned reverse variance (var_type='learned_range')")
            self._check_eps_form(t)
            pred, vraw = self._split_output(model(z_t, t, c), z_t)
            noise_pred = self.model_output_to_eps(z_t, t, pred.contiguous())
            mean, log_variance = self._posterior_lv(z_t, t, noise_pred, vraw, None, clip_denoised, True)
            return mean, torch.exp(log_variance), log_variance
        if self._x0_form():
            mean = self._x0_posterior(z_t, t, model(z_t, t, c), None, clip_denoised)
        else:
            self._check_eps_form(t)
            noise_pred = self.model_output_to_eps(z_t, t, model(z_t, t, c))
            _, mean = self._posterior(z_t, t, noise_pred, None, clip_denoised, False, True)
        variance = self._extract(self.posterior_variance, t, z_t.shape)
        log_variance = self._extract(self.posterior_log_variance_clipped, t, z_t.shape)
        return mean, variance, log_variance

    @torch.no_grad()
    def p_sample(self, model, z_t, t, c, clip_denoised=True, noise=None):
        """One DDPM step z_t -> z_{t-1} (diffusion.py:310-338); per-sample `t` and `clip_denoised=False` as in the
        reference.  The noise is drawn with `torch.randn_like(z_t)` after the network evaluation, where the reference
        draws it (`noise=` injects it instead: tests).  A batch-uniform clipped step on the engine's own UNet3D takes
        the captured-graph path of the sampling loop (same arithmetic, ctsi_ddpm_step)."""
        from .sampler import _is_engine_unet, run_sampler
        tv = [int(v) for v in t.reshape(-1).tolist()]
        if self._learned():
            if self._x0_form():
                raise CtsiError("update_form='x0' does not support a learned reverse variance (var_type='learned_range')")
            self._check_eps_form(t)
            pred, vraw = self._split_output(model(z_t, t, c), z_t)
            if noise is None:
                noise = torch.randn_like(z_t)
            noise_pred = self.model_output_to_eps(z_t, t, pred.contiguous())
            return self._posterior_lv(z_t, t, noise_pred, vraw, noise, clip_denoised, False)[0]
        if len(set(tv)) == 1 and clip_denoised and noise is None and _is_engine_unet(model):
            return run_sampler(self, model, tuple(z_t.shape), c, z_t.device, kind="ddpm", t_desc=[tv[0]],
                               progress=False, z_init=z_t)
        x0_form = self._x0_form()
        if not x0_form:
            self._check_eps_form(t)
        out = model(z_t, t, c)
        if noise is None:
            noise = torch.randn_like(z_t)
        if x0_form:       # (the raw v, no division)
            return self._x0_posterior(z_t, t, out, noise, clip_denoised)
        noise_pred = self.model_output_to_eps(z_t, t, out)
        return self._posterior(z_t, t, noise_pred, noise, clip_denoised, False, True)[1]

    def _snr_weight(self, t):
        """The per-sample loss weight of training_loss (folded into norm[b] on the host).  'min_snr' -- Min-SNR-5 (Hang et al.
        2023): min(snr, 5) / snr on an eps target, min(snr, 5) / (snr + 1) on a v target.  'uniform' (DESIGN section 20): 1,
        the plain loss Lin et al. train with -- at SNR 0, the terminal step of a zero-terminal-SNR schedule, the Min-SNR v
        weight is 0 and that step would never be trained."""
        from .x0_form import check_loss_weighting
        uniform = check_loss_weighting(self.loss_weighting) == "uniform"
        snr = self.alphas_cumprod[t] / (1 - self.alphas_cumprod[t] + 1e-8)
        v_pred = self.prediction_type == "v_prediction"
        snr_weight = torch.clamp(snr, max=5.0) / (snr + 1.0 if v_pred else snr + 1e-8)
        return torch.ones_like(snr_weight) if uniform else snr_weight

    def training_loss(self, model, z_0, c, mask=None, vae=None, v_gt=None, use_ssim=False, ssim_weight=0.0,
                      t=None, noise=None, cond_drop_prob=0.0, cond_keep=None):
        """Min-SNR-5 weighted epsilon-prediction loss (diffusion.py:108-247; under prediction_type='v_prediction' the
        target is v and the weight min(snr, 5) / (snr + 1), everything else unchanged; `self.loss_weighting = 'uniform'`
        makes the weight 1) with forward AND backward on the HIP
        engine: the returned scalar carries an autograd node whose backward launches the engine's gradient kernels
        and feeds the U-Net parameters' .grad.

        t ~ randint(0, T, (B,)) and noise ~ randn_like(z_0) are drawn with torch's generator in the reference's
        order; `t=` / `noise=` (additive kwargs) inject them instead (tests).  The three normalisations of the
        reference (no mask; mask with equal valid counts; mask with per-sample counts) are folded into one
        per-sample factor.  The optional MS-SSIM term (a gradient-free logging term: the reference decodes under no_grad)
        needs the third-party `pytorch_msssim`; without it the reference warns and returns the MSE loss, and so does this
        engine (see the end of the function).

        Conditioning dropout (additive; what makes a checkpoint guidable): sample b trains on the null
        conditioning c = 0 where keep[b] is False.  keep = torch.rand(B) >= cond_drop_prob is drawn AFTER t and noise, and
        only when cond_drop_prob > 0, `cond_keep` is None and the U-Net is in training mode -- so cond_drop_prob = 0 leaves
        the generator where it was, and a seed gives the same t and noise at every probability.  `cond_keep` (bool, (B,))
        injects the mask.  The conditioning carries no gradient, so the backward is unchanged.  loss_dict gains
        'cond_dropped' (the number of dropped samples) when a mask was in force.

        ResBlock dropout (additive): with `model.dropout` > 0 (read here, at every forward) and the U-Net in
        training mode, conv2's input of every ResBlock is dropped by a mask that is a pure function of (seed, block, element).
        The 64-bit seed is drawn from torch's default CPU generator AFTER t and noise, and only when the threshold
        floor(dropout * 65536) is > 0 -- so dropout = 0 consumes exactly the random numbers it always did; the plain attribute
        `model.dropout_seed` (an int; None, the default, draws) injects it instead, the test hook beside `t=` / `noise=` (an
        attribute because this signature is pinned).  `model.eval()` turns dropout off.

        `training_loss_and_prediction` runs this body too: its request for the predicted clean latent is the
        private per-call attribute `_pred_request` (an attribute for the same reason), taken off the object first thing."""
        pred_request = self.__dict__.pop("_pred_request", None)
        p_drop = float(cond_drop_prob)
        if not 0.0 <= p_drop <= 1.0:
            raise ValueError(f"cond_drop_prob must lie in [0, 1], got {cond_drop_prob!r}")
        if cond_keep is not None and (not torch.is_tensor(cond_keep) or cond_keep.dtype != torch.bool
                                      or tuple(cond_keep.shape) != (z_0.shape[0],)):
            raise ValueError(f"cond_keep must be a bool tensor of shape ({z_0.shape[0]},)")
        from .train_engine import UNetTrainProgram, train_step
        from .engine import Ctx, cached_program, check_attention_mode
        from .norm_mod import dropout_active
        mode = check_attention_mode(getattr(model, "attention_mode", "fast"))
        from .learned_sigma import check_pairing, hybrid_norms
        check_pairing(self, model)
        learned = self._learned()
        drop_on = dropout_active(model)                     # (validates the plain attribute, read at every forward)
        drop_p = getattr(model, "dropout", 0.0)
        if not z_0.is_cuda:
            raise CtsiError("training_loss runs on the HIP engine: move the tensors to a ROCm device")
        B, L, d, h, w = z_0.shape
        device = z_0.device
        if t is None:
            t = torch.randint(0, self.timesteps, (B,), device=device, dtype=torch.long)
        if noise is None:
            noise = torch.randn_like(z_0)
        dropout_seed = getattr(model, "dropout_seed", None)
        if drop_on and dropout_seed is None:
            dropout_seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64).item())
        keep = cond_keep
        if keep is None and p_drop > 0.0 and getattr(model, "training", False):
            keep = torch.rand(B, device=device) >= p_drop
        if keep is not None:
            keep = keep.to(device)
            c = c * keep.to(c.dtype)[:, None, None, None, None]
        v_pred = self.prediction_type == "v_prediction"
        snr_weight = self._snr_weight(t)
        if mask is not None:
            m = mask.to(device=device, dtype=torch.float32)
            if m.dim() != 3 or m.shape[0] != B or m.shape[2] != d or m.shape[1] not in (1, L):
                raise ValueError(f"mask must be (B, C, T) = ({B}, 1 or {L}, {d}), got {tuple(m.shape)}")
            m = m.expand(B, L, d).contiguous()     # mask.unsqueeze(-1).unsqueeze(-1).expand_as(noise_pred)
            num_valid = m.reshape(B, -1).sum(dim=1) * (h * w)
            if bool((num_valid == num_valid[0]).all()):
                norm = (snr_weight.mean() / num_valid.sum()).expand(B)
                count_norm = (1.0 / num_valid.sum()).expand(B)
            else:
                norm = torch.where(num_valid > 0, snr_weight / (num_valid.clamp(min=1) * B),
                                   torch.zeros_like(snr_weight))
                count_norm = torch.where(num_valid > 0, 1.0 / (num_valid.clamp(min=1) * B), torch.zeros_like(snr_weight))
        else:
            m = None
            norm = snr_weight / float(B * L * d * h * w)
            count_norm = torch.full_like(snr_weight, 1.0 / float(B * L * d * h * w))
        # 'learned_range' (DESIGN section 24): L_simple keeps `norm`; the bound takes the same batch / element normalisation
        # without the loss weight, times lambda / ln 2
        norm_vb = hybrid_norms(torch.ones_like(snr_weight), count_norm, self.timesteps)[1] if learned else None
        ctx = Ctx.get(device)
        with ctx.scope():
            # the epsilon key is what it always was; a v program (q_sample_v, a target buffer) has its own
            film = bool(getattr(model, "use_scale_shift_norm", False))
            key = ("unet-train", ctx.device.index, B, d, h, w) + ((self.prediction_type,) if v_pred else ()) + (
                () if mode == "fast" else ("attn-" + mode,)) + (((film, drop_on),) if (film or drop_on) else ()) + (
                ("learn_sigma",) if learned else ())
            kw = dict(prediction=self.prediction_type) if v_pred else {}
            if drop_on:
                kw["dropout"] = True
            prog = cached_program(model, key, lambda: UNetTrainProgram(ctx, model, B, d, h, w, **kw))
            prog.set_diffusion(self)
            if drop_on:
                prog.set_dropout(drop_p, dropout_seed)
            if learned:
                prog.set_vb_norm(norm_vb)
        if pred_request is not None:      # the same forward launches, then ctsi_z0_pred; two differentiable outputs
            from .train_engine import train_step_pred
            loss, pred_request["z0_pred"] = train_step_pred(prog, z_0.detach().float(), c.detach().float(), t, noise.float(),
                                                            norm, m, pred_request["active"])
        else:
            loss = train_step(prog, z_0.detach().float(), c.detach().float(), t, noise.float(), norm, m)
        loss_dict = {'mse': loss.item()}
        if learned:       # the program's loss_out = {total, mse, vb, ...}: 'mse' keeps its meaning, 'vb' = lambda L_vb (bits)
            parts = prog.loss_out[1:3].tolist()
            loss_dict = {'mse': parts[0], 'vb': parts[1]}
        if keep is not None:
            loss_dict['cond_dropped'] = int((~keep).sum().item())
        prog.check_errors()     # (the stream is synchronised by the .item() above: a sticky split-K hand-off error of this forward,
                                #  or of the previous step's backward, surfaces here)
        # Optional MS-SSIM term (diffusion.py:204-240).  The reference decodes the predicted z_0 under torch.no_grad(), so the
        # term carries NO gradient: total = (1 - w) * mse + w * (1 - ms_ssim) scales the MSE gradient by (1 - w) and adds a
        # constant.  ms_ssim itself is `pytorch_msssim.ms_ssim` (requirements.txt:24, `pytorch-msssim>=1.0.0`), a third-party
        # package; where it is absent the reference prints the warning below and returns the MSE loss -- so does this
        # engine (model.forward never enables the term: models/model.py:218-219).
        if use_ssim and ssim_weight > 0.0 and vae is not None and v_gt is not None:
            try:
                from pytorch_msssim import ms_ssim
                with torch.no_grad():
                    z_t, _ = self.q_sample(z_0.detach().float(), t, noise.float())
                    eps = torch.empty((B, L, d, h, w), dtype=torch.float32, device=device)
                    with ctx.scope():
                        pred_nd = prog.eps
                        if learned:       # the prediction half of the 2L-channel head
                            pred_nd = torch.empty((B, d, h, w, L), dtype=torch.float32, device=device)
                            ctx.lib.sigma_split(C.c_void_p(prog.eps.data_ptr()), C.c_void_p(pred_nd.data_ptr()), None, B, 0, L,
                                                d, h, w, ctx.sptr)
                        ctx.lib.ndhwc_f32_to_ncdhw_f32(C.c_void_p(pred_nd.data_ptr()), C.c_void_p(eps.data_ptr()), B, L, d, h,
                                                       w, ctx.sptr)
                    z0_pred = (self._predict_z_0_from_v if v_pred else self._predict_z_0_from_noise)(z_t, t, eps)
                    # training keeps the bf16 programs whatever `vae.inference_precision` says
                    v_pred = vae._decode(z0_pred, "bf16") if hasattr(vae, "_decode") else vae.decode(z0_pred)
                    terms = []
                    for i in range(v_gt.shape[2]):
                        terms.append(1.0 - ms_ssim((v_pred[:, :, i] + 1.0) / 2.0, (v_gt[:, :, i].float() + 1.0) / 2.0,
                                                   data_range=1.0, size_average=True))
                    loss_ssim = torch.stack(terms).mean()
                loss_dict['ssim'] = loss_ssim.item()
                total = (1.0 - ssim_weight) * loss + ssim_weight * loss_ssim
                loss_dict['total'] = total.item()
                return total, loss_dict
            except ImportError:
                print("Warning: pytorch-msssim not installed. Falling back to MSE-only loss.")
            except Exception as e:
                print(f"Warning: MS-SSIM calculation failed: {e}. Using MSE-only loss.")
        loss_dict['total'] = loss.item() if learned else loss_dict['mse']
        return loss, loss_dict

    def training_loss_and_prediction(self, model, z_0, c, mask=None, t=None, noise=None, cond_drop_prob=0.0, cond_keep=None,
                                     active=None):
        """training_loss that also returns the clean latent its prediction stands for, with a gradient (additive; DESIGN
        section 27): (loss, loss_dict, z0_pred).  It IS training_loss -- the same body, the same draws from torch's generators
        in the same order, the same program, the same loss bits -- followed by one ctsi_z0_pred launch on the training
        program's own buffers: epsilon (z_t - sqrt(1 - abar_t) eps^) / sqrt(abar_t), v sqrt(abar_t) z_t - sqrt(1 - abar_t) v^,
        fp32, z_0's shape.  The gradient of z0_pred enters the U-Net backward through ctsi_loss_bwd_z0, added to the loss
        gradient in fp32 before the one rounding to bf16.  `active` (bool, (B,); None = every row): the rows that take part;
        the others come back as z_0 itself and carry no gradient (the epsilon form's d z0^ / d eps^ = -sqrt(1 / abar_t - 1)
        is unbounded as t -> T: callers gate on the SNR, see VideoToVideoDiffusion.image_loss_min_snr).  The loss `mask` acts
        on the MSE term only.  A learn_sigma model raises CtsiError: the hybrid loss has a backward kernel of its own."""
        if self._learned() or bool(getattr(model, "learn_sigma", False)):
            raise CtsiError("training_loss_and_prediction does not support learn_sigma models (var_type='learned_range'): the "
                            "hybrid loss has its own backward kernel, which takes no gradient of the predicted latent")
        if active is not None and (not torch.is_tensor(active) or active.dtype != torch.bool
                                   or tuple(active.shape) != (z_0.shape[0],)):
            raise ValueError(f"active must be a bool tensor of shape ({z_0.shape[0]},)")
        request = dict(active=active)
        self.__dict__["_pred_request"] = request
        try:
            loss, loss_dict = self.training_loss(model, z_0, c, mask=mask, t=t, noise=noise, cond_drop_prob=cond_drop_prob,
                                                 cond_keep=cond_keep)
        finally:
            self.__dict__.pop("_pred_request", None)
        return loss, loss_dict, request["z0_pred"]
