"""VideoToVideoDiffusion façade (mirror of reference models/model.py): config parsing, module
construction, `generate`, checkpoint layout.  Inference runs entirely on the HIP engine."""
from __future__ import annotations

import logging
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .consistency import check_data_consistency, data_consistency_from_config, refuse_depth_sharding
from .diffusion import GaussianDiffusion
from .engine import Ctx, check_attention_mode, nan_to_num_, trilinear_depth
from .engine_f32 import check_precision
from .lib import CtsiError
from .measurement_guidance import (check_measurement_guidance, measurement_guidance_from_config,
                                   refuse_unguidable_model)
from .sampler import SAMPLERS, check_guidance
from .unet3d import UNet3D
from .vae import VideoVAE

logger = logging.getLogger(__name__)


def _config_bool(config, key, default):
    """A config key that must hold a real bool (YAML `true` / `false`): a string such as 'false' would otherwise count as true."""
    v = config.get(key, default)
    if not isinstance(v, bool):
        raise ValueError(f"{key} must be true or false, got {v!r}")
    return v


def check_image_loss_min_snr(v) -> float:
    """`image_loss_min_snr` must be a finite number > 0 (ValueError otherwise): 1 / sqrt(min_snr) bounds the factor
    sqrt(1 / abar_t - 1) by which the epsilon form turns a gradient of the predicted latent into one of the prediction."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"image_loss_min_snr must be a finite number > 0, got {v!r}")
    return float(v)


def image_loss_rows(diffusion, t: torch.Tensor, min_snr: float) -> torch.Tensor:
    """The rows of a batch that take part in the image-space loss terms: abar_t / (1 - abar_t) >= min_snr, decided in float64
    on `alphas_cumprod` without the division (bool, t's shape and device)."""
    ab = diffusion.alphas_cumprod.detach().double().to(t.device)[t.long()]
    return ab >= check_image_loss_min_snr(min_snr) * (1.0 - ab)


def image_loss_from_config(config):
    """(image_loss, image_loss_min_snr) of a config.  The reference's `losses:` section is honoured only when it carries the
    additive key `apply_image_losses: true` (a real bool); without the key the section is ignored, as it always was."""
    sec = config.get('losses', None)
    if not isinstance(sec, dict) or not _config_bool(sec, 'apply_image_losses', False):
        return None, 1.0
    from .losses import CombinedLoss
    for key in ('perceptual_every_n_steps', 'ssim_every_n_steps'):
        v = sec.get(key, 10)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"losses.{key} must be an integer >= 1, got {v!r}")
    lam = {}
    for key in ('lambda_perceptual', 'lambda_ssim'):
        v = sec.get(key, 0.1)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"losses.{key} must be a finite number >= 0, got {v!r}")
        lam[key] = float(v)
    loss = CombinedLoss(lam['lambda_perceptual'] if _config_bool(sec, 'use_perceptual_loss', False) else 0.0,
                        lam['lambda_ssim'] if _config_bool(sec, 'use_ms_ssim_loss', False) else 0.0,
                        sec.get('perceptual_every_n_steps', 10), sec.get('ssim_every_n_steps', 10))
    return loss, check_image_loss_min_snr(sec.get('image_loss_min_snr', 1.0))


class VideoToVideoDiffusion(nn.Module):
    def __setattr__(self, name, value):
        # `image_loss` stays OUT of the module tree even when it is an nn.Module (a CombinedLoss): the model's parameters, its
        # state dict and its checkpoints keep their layout, and a VGG-19 inside the loss is not saved with every checkpoint
        if name == "image_loss":
            if value is not None and not callable(value):
                raise ValueError(f"image_loss must be None or a callable (pred, target, diffusion_loss, "
                                 f"compute_auxiliary=True) -> (total, dict), got {type(value).__name__}")
            self.__dict__["image_loss"] = value
            return
        # `data_consistency` is a plain attribute too: never a submodule, never in the state dict
        if name == "data_consistency":
            self.__dict__["data_consistency"] = check_data_consistency(value)
            return
        # and so is `measurement_guidance`
        if name == "measurement_guidance":
            self.__dict__["measurement_guidance"] = check_measurement_guidance(value)
            return
        super().__setattr__(name, value)

    def __init__(self, config, load_pretrained=False):
        super().__init__()
        pre = config.get('pretrained', {})
        use_pretrained = pre.get('use_pretrained', False) or load_pretrained
        grad_ckpt = config.get('hardware', {}).get('gradient_checkpointing',
                                                   config.get('gradient_checkpointing', False))
        # VAE keys are looked up inside config['model'] first, then at top level (model.py:58-62, 86-90)
        mc = config.get('model', config)

        def vae_arg(key, default):
            return mc.get(key, config.get(key, default))

        pre_vae = pre.get('vae', {})
        if use_pretrained and pre_vae.get('enabled', False):
            if pre_vae.get('checkpoint_path'):
                defaults = dict(in_channels=1, vae_base_channels=128, latent_dim=8, vae_scaling_factor=1.0)
            elif pre_vae.get('model_name'):
                VideoVAE.from_pretrained(pre_vae['model_name'])  # raises NotImplementedError (vae.py:308-321)
                defaults = {}
            else:
                raise ValueError("VAE enabled but neither checkpoint_path nor model_name specified in config")
        else:
            defaults = dict(in_channels=3, vae_base_channels=64, latent_dim=4, vae_scaling_factor=0.18215)
        self.vae = VideoVAE(in_channels=vae_arg('in_channels', defaults['in_channels']),
                            latent_dim=vae_arg('latent_dim', defaults['latent_dim']),
                            base_channels=vae_arg('vae_base_channels', defaults['vae_base_channels']),
                            scaling_factor=vae_arg('vae_scaling_factor', defaults['vae_scaling_factor']),
                            gradient_checkpointing=grad_ckpt)
        # U-Net keys are read from the TOP level of the config only (model.py:103-112): a YAML that nests
        # them under `model:` silently gets the defaults below.  Kept so checkpoint['config'] rebuilds
        # the same network.
        self.unet = UNet3D(latent_dim=self.vae.latent_dim,
                           model_channels=config.get('unet_model_channels', 128),
                           num_res_blocks=config.get('unet_num_res_blocks', 2),
                           attention_levels=config.get('unet_attention_levels', [1, 2]),
                           channel_mult=tuple(config.get('unet_channel_mult', [1, 2, 4, 4])),
                           num_heads=config.get('unet_num_heads', 4),
                           time_embed_dim=config.get('unet_time_embed_dim', 512),
                           use_checkpoint=grad_ckpt,
                           # additive keys, top level like every U-Net key (UNet3D's docstring): the
                           # ResBlocks' time conditioning (a real bool; anything else is a ValueError) and their
                           # training-time dropout probability in [0, 1) (validated by UNet3D)
                           use_scale_shift_norm=_config_bool(config, 'unet_use_scale_shift_norm', False),
                           dropout=config.get('unet_dropout', 0.0),
                           # additive key: a 2L-channel head whose second half is the learned variance
                           learn_sigma=_config_bool(config, 'unet_learn_sigma', False),
                           # additive key: the levels that carry in-plane SpatialAttention blocks
                           spatial_attention_levels=config.get('unet_spatial_attention_levels', ()))
        # additive key, top level like every U-Net key: how TemporalAttention is evaluated -- 'fast' (default) / 'exact': the
        # reference's einsum as written (a depth sum); 'softmax': true attention over depth (UNet3D's docstring)
        self.unet.attention_mode = check_attention_mode(config.get('unet_attention_mode', 'fast'))
        self.diffusion = GaussianDiffusion(noise_schedule=config.get('noise_schedule', 'cosine'),
                                           timesteps=config.get('diffusion_timesteps', 1000),
                                           beta_start=config.get('beta_start', 0.0001),
                                           beta_end=config.get('beta_end', 0.02),
                                           # additive key, top level like `noise_schedule`: 'epsilon' | 'v_prediction'
                                           prediction_type=config.get('prediction_type', 'epsilon'))
        # additive key, top level: `var_type` 'fixed_small' | 'learned_range'; the latter needs
        # `unet_learn_sigma: true` and the former forbids it (ValueError here, CtsiError at first use elsewhere)
        from .learned_sigma import check_var_type, pairing_error
        self.diffusion.var_type = check_var_type(config.get('var_type', 'fixed_small'))
        if pairing_error(self.diffusion.var_type, self.unet.learn_sigma):
            raise ValueError(pairing_error(self.diffusion.var_type, self.unet.learn_sigma))
        # additive keys, top level like `prediction_type`: `update_form` 'eps' | 'x0', `loss_weighting`
        # 'min_snr' | 'uniform', and `zero_terminal_snr: true`, which rescales the schedule (and sets update_form 'x0')
        from .x0_form import check_loss_weighting, check_update_form
        self.diffusion.update_form = check_update_form(config.get('update_form', 'eps'), self.diffusion.prediction_type)
        self.diffusion.loss_weighting = check_loss_weighting(config.get('loss_weighting', 'min_snr'))
        if config.get('zero_terminal_snr', False):
            self.diffusion.rescale_zero_terminal_snr()
        self.config = config
        self.use_pretrained = use_pretrained
        # additive key, top level like every U-Net / diffusion key: the conditioning-dropout probability of `forward`
        self.cond_drop_prob = float(config.get('cond_drop_prob', 0.0))
        if not 0.0 <= self.cond_drop_prob <= 1.0:
            raise ValueError(f"cond_drop_prob must lie in [0, 1], got {config.get('cond_drop_prob')!r}")
        # additive key: the arithmetic of generate() / the samplers / encode / decode ('bf16' default, 'fp32' or 'bf16x3')
        self.set_inference_precision(config.get('hardware', {}).get('inference_precision', 'bf16'))
        # image-space loss terms of `forward`, plain attributes: `image_loss` -- None (default) or a callable
        # with CombinedLoss.forward's signature -- and the SNR gate of the rows that take part.  From the config only when its
        # `losses:` section says `apply_image_losses: true`.
        self.image_loss, self.image_loss_min_snr = image_loss_from_config(config)
        # data consistency of generate(), a plain attribute: None (default) or a consistency.DataConsistency.
        # From the config only when its additive `data_consistency:` section says `enabled: true`.
        self.data_consistency = data_consistency_from_config(config)
        self._consistency_warned = False
        # measurement guidance of generate(), a plain attribute: None (default) or a
        # measurement_guidance.MeasurementGuidance.  From the config only when its additive `measurement_guidance:` section
        # says `enabled: true`.
        self.measurement_guidance = measurement_guidance_from_config(config)
        self._guidance_warned = False

    def set_inference_precision(self, precision):
        """'bf16' (default), 'fp32' or 'bf16x3' (fp32 tensors, split-bf16 MFMA convolutions: engine_x3.py): sets `unet.inference_precision` and `vae.inference_precision`, i.e. the arithmetic
        of generate(), the samplers and VAE encode / decode (engine_f32.py: fp32 activations, fp32 MFMA operands, the
        reference's fp32 inference of models/model.py:254-259).  Training (`forward`) keeps its bf16 programs."""
        check_precision(precision)
        self.unet.inference_precision = precision
        self.vae.inference_precision = precision

    def invalidate_engine_cache(self):
        """Drop the engine's cached programs (packed bf16 weights, captured graphs) -- needed only after weight
        writes torch cannot observe (`p.data[...] = ...`, raw-pointer copies); optimizer steps, `load_state_dict`
        and replaced parameters are detected automatically (engine.Program._fingerprint)."""
        from .engine import invalidate_engine_cache
        invalidate_engine_cache(self)

    def encode_videos(self, v_in, v_gt=None):
        z_in = self.vae.encode(v_in)
        if v_gt is not None:
            return z_in, self.vae.encode(v_gt)
        return z_in

    def decode_latent(self, z):
        return self.vae.decode(z)

    def forward(self, v_in, v_gt, mask=None, t=None, noise=None, cond_keep=None):
        """Training forward (model.py:158-228): frozen-VAE encode of both volumes, depth upsample of the
        conditioning when the depths differ, then `diffusion.training_loss` on the HIP engine.  Returns
        (loss, metrics); `loss.backward()` runs the engine's backward.  `t=` / `noise=` are test hooks.
        In training mode every sample's conditioning is replaced by the null conditioning (zeros) with the probability
        of the top-level config key `cond_drop_prob` (default 0: never, and no random number is drawn), which is what
        classifier-free guidance at sampling time needs; `cond_keep` (bool, (B,)) injects the mask instead."""
        if not v_in.is_cuda:
            raise CtsiError("the training forward runs on the HIP engine: move the inputs to a ROCm device")
        ctx = Ctx.get(v_in.device)
        with torch.no_grad():
            # training keeps the bf16 programs whatever `inference_precision` says
            z_in = self.vae._encode(v_in, "bf16")
            z_gt = self.vae._encode(v_gt, "bf16")
            if z_in.shape[2] != z_gt.shape[2]:
                with ctx.scope():
                    z_cond = trilinear_depth(ctx, z_in, int(z_gt.shape[2]))
                z_mask = None
                if mask is not None:   # nearest-neighbour pick of the (B, C, T) mask at the latent depth (model.py:205-212)
                    z_mask = F.interpolate(mask.float().unsqueeze(-1).unsqueeze(-1), size=(z_gt.shape[2], 1, 1),
                                           mode='nearest').squeeze(-1).squeeze(-1)
            else:
                z_cond, z_mask = z_in, mask
        if self.image_loss is not None:
            return self._forward_image_loss(v_gt, z_gt, z_cond, z_mask, t, noise, cond_keep)
        loss, loss_dict = self.diffusion.training_loss(self.unet, z_gt, z_cond, mask=z_mask, vae=self.vae, v_gt=v_gt,
                                                       use_ssim=False, ssim_weight=0.0, t=t, noise=noise,
                                                       cond_drop_prob=self.cond_drop_prob, cond_keep=cond_keep)
        return loss, {'loss': loss.item(), **loss_dict}

    def _forward_image_loss(self, v_gt, z_gt, z_cond, z_mask, t, noise, cond_keep):
        """`forward` with `image_loss` set: the diffusion loss and the predicted clean latent of the rows
        whose SNR passes `image_loss_min_snr` (training_loss_and_prediction), those rows decoded through the frozen VAE with a
        data-gradient tape (vae.decode_with_grad), then `total, d = image_loss(pred, v_gt[rows], loss)`.  Returns
        (total, {**the plain metrics, **d, 'image_rows': k}).  Only the k active rows are decoded.  The term is skipped --
        `image_loss(None, None, loss, compute_auxiliary=False)`, no prediction, no decode -- when no row is active or when a
        CombinedLoss has no auxiliary term due at its current step (losses.auxiliary_due).  Under torch.no_grad() the term is
        evaluated through the plain decode and nothing is kept.  The loss `mask` acts on the MSE term only: the image term
        compares whole decoded rows.  t is drawn here, where training_loss would draw it (first, from the same generator)."""
        from .losses import auxiliary_due
        fn, kw = self.image_loss, dict(cond_drop_prob=self.cond_drop_prob, cond_keep=cond_keep)
        if t is None:
            t = torch.randint(0, self.diffusion.timesteps, (z_gt.shape[0],), device=z_gt.device, dtype=torch.long)
        rows = image_loss_rows(self.diffusion, t, self.image_loss_min_snr)
        k = int(rows.sum().item())
        if k == 0 or not auxiliary_due(fn):
            loss, loss_dict = self.diffusion.training_loss(self.unet, z_gt, z_cond, mask=z_mask, t=t, noise=noise, **kw)
            total, d = fn(None, None, loss, compute_auxiliary=False)
            return total, {'loss': loss.item(), **loss_dict, **d, 'image_rows': k}
        loss, loss_dict, z0_pred = self.diffusion.training_loss_and_prediction(self.unet, z_gt, z_cond, mask=z_mask, t=t,
                                                                               noise=noise, active=rows, **kw)
        idx = rows.nonzero().flatten()
        pred = self.vae.decode_with_grad(z0_pred.index_select(0, idx))
        total, d = fn(pred, v_gt.index_select(0, idx).float(), loss)
        return total, {'loss': loss.item(), **loss_dict, **d, 'image_rows': k}

    @torch.no_grad()
    def generate(self, v_in, sampler, num_inference_steps=20, guidance_scale=1.0, target_depth=None,
                 noise_fn=None, precision=None, guidance_rescale=0.0):
        """thick slices (B, C, T_in, H, W) -> thin slices (B, C, T_out, H, W), fp32.

        encode -> trilinear depth upsample of the conditioning -> DDIM/DDPM -> decode, with the
        reference's nan_to_num guards applied unconditionally on device (model.py:230-343).
        `guidance_scale` s is honoured (the reference accepts and ignores it): classifier-free guidance against the null
        conditioning, the all-zero latent -- eps = eps_u + s (eps_c - eps_u), both from ONE batch-2n U-Net evaluation per
        step (sampler.run_sampler).  1.0 (default) is the unguided path, bit for bit; 0 samples
        unconditionally.  `guidance_rescale` phi in [0, 1] (additive, default 0) rescales eps to the conditional branch's
        per-sample standard deviation: eps <- phi eps std(eps_c) / std(eps) + (1 - phi) eps.  Encode, depth upsample and
        decode run once per volume.  Only a model trained with `cond_drop_prob` > 0 has seen the null conditioning.
        `sampler` also accepts 'ddpm_spaced' (additive): the ancestral sampler on `num_inference_steps` strided steps
        (sampler.DDPMSampler.sample(num_inference_steps=); 'ddpm' keeps walking all of them and ignores the count), 'dpmpp_2m' (additive): DPM-Solver++(2M) with `num_inference_steps` steps
        (sampler.DPMSolverSampler), e.g. 20 steps in place of DDIM-50, and 'heun' (additive): EDM Heun with
        `num_inference_steps` steps on Karras sigmas, 2 N - 1 U-Net evaluations (sampler.HeunSampler).
        `precision` (additive, default None = the models' `inference_precision` attributes): 'bf16', 'fp32' or 'bf16x3' for this
        call only; the attributes are restored afterwards.
        With `self.data_consistency` set (a consistency.DataConsistency; default None: the launches and bits of a model without it) and a
        `target_depth` that changes the depth, the decoded, sanitised volume is projected onto the sanitised `v_in` as the last
        device step; when the depth does not change the attribute has no effect and one warning says so.
        With `self.measurement_guidance` set (a measurement_guidance.MeasurementGuidance of scale > 0; default None: the launches
        and bits of a model without it) and a `target_depth` that changes the depth, the guidance's evaluations are steered
        toward the sanitised `v_in` through the frozen decoder: samplers 'ddim', 'ddpm' and 'dpmpp_2m', bf16,
        unsharded, fixed_small (CtsiError otherwise, before any device work); an unchanged depth warns once and has no effect.
        Together with `data_consistency` the projection stays the last device step."""
        check_guidance(guidance_scale, guidance_rescale)
        if precision is not None:
            check_precision(precision)
            saved = (self.unet.inference_precision, self.vae.inference_precision)
            self.unet.inference_precision = self.vae.inference_precision = precision
            try:
                return self.generate(v_in, sampler, num_inference_steps, guidance_scale, target_depth, noise_fn,
                                     guidance_rescale=guidance_rescale)
            finally:
                self.unet.inference_precision, self.vae.inference_precision = saved
        if sampler not in SAMPLERS:
            raise ValueError(f"Unknown sampler: {sampler}")
        dc = self.data_consistency
        if dc is not None:      # what the projection refuses is refused before any work
            refuse_depth_sharding(self.unet, self.vae)
            if target_depth is not None and int(target_depth) < int(v_in.shape[2]):
                raise ValueError(f"data_consistency: target_depth={int(target_depth)} is below the {int(v_in.shape[2])} input "
                                 f"slices; a slice profile maps thin slices onto fewer thick ones")
        mg = self.measurement_guidance
        if mg is not None and mg.scale == 0.0:
            mg = None
        if mg is not None:      # what the guidance refuses is refused before any work
            for m in (self.vae, self.unet):
                refuse_unguidable_model(self, sampler, check_precision(getattr(m, "inference_precision", "bf16")))
            if target_depth is not None and int(target_depth) < int(v_in.shape[2]):
                raise ValueError(f"measurement_guidance: target_depth={int(target_depth)} is below the {int(v_in.shape[2])} "
                                 f"input slices; a slice profile maps thin slices onto fewer thick ones")
            if target_depth is None or int(target_depth) == int(v_in.shape[2]):
                self._warn_guidance_without_depth_change(v_in)
                mg = None
        if not v_in.is_cuda:
            raise CtsiError("generate runs on the HIP engine: move the input to a ROCm device")
        device = v_in.device
        ctx = Ctx.get(device)
        v_in, z_cond = self._encode_conditioning(ctx, v_in, target_depth)
        latent_shape = tuple(z_cond.shape)
        if noise_fn is None:
            torch.randn(latent_shape, device=device)  # model.py:303 draws (and discards) one latent
        z_0 = SAMPLERS[sampler](self.diffusion, self.unet, latent_shape, z_cond, num_inference_steps, device,
                                noise_fn=noise_fn, guidance_scale=guidance_scale,
                                guidance_rescale=guidance_rescale,
                                **({} if mg is None else dict(measurement=mg.bind(v_in, self.vae))))
        v_out = self._decode_sanitised(ctx, z_0)
        if dc is not None:
            if v_out.shape[2] != v_in.shape[2]:
                dc.project_(v_out, v_in)
            else:
                self._warn_consistency_without_depth_change(v_in)
        return v_out

    def _encode_conditioning(self, ctx, v_in, target_depth):
        """The head of generate() and generate_ensemble(): (sanitised fp32 v_in, conditioning latent) -- VAE encode, then the
        trilinear depth upsample when `target_depth` is given, with the nan_to_num guards on the device."""
        v_in = torch.nan_to_num(v_in.float(), nan=0.0)
        z_in = self.vae.encode(v_in)
        with ctx.scope():
            nan_to_num_(ctx, z_in)
            if target_depth is not None:
                z_cond = trilinear_depth(ctx, z_in, int(target_depth))
                nan_to_num_(ctx, z_cond)
            else:
                z_cond = z_in
        return v_in, z_cond

    def _decode_sanitised(self, ctx, z_0):
        """The tail of generate() and generate_ensemble(): nan_to_num on the sampled latent (in place), VAE decode, nan_to_num."""
        with ctx.scope():
            nan_to_num_(ctx, z_0)
        v_out = self.vae.decode(z_0)
        with ctx.scope():
            nan_to_num_(ctx, v_out)
        return v_out

    def _warn_consistency_without_depth_change(self, v_in):
        if not self._consistency_warned:
            self._consistency_warned = True
            logger.warning("data_consistency is set but generate() keeps the depth (%d slices): there is nothing to "
                           "project, the attribute has no effect", int(v_in.shape[2]))

    def _warn_guidance_without_depth_change(self, v_in):
        if not self._guidance_warned:
            self._guidance_warned = True
            logger.warning("measurement_guidance is set but generate() keeps the depth (%d slices): there is no slice profile "
                           "to guide toward, the attribute has no effect", int(v_in.shape[2]))

    @torch.no_grad()
    def generate_ensemble(self, v_in, sampler, num_inference_steps=20, num_members=8, guidance_scale=1.0, target_depth=None,
                          member_noise_fn=None, precision=None, guidance_rescale=0.0, member_batch=None, keep_members=False):
        """`num_members` draws of generate() folded into per-voxel statistics: an ensemble.EnsembleResult
        with the mean (the MMSE estimate), the standard deviation (unbiased; 0 for one member), the per-slice uncertainty
        profile `slice_std` and, with `keep_members=True`, the decoded members (K, N, C, D, H, W).

        `v_in` is sanitised and encoded and the conditioning is depth-upsampled ONCE.  The members are sampled `member_batch` at
        a time as rows of one sampler call -- shape (m N, L, d, h, w), the conditioning rows repeated, member-major (row
        k N + b) -- so guidance, v-prediction, the x0 form, learn_sigma, every sampler and the three precisions are the
        existing batch path.  They are decoded in groups; each group is sanitised, projected when `self.data_consistency` is
        set and the depth changes (a mean of consistent members is consistent), and folded into the running statistics by
        one streaming pass (ensemble.EnsembleAccumulator), so memory does not grow with `num_members`.  The default
        `member_batch` and the decode group follow sample_with_stitching's memory rule on the TOTAL device memory.

        Noise: `member_noise_fn(k, i, shape)` returns member k's noise of shape (N, L, d, h, w), i = -1 for the initial draw
        as with `noise_fn`; the result then depends on `member_batch` only through the batch-size dependence of the network
        arithmetic.  Without it the draws come from torch's generator, once per batch of members after one drawn-and-discarded
        latent: with `num_members=1` that is generate()'s RNG stream (one seed, the same bits); for more members the default
        RNG makes the result depend on `member_batch`.

        Checked before any work: `num_members` an int >= 1, `member_batch` None or an int >= 1 (ValueError), guidance,
        precision and the sampler name as in generate(), a CPU input (CtsiError), depth sharding (CtsiError: each rank holds
        a slab, not a volume)."""
        from .ensemble import generate_ensemble
        return generate_ensemble(self, v_in, sampler, num_inference_steps, num_members, guidance_scale, target_depth,
                                 member_noise_fn, precision, guidance_rescale, member_batch, keep_members)

    def save_checkpoint(self, path, optimizer=None, scheduler=None, scaler=None, epoch=None, global_step=None,
                        current_phase=None, best_loss=None, **kwargs):
        """Same dict layout as the reference (model.py:362-387).  Extra keyword arguments go into the dict as they are:
        `ema_state_dict=ema.state_dict()` (ema.EMAWeights) is what `load_model_from_checkpoint(..., use_ema=True)` reads."""
        ckpt = {'model_state_dict': self.state_dict(), 'config': self.config}
        for key, obj in (('optimizer_state_dict', optimizer), ('scheduler_state_dict', scheduler),
                         ('scaler_state_dict', scaler)):
            if obj is not None:
                ckpt[key] = obj.state_dict()
        for key, val in (('epoch', epoch), ('global_step', global_step), ('current_phase', current_phase),
                         ('best_loss', best_loss)):
            if val is not None:
                ckpt[key] = val
        ckpt.update(kwargs)
        torch.save(ckpt, path)
        print(f"Checkpoint saved to {path}")

    def count_parameters(self):
        total = sum(p.numel() for p in self.parameters())
        return {
            'total': total,
            'trainable': sum(p.numel() for p in self.parameters() if p.requires_grad),
            'vae': sum(p.numel() for p in self.vae.parameters()),
            'vae_trainable': sum(p.numel() for p in self.vae.parameters() if p.requires_grad),
            'unet': sum(p.numel() for p in self.unet.parameters() if p.requires_grad),
            'diffusion': 0,
        }
