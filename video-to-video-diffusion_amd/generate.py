"""Batch inference helpers (mirror of reference inference/generate.py:98-226; the video-file I/O
wrapper `generate_video` of the legacy RGB path is out of scope)."""
from __future__ import annotations

import torch

from .sampler import SAMPLERS, check_guidance


def _sample(model, z_cond, sampler_type, num_inference_steps, device, progress, noise_fn=None, guidance_scale=1.0,
            guidance_rescale=0.0):
    return SAMPLERS[sampler_type](model.diffusion, model.unet, z_cond.shape, z_cond, num_inference_steps, device,
                                  progress=progress, noise_fn=noise_fn, guidance_scale=guidance_scale,
                                  guidance_rescale=guidance_rescale)


@torch.no_grad()
def generate_batch(model, input_videos, sampler_type='ddim', num_inference_steps=20, device='cuda',
                   noise_fn=None, guidance_scale=1.0, guidance_rescale=0.0):
    """encode -> sample at the input's latent shape (no depth change) -> decode (generate.py:98-155).
    sampler_type: 'ddim', 'ddpm' or (additive) 'dpmpp_2m' or 'heun'.  `guidance_scale` / `guidance_rescale` (additive):
    classifier-free guidance as in VideoToVideoDiffusion.generate; the VAE still runs once per clip."""
    if sampler_type not in SAMPLERS:
        raise ValueError(f"Unknown sampler type: {sampler_type}")
    check_guidance(guidance_scale, guidance_rescale)
    model.eval()
    model.to(device)
    input_videos = input_videos.to(device)
    print(f"Generating batch of {input_videos.shape[0]} videos...")
    z_in = model.vae.encode(input_videos)
    z_0 = _sample(model, z_in, sampler_type, num_inference_steps, device, True, noise_fn, guidance_scale,
                  guidance_rescale)
    return model.vae.decode(z_0)


@torch.no_grad()
def interpolate_videos(model, video_a, video_b, num_interpolations=5, sampler_type='ddim',
                       num_inference_steps=20, device='cuda', guidance_scale=1.0, guidance_rescale=0.0):
    """Latent-space lerp between two clips used as conditioning (generate.py:158-226).  `guidance_scale` /
    `guidance_rescale` (additive): classifier-free guidance of every interpolated sample."""
    check_guidance(guidance_scale, guidance_rescale)
    model.eval()
    model.to(device)
    z_a = model.vae.encode(video_a.unsqueeze(0).to(device))
    z_b = model.vae.encode(video_b.unsqueeze(0).to(device))
    outs = []
    for alpha in torch.linspace(0, 1, num_interpolations).to(device):
        z_mix = (1 - alpha) * z_a + alpha * z_b
        kind = 'ddim' if sampler_type == 'ddim' else 'ddpm'
        z_0 = _sample(model, z_mix, kind, num_inference_steps, device, False, None, guidance_scale, guidance_rescale)
        outs.append(model.vae.decode(z_0).squeeze(0))
    return outs
