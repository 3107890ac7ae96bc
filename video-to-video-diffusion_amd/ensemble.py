"""Ensemble sampling: the per-voxel mean and standard deviation of several draws of the sampler.

Every sampler is stochastic in its initial noise, and the thick input does not determine the thin volume: the mean of K draws
is the MMSE estimate, the per-voxel standard deviation says which voxels the input pins down, and its profile along depth
(`EnsembleResult.slice_std`) is the uncertainty per output slice.  `EnsembleAccumulator` folds decoded volumes into running
statistics with one streaming HIP pass per group of members (csrc/ensemble.hip: the sequential Welford recurrence, the same
bits whatever the grouping), so memory does not grow with K; `VideoToVideoDiffusion.generate_ensemble` drives it, sampling
the members as rows of one network batch.  There is no CPU path."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .lib import CtsiError


class _EnsembleFields(NamedTuple):
    mean: torch.Tensor
    std: torch.Tensor
    count: int
    slice_std: torch.Tensor
    members: Optional[torch.Tensor]


class EnsembleResult(_EnsembleFields):
    """mean, std: fp32 (N, C, D, H, W) on the device; count: the number of members; slice_std: float64 (N, C, D, 3) on the
    CPU -- mean std, rms std and max std over each output slice -- copied from the device when the field is read by name, not
    by the call that made the result; members: None or the decoded members, fp32 (K, N, C, D, H, W)."""
    __slots__ = ()

    @property
    def slice_std(self) -> torch.Tensor:
        return tuple.__getitem__(self, 3).cpu()


class EnsembleAccumulator:
    """Running per-voxel mean and sum of squared deviations of fp32 volumes.  `add` folds one volume (N, C, D, H, W) or a
    group (m, N, C, D, H, W) in one pass that reads the state once and writes it once; `result` may be called at any time
    and more members may follow it.  The launches go to the engine stream, outside any cached program."""

    def __init__(self):
        self.count = 0
        self._shape = None
        self._mean = self._m2 = None

    def add(self, volumes: torch.Tensor) -> "EnsembleAccumulator":
        from .engine import Ctx, _ptr
        if not torch.is_tensor(volumes) or volumes.dim() not in (5, 6):
            raise ValueError("add: expected one (N, C, D, H, W) volume or a group (m, N, C, D, H, W)")
        if not volumes.is_cuda:
            raise CtsiError("the ensemble statistics run on the HIP engine: pass ROCm tensors (there is no CPU path)")
        if volumes.dtype != torch.float32 or not volumes.is_contiguous():
            raise CtsiError(f"add works on a contiguous fp32 tensor, got {volumes.dtype}, "
                            f"contiguous={volumes.is_contiguous()}")
        shape = tuple(volumes.shape[-5:])
        rows = 1 if volumes.dim() == 5 else int(volumes.shape[0])
        if rows < 1 or 0 in shape:
            raise ValueError(f"add: an empty tensor {tuple(volumes.shape)}")
        if self._shape is None:
            self._shape = shape
            self._mean = torch.empty(shape, dtype=torch.float32, device=volumes.device)
            self._m2 = torch.empty(shape, dtype=torch.float32, device=volumes.device)
        elif shape != self._shape or volumes.device != self._mean.device:
            raise ValueError(f"add: members of shape {shape} on {volumes.device} after members of shape {self._shape} on "
                             f"{self._mean.device}")
        ctx = Ctx.get(volumes.device)
        with ctx.scope():
            ctx.lib.ensemble_accumulate(_ptr(volumes), rows, self._mean.numel(), self.count, _ptr(self._mean), _ptr(self._m2),
                                        ctx.sptr)
        for t in (volumes, self._mean, self._m2):
            t.record_stream(ctx.stream)
        self.count += rows
        return self

    def result(self, unbiased: bool = True, members: Optional[torch.Tensor] = None) -> EnsembleResult:
        """std = sqrt(m2 / (count - 1)) (`unbiased`, default) or sqrt(m2 / count), 0 for one member.  The mean is a copy and
        the std a new tensor: the accumulator stays valid.  `members` is passed through into the result."""
        from .engine import Ctx, _ptr
        if self.count < 1:
            raise ValueError("result: no member has been added")
        if not isinstance(unbiased, bool):
            raise ValueError(f"unbiased must be True or False, got {unbiased!r}")
        n, c, d, h, w = self._shape
        planes, plane = n * c * d, h * w
        ctx = Ctx.get(self._mean.device)
        dev = self._mean.device
        std = torch.empty(self._shape, dtype=torch.float32, device=dev)
        with ctx.scope():
            mean = self._mean.clone()
            partials = torch.empty(ctx.lib.ensemble_blocks(planes, plane) * 4, dtype=torch.float64, device=dev)
            table = torch.empty((planes, 3), dtype=torch.float64, device=dev)
            ctx.lib.ensemble_finalize(_ptr(self._m2), _ptr(std), self.count, int(unbiased), planes, plane, _ptr(partials),
                                      _ptr(table), ctx.sptr)
            prof = torch.stack([table[:, 0] / plane, (table[:, 1] / plane).sqrt(), table[:, 2]], dim=1).view(n, c, d, 3)
        for t in (std, self._m2, self._mean):
            t.record_stream(ctx.stream)
        return EnsembleResult(mean, std, self.count, prof, members)


def check_members(num_members, member_batch):
    """`num_members` an int >= 1, `member_batch` None or an int >= 1 (ValueError naming the value otherwise; a bool is not an
    int here)."""
    if isinstance(num_members, bool) or not isinstance(num_members, int) or num_members < 1:
        raise ValueError(f"num_members must be an integer >= 1, got {num_members!r}")
    if member_batch is not None and (isinstance(member_batch, bool) or not isinstance(member_batch, int) or member_batch < 1):
        raise ValueError(f"member_batch must be None or an integer >= 1, got {member_batch!r}")


def auto_member_batch(ctx, vae, shape, members: int, guided: bool = False) -> int:
    """How many members of decoded shape (N, C, D, H, W) go into one batch when the caller names none: the rule of
    sample_with_stitching's window batch (sampler._auto_window_batch: a fifth of the TOTAL device memory over the decoder's
    activations per member, so the batch shape and its cached programs stay the same from call to call)."""
    from .sampler import _auto_window_batch
    n, _, d, h, w = shape
    return _auto_window_batch(ctx, vae, int(n), int(d), int(h), int(w), int(members), guided)


def generate_ensemble(model, v_in, sampler, num_inference_steps=20, num_members=8, guidance_scale=1.0, target_depth=None,
                      member_noise_fn=None, precision=None, guidance_rescale=0.0, member_batch=None,
                      keep_members=False) -> EnsembleResult:
    """The body of `VideoToVideoDiffusion.generate_ensemble` (documented there)."""
    from .consistency import refuse_depth_sharding
    from .engine import Ctx
    from .engine_f32 import check_precision
    from .sampler import SAMPLERS, check_guidance
    check_members(num_members, member_batch)
    mg = getattr(model, "measurement_guidance", None)
    if mg is not None and mg.scale > 0.0:
        raise CtsiError("generate_ensemble does not support measurement_guidance: the members are rows of one sampler batch and "
                        "the guidance holds one thick volume per row; call generate() per member, or set "
                        "measurement_guidance = None")
    if member_noise_fn is not None and not callable(member_noise_fn):
        raise ValueError(f"member_noise_fn must be None or a callable (k, i, shape) -> noise, got "
                         f"{type(member_noise_fn).__name__}")
    check_guidance(guidance_scale, guidance_rescale)
    if precision is not None:
        check_precision(precision)
        saved = (model.unet.inference_precision, model.vae.inference_precision)
        model.unet.inference_precision = model.vae.inference_precision = precision
        try:
            return generate_ensemble(model, v_in, sampler, num_inference_steps, num_members, guidance_scale, target_depth,
                                     member_noise_fn, None, guidance_rescale, member_batch, keep_members)
        finally:
            model.unet.inference_precision, model.vae.inference_precision = saved
    if sampler not in SAMPLERS:
        raise ValueError(f"Unknown sampler: {sampler}")
    refuse_depth_sharding(model.unet, model.vae, feature="generate_ensemble")
    dc = model.data_consistency
    if dc is not None and target_depth is not None and int(target_depth) < int(v_in.shape[2]):
        raise ValueError(f"data_consistency: target_depth={int(target_depth)} is below the {int(v_in.shape[2])} input "
                         f"slices; a slice profile maps thin slices onto fewer thick ones")
    if not v_in.is_cuda:
        raise CtsiError("generate_ensemble runs on the HIP engine: move the input to a ROCm device")
    device = v_in.device
    ctx = Ctx.get(device)
    v_in, z_cond = model._encode_conditioning(ctx, v_in, target_depth)
    one = tuple(z_cond.shape)                      # (N, L, d, h, w): one member
    n = one[0]
    d_out = int(target_depth) if target_depth is not None else int(v_in.shape[2])
    out_shape = (n, int(v_in.shape[1]), d_out, int(v_in.shape[3]), int(v_in.shape[4]))
    guided = float(guidance_scale) != 1.0
    batch = member_batch if member_batch is not None else auto_member_batch(ctx, model.vae, out_shape, num_members, guided)
    batch = min(batch, num_members)
    group = min(batch, auto_member_batch(ctx, model.vae, out_shape, num_members))
    project = dc is not None and d_out != int(v_in.shape[2])
    if dc is not None and not project:
        model._warn_consistency_without_depth_change(v_in)
    if member_noise_fn is None:
        torch.randn(one, device=device)            # generate() draws (and discards) one latent: the same RNG stream
    acc, kept = EnsembleAccumulator(), []
    for k0 in range(0, num_members, batch):
        m = min(batch, num_members - k0)
        cond = z_cond if m == 1 else z_cond.repeat(m, 1, 1, 1, 1)      # member-major rows: k * N + b
        noise_fn = None
        if member_noise_fn is not None:
            def noise_fn(i, shape, k0=k0, m=m):
                rows = [member_noise_fn(k0 + j, i, one) for j in range(m)]
                return rows[0] if m == 1 else torch.cat([r.to(rows[0].device) for r in rows], dim=0)
        z_0 = SAMPLERS[sampler](model.diffusion, model.unet, (m * n,) + one[1:], cond, num_inference_steps, device,
                                noise_fn=noise_fn, guidance_scale=guidance_scale, guidance_rescale=guidance_rescale)
        for j0 in range(0, m, group):
            g = min(group, m - j0)
            v = model._decode_sanitised(ctx, z_0[j0 * n:(j0 + g) * n])
            if project:
                dc.project_(v, v_in if g == 1 else v_in.repeat(g, 1, 1, 1, 1))
            v = v.view((g, n) + tuple(v.shape[1:]))
            acc.add(v)
            if keep_members:
                kept.append(v)
    return acc.result(members=torch.cat(kept, dim=0) if keep_members else None)
