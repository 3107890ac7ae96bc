"""Measurement guidance: steer sampling toward the thick input.

The acquired thick slices are y = W x of the thin slices x the engine generates (consistency.SliceProfile).  On a chosen subset
of the U-Net evaluations the sampler's predicted clean latent z0 is decoded through the frozen VAE with a data-gradient tape
(vae.decode_with_grad), the residual r = y - W D(z0) is formed, and its gradient is taken back to the latent:

    g_z = grad_{z0} 1/2 ||r||^2 = -J_D^T W^T r,        dz0 = -zeta g_z / ||r||_2        (normalize='residual')

i.e. a step of length zeta along the gradient of the residual NORM (dz0 = -zeta g_z with normalize='none').  The update's
output becomes z' + kappa_e dz0, kappa_e being the weight of the data prediction in the sampler's own update, with the
predicted noise held fixed (MPGD / latent DPS without the U-Net Jacobian).  The correction is ADDED to the update's output: the
update's clip of z0 is not re-applied to z0 + dz0.  A data-prediction history (DPM-Solver++) receives dz0 as well.

The captured step graph is untouched; a guided evaluation runs three more kernels (csrc/measure_guide.hip) and the decoder
tape eagerly around its replay (sampler._run_step_program).  Nothing here synchronises.  Image quality is not measured by any of
this: that the correction is the stated gradient and lowers the stated functional holds whatever the weights.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .consistency import SliceProfile, _check_fwhm, _check_kind
from .lib import CtsiError

NORMALIZE = ("residual", "none")
GUIDED_KINDS = ("ddim", "ddpm", "dpmpp")
FEATURE = "measurement_guidance"


class MeasurementGuidance:
    """Guidance toward the thick input inside the sampling loop.  `kind`, `fwhm`, `matrix`: the slice profile, as for
    consistency.DataConsistency.  `scale` zeta >= 0 (0 disables: the launches and bits of a model without the attribute).
    Of E U-Net evaluations those from ceil(start (E - 1)) on are eligible, and every `every`-th of them, counted back from the
    LAST one, is guided (the last evaluation always is).  `normalize` 'residual': dz0 = -zeta grad ||r||_2; 'none':
    dz0 = -zeta grad 1/2 ||r||^2.  `last_stats`: float64 (guided evaluations, n) on the CPU, ||r||_2 of every sample before each
    correction of the last run; it is copied from the device when read, not by the run."""

    def __init__(self, kind="box", fwhm=None, matrix=None, scale=1.0, start=0.5, every=1, normalize="residual"):
        if matrix is None:
            fwhm = _check_fwhm(_check_kind(kind), fwhm)
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale < 0:
            raise ValueError(f"scale must be a finite number >= 0, got {scale!r}")
        if isinstance(start, bool) or not isinstance(start, (int, float)) or not 0.0 <= start <= 1.0:
            raise ValueError(f"start must lie in [0, 1], got {start!r}")
        if isinstance(every, bool) or not isinstance(every, int) or every < 1:
            raise ValueError(f"every must be an integer >= 1, got {every!r}")
        if normalize not in NORMALIZE:
            raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
        self.kind, self.fwhm, self.matrix = kind, fwhm, matrix
        self.scale, self.start, self.every, self.normalize = float(scale), float(start), every, normalize
        self._profiles: Dict[Tuple[int, int], SliceProfile] = {}
        self._stats_dev: Optional[torch.Tensor] = None

    def guided_evaluations(self, evaluations: int) -> Tuple[int, ...]:
        """The indices of the guided ones among `evaluations` U-Net evaluations, ascending.  Pure host code."""
        if isinstance(evaluations, bool) or not isinstance(evaluations, (int, np.integer)) or evaluations < 1:
            raise ValueError(f"the number of evaluations must be an integer >= 1, got {evaluations!r}")
        E = int(evaluations)
        if self.scale == 0.0:
            return ()
        first = int(math.ceil(self.start * (E - 1)))
        return tuple(sorted(range(E - 1, first - 1, -self.every)))

    def profile(self, d_in: int, d_out: int) -> SliceProfile:
        key = (int(d_in), int(d_out))
        if key not in self._profiles:
            self._profiles[key] = SliceProfile(key[0], key[1], self.kind, self.fwhm, self.matrix)
        return self._profiles[key]

    @property
    def last_stats(self) -> Optional[torch.Tensor]:
        return None if self._stats_dev is None else self._stats_dev.sqrt().cpu()

    def bind(self, y: torch.Tensor, vae) -> "Measurement":
        """What the samplers' sample(measurement=) and sampler.measurement_scope take: this object, the thick volume and the
        decoder."""
        return Measurement(self, y, vae)


class Measurement(NamedTuple):
    guidance: MeasurementGuidance
    y: torch.Tensor               # the sanitised thick input (N, C, d_in, H, W)
    vae: object                   # the frozen VAE whose decode maps the latent to the thin volume


def check_measurement_guidance(value):
    """What `model.measurement_guidance` accepts: a MeasurementGuidance or None (ValueError otherwise)."""
    if value is not None and not isinstance(value, MeasurementGuidance):
        raise ValueError(f"measurement_guidance must be None or a MeasurementGuidance, got {type(value).__name__}")
    return value


def measurement_guidance_from_config(config) -> Optional[MeasurementGuidance]:
    """The additive top-level section `measurement_guidance: {enabled: true, kind, fwhm, scale, start, every, normalize}`; read
    only when `enabled` is a real `true`.  Bad values raise ValueError."""
    sec = config.get("measurement_guidance", None)
    if not isinstance(sec, dict) or sec.get("enabled", False) is not True:
        return None
    unknown = set(sec) - {"enabled", "kind", "fwhm", "scale", "start", "every", "normalize"}
    if unknown:
        raise ValueError(f"measurement_guidance: unknown key(s) {sorted(unknown)}")
    return MeasurementGuidance(kind=sec.get("kind", "box"), fwhm=sec.get("fwhm", None), scale=sec.get("scale", 1.0),
                               start=sec.get("start", 0.5), every=sec.get("every", 1),
                               normalize=sec.get("normalize", "residual"))


def kappa_rows(diffusion, kind: str, t_desc: Sequence[int], order: int = 2) -> np.ndarray:
    """kappa_e, float64, one per evaluation: the weight of the data prediction in the update of sampler `kind` on the
    timesteps `t_desc`, from `alphas_cumprod` and independent of the update form.
      'ddim'   sqrt(abar_next), 1 after the last step (the predicted noise is held fixed)
      'ddpm'   posterior_mean_coef1[t]
      'dpmpp'  the coefficient b_e of the current data prediction in sampler.dpm_coef_rows."""
    idx = [int(t) for t in t_desc]
    ac = diffusion.alphas_cumprod.detach().double().cpu().numpy()
    if kind == "ddim":
        return np.sqrt(np.append(ac[idx][1:], 1.0))
    if kind == "ddpm":
        return diffusion.posterior_mean_coef1.detach().double().cpu().numpy()[idx]
    if kind == "dpmpp":
        from .sampler import dpm_coef_rows
        with np.errstate(divide="ignore", invalid="ignore"):
            return dpm_coef_rows(diffusion.alphas_cumprod, idx, order, torch.float64)[:, 3].numpy().copy()
    raise CtsiError(_refusal(f"the sampler kind {kind!r}", "sample with 'ddim', 'ddpm' or 'dpmpp_2m'"))


def z0_rows(plan) -> np.ndarray:
    """(E, 4) float32 rows {alpha, sigma, mode, clip} of ctsi_guide_z0, taken from the coefficient rows the update itself reads
    (sampler.StepPlan.coef), so both form the same data prediction: the eps-form DDIM / DDPM rows divide (mode 0; clip 10 / 1),
    the eps-form DPM-Solver++ rows hold 1 / alpha and sigma / alpha (mode 1; clip 10), the x0-form rows alpha, sigma and
    their own clip (mode 1)."""
    coef = plan.coef.detach().float().cpu().numpy()
    rows = np.zeros((coef.shape[0], 4), dtype=np.float32)
    if plan.x0:
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = coef[:, 0], coef[:, 1], 1.0, coef[:, 6]
    elif plan.kind == "dpmpp":
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = coef[:, 0], coef[:, 1], 1.0, 10.0
    else:
        rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = coef[:, 1], coef[:, 0], 0.0, (1.0 if plan.kind == "ddpm" else 10.0)
    return rows


def _refusal(what: str, alternative: str) -> str:
    return f"{FEATURE} does not support {what}; {alternative}, or set measurement_guidance = None"


def refuse_unguidable_model(model, sampler: str, precision: str):
    """What generate() refuses with the attribute set, before any device work (CtsiError, each naming the alternative)."""
    if sampler == "heun":
        raise CtsiError(_refusal("the 'heun' sampler (two evaluations share one step)", "sample with 'ddim', 'ddpm' or "
                                 "'dpmpp_2m'"))
    if sampler == "ddpm_spaced":
        raise CtsiError(_refusal("the strided ancestral sampler 'ddpm_spaced'", "sample with 'ddpm', 'ddim' or 'dpmpp_2m'"))
    if getattr(model.unet, "learn_sigma", False) or getattr(model.diffusion, "var_type", "fixed_small") != "fixed_small":
        raise CtsiError(_refusal("a learned reverse variance (learn_sigma / var_type='learned_range')",
                                 "use a fixed_small model"))
    refuse_unguidable_run(model.unet, model.vae, precision)


def refuse_unguidable_run(unet, vae, precision: str, kind: Optional[str] = None, learned: bool = False):
    """The refusals run_sampler repeats for a direct caller (CtsiError)."""
    if kind is not None and kind not in GUIDED_KINDS or learned:
        raise CtsiError(_refusal(f"the sampler kind {kind!r}" + (" with a learned variance" if learned else ""),
                                 "sample with 'ddim', 'ddpm' or 'dpmpp_2m' on a fixed_small model"))
    if not (type(unet).__name__ == "UNet3D" and hasattr(unet, "program")):
        raise CtsiError(_refusal("a generic model(z, t, c) callable (the correction runs around the engine's step program)",
                                 "pass the engine's UNet3D"))
    if precision != "bf16":
        raise CtsiError(_refusal(f"the {precision} inference precision (the decoder's gradient tape is a bf16 program)",
                                 "set inference_precision='bf16'"))
    for m in (unet, vae):
        if getattr(m, "depth_shard_comm", None) is not None:
            raise CtsiError(_refusal("depth sharding (depth_shard_comm): a depth column spans ranks", "drop the communicator"))
    if int(getattr(vae, "latent_dim", 0)) % 8 != 0:
        raise CtsiError(_refusal(f"latent_dim={getattr(vae, 'latent_dim', None)} (the decoder's gradient tape needs a multiple "
                                 "of 8)", "use a latent_dim that is a multiple of 8"))


class GuideRun:
    """One sampling run's guidance on a step program: which evaluations, their kappa and z0 rows, the device operands.
    `correct(e)` is issued behind the replay of a guided evaluation e, on the engine stream."""

    def __init__(self, measurement: Measurement, diffusion, plan, order: int, ctx, shape):
        mg, y, vae = measurement
        n, L, d, h, w = [int(v) for v in shape]
        if not (torch.is_tensor(y) and y.dim() == 5 and int(y.shape[0]) == n):
            raise ValueError(f"measurement: the thick volume must be a ({n}, C, d_in, H, W) tensor, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        self.mg, self.vae, self.ctx = mg, vae, ctx
        self.shape = (n, L, d, h, w)
        self.evals = mg.guided_evaluations(len(plan.t))
        self.slot = {e: i for i, e in enumerate(self.evals)}
        self.kappa = kappa_rows(diffusion, plan.kind, plan.t, order)
        self.rows = z0_rows(plan)
        self.profile = mg.profile(int(y.shape[2]), d)
        self.y = y.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
        dev = ctx.device
        c, hw = int(y.shape[1]), int(y.shape[3]) * int(y.shape[4])
        self.c, self.hw = c, hw
        self.z0 = torch.empty(self.shape, dtype=torch.float32, device=dev).requires_grad_(True)
        self.partials = torch.empty(max(ctx.lib.depth_project_blocks(n * c, hw), 1), dtype=torch.float64, device=dev)
        self.sumsq = torch.zeros((max(len(self.evals), 1), n), dtype=torch.float64, device=dev)
        mg._stats_dev = self.sumsq[:len(self.evals)]

    def save_state(self, prog):
        """Before the replay: the state the update is about to read, into the scratch buffer the program owns."""
        prog.guide_scratch().copy_(prog.z)

    def correct(self, prog, e: int):
        """Behind the replay of guided evaluation e: z0 -> decode -> g_x and sum r^2 -> decoder backward -> apply."""
        self.form_z0(prog, e)
        with torch.enable_grad():
            x = self.vae.decode_with_grad(self.z0)
        g_x = self.residual(x, e)
        g_z, = torch.autograd.grad(x, self.z0, g_x)
        self.apply(prog, e, g_z)

    def form_z0(self, prog, e: int):
        from .engine import _ptr
        n, L, d, h, w = self.shape
        alpha, sigma, mode, clip = (float(v) for v in self.rows[e])
        self.ctx.lib.guide_z0(_ptr(prog.guide_z), _ptr(prog.eps), alpha, sigma, int(mode), clip, _ptr(self.z0), n, L, d, h, w,
                              self.ctx.sptr)

    def _sumsq(self, e: int):
        import ctypes as C
        return C.c_void_p(self.sumsq.data_ptr() + self.slot[e] * self.shape[0] * 8)

    def residual(self, x: torch.Tensor, e: int) -> torch.Tensor:
        """g_x = -W^T (y - W x) of the decoded volume, and sum r^2 per sample into the evaluation's statistics row."""
        from .engine import _ptr
        n, _, d, _, _ = self.shape
        if tuple(x.shape) != (n, self.c, d) + tuple(self.y.shape[3:]):
            raise ValueError(f"measurement: the decoded volume {tuple(x.shape)} and the thick volume {tuple(self.y.shape)} "
                             f"differ outside depth")
        xd = x.detach().contiguous()
        g_x = torch.empty_like(xd)
        W32, _, band_w, _ = self.profile.device_tables(self.ctx.device)
        self.ctx.lib.depth_residual_adj(_ptr(xd), _ptr(self.y), _ptr(W32), _ptr(band_w), _ptr(g_x), _ptr(self.partials),
                                        self._sumsq(e), n, self.c, self.profile.d_in, d, self.hw, self.ctx.sptr)
        return g_x

    def apply(self, prog, e: int, g_z: torch.Tensor):
        from .engine import _ptr
        lib, sptr = self.ctx.lib, self.ctx.sptr
        n, L, d, h, w = self.shape
        g_z = g_z.contiguous()
        kappa = float(self.kappa[e])
        zin, c_total, nbytes, f32 = prog._sampler_zin()        # the operands of the update itself: the z slice starts the voxel
        if f32 or nbytes != 2:
            raise CtsiError(_refusal("a step program with an fp32 network input", "set inference_precision='bf16'"))
        lib.guide_apply(_ptr(prog.z), _ptr(prog.hist), _ptr(g_z), self._sumsq(e), -self.mg.scale * kappa, -self.mg.scale,
                        1 if self.mg.normalize == "residual" else 0, zin, c_total, 0, n, L, d, h, w, sptr)
        prog.xin.dirty = True
        if prog.guided:         # the input fan-out of a classifier-free-guidance program, once more: rows [n, 2n) see the new z
            lib.cfg_mirror(zin, prog._uncond_zin(), n * d * h * w, L * nbytes, c_total * nbytes, sptr)
