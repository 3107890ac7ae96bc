"""Data consistency along depth: the slice-profile operator of the thick acquisition and the projection
of a generated thin volume onto the volumes that reproduce it.

`SliceProfile` holds W (d_in, d_out), float64, non-negative, rows summing to 1: y = W x along depth, in the geometry of the
trilinear depth upsample (align_corners=False).  With r = d_out / d_in, thick slice k is centred at thin coordinate
(k + 0.5) r - 0.5, its slab is [k r - 0.5, (k + 1) r - 0.5), and thin slice j occupies [j - 0.5, j + 0.5).
`DataConsistency.project` replaces x by x + P (y - W x), P = W^T (W W^T)^-1: the closest volume (least squares) with W x = y.
The device work is csrc/depth_consistency.hip; nothing here synchronises.  Image quality is not measured by any of this:
W x = y is a property of the output, whatever the weights.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .lib import CtsiError

MAX_D_IN, MAX_D_OUT = 64, 512
KINDS = ("box", "gaussian", "pick")
FWHM_TO_SIGMA = 2.35482
MAX_COND = 1e6


def _check_fwhm(kind, fwhm):
    if kind == "gaussian":
        if isinstance(fwhm, bool) or not isinstance(fwhm, (int, float)) or not math.isfinite(fwhm) or fwhm <= 0:
            raise ValueError(f"a gaussian slice profile needs fwhm, a finite number > 0 in thick-slice units, got {fwhm!r}")
        return float(fwhm)
    if fwhm is not None:
        raise ValueError(f"fwhm belongs to kind='gaussian', not to kind={kind!r}")
    return None


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError(f"slice profile kind must be one of {KINDS}, got {kind!r}")
    return kind


def profile_matrix(d_in: int, d_out: int, kind: str = "box", fwhm: Optional[float] = None) -> np.ndarray:
    """W (d_in, d_out) float64 of one of the built-in kinds, rows normalised to 1."""
    r = d_out / d_in
    j = np.arange(d_out, dtype=np.float64)
    W = np.zeros((d_in, d_out), dtype=np.float64)
    for k in range(d_in):
        c = (k + 0.5) * r - 0.5
        if kind == "box":       # overlap length of cell [j - 0.5, j + 0.5) with the slab
            row = np.minimum(j + 0.5, (k + 1) * r - 0.5) - np.maximum(j - 0.5, k * r - 0.5)
            row[row < 1e-12] = 0.0
        elif kind == "gaussian":
            sigma = fwhm * r / FWHM_TO_SIGMA
            row = np.exp(-0.5 * ((j - c) / sigma) ** 2)
            row[row < 1e-4 * row.max()] = 0.0
        else:                   # 'pick': the thin slice nearest the centre
            row = np.zeros(d_out, dtype=np.float64)
            row[min(max(int(math.floor(c + 0.5)), 0), d_out - 1)] = 1.0
        W[k] = row / row.sum()
    return W


def band_table(M: np.ndarray) -> np.ndarray:
    """(rows, 2) int32: the first and the last non-zero column of each row of M; (0, -1), an empty range, for an all-zero
    row (a thin slice that a 'pick' profile never reads has such a row in P)."""
    out = np.zeros((M.shape[0], 2), dtype=np.int32)
    for i, row in enumerate(M):
        nz = np.flatnonzero(row)
        out[i] = (nz[0], nz[-1]) if nz.size else (0, -1)
    return out


class SliceProfile:
    """The measurement model of one (d_in, d_out) pair and everything derived from it: W, P = W^T (W W^T)^-1 (float64), their
    band tables (int32) and fp32 copies (each rounded once from float64); device copies are cached per device."""

    def __init__(self, d_in, d_out, kind="box", fwhm=None, matrix=None):
        for name, v in (("d_in", d_in), ("d_out", d_out)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        d_in, d_out = int(d_in), int(d_out)
        if d_in == d_out:
            raise ValueError(f"d_in == d_out == {d_in}: the depth does not change, there is nothing to project")
        if d_in > d_out:
            raise ValueError(f"d_in={d_in} > d_out={d_out}: a slice profile maps thin slices onto fewer thick ones")
        if d_in > MAX_D_IN or d_out > MAX_D_OUT:
            raise CtsiError(f"slice profile depths d_in={d_in}, d_out={d_out} exceed the limits d_in <= {MAX_D_IN}, "
                            f"d_out <= {MAX_D_OUT} of the depth-consistency kernels")
        if matrix is not None:
            W = np.array(matrix.detach().cpu().numpy() if torch.is_tensor(matrix) else matrix, dtype=np.float64)
            if W.shape != (d_in, d_out):
                raise ValueError(f"matrix has shape {W.shape}, expected (d_in, d_out) = ({d_in}, {d_out})")
            if not np.isfinite(W).all() or (W < 0).any():
                raise ValueError("matrix must hold finite, non-negative weights")
            if (W.sum(axis=1) <= 0).any():
                raise ValueError(f"matrix row(s) {np.flatnonzero(W.sum(axis=1) <= 0).tolist()} are all zero")
            W = W / W.sum(axis=1, keepdims=True)
            kind, fwhm = "matrix", None
        else:
            fwhm = _check_fwhm(_check_kind(kind), fwhm)
            W = profile_matrix(d_in, d_out, kind, fwhm)
        G = W @ W.T
        try:
            cond = float(np.linalg.cond(G))
            P = np.linalg.solve(G, W).T if math.isfinite(cond) and cond <= MAX_COND else None
        except np.linalg.LinAlgError:
            cond, P = float("inf"), None
        if P is None:
            raise ValueError(f"the slice profile cannot be inverted: W W^T is singular or ill-conditioned (cond = {cond:.3g}, "
                             f"limit {MAX_COND:.0e}); its rows overlap too much to be told apart")
        self.d_in, self.d_out, self.kind, self.fwhm, self.cond = d_in, d_out, kind, fwhm, cond
        self.W, self.P = W, np.ascontiguousarray(P)
        self.band_w, self.band_p = band_table(self.W), band_table(self.P)
        self.W32, self.P32 = self.W.astype(np.float32), self.P.astype(np.float32)
        self._device: Dict[torch.device, Tuple[torch.Tensor, ...]] = {}

    def device_tables(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(W32, P32, band_w, band_p) on `device`, uploaded once."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(a).to(device).contiguous()
                                         for a in (self.W32, self.P32, self.band_w, self.band_p))
        return self._device[device]

    def _check_volume(self, x: torch.Tensor, depth: int, what: str):
        if not torch.is_tensor(x) or x.dim() != 5 or x.shape[2] != depth:
            raise ValueError(f"{what}: expected a (N, C, {depth}, H, W) tensor, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")

    def measure(self, x: torch.Tensor) -> torch.Tensor:
        """W x along depth: (N, C, d_out, H, W) -> (N, C, d_in, H, W), differentiable (twice).  ROCm tensors run
        ctsi_depth_measure / ctsi_depth_measure_adj in fp32; CPU tensors take an einsum in their own dtype."""
        self._check_volume(x, self.d_out, "measure")
        if not x.is_cuda:
            return torch.einsum("kj,ncjhw->nckhw", torch.from_numpy(self.W).to(x.dtype), x)
        return _Measure.apply(x.float(), self)


def _launch_measure(profile: SliceProfile, t: torch.Tensor, adjoint: bool) -> torch.Tensor:
    from .engine import Ctx, _ptr
    t = t.contiguous()
    n, c, d, h, w = t.shape
    ctx = Ctx.get(t.device)
    W32, _, band_w, _ = profile.device_tables(t.device)
    with ctx.scope():
        out = torch.empty((n, c, profile.d_out if adjoint else profile.d_in, h, w), dtype=torch.float32, device=t.device)
        if adjoint:
            ctx.lib.depth_measure_adj(_ptr(t), _ptr(W32), _ptr(band_w), _ptr(out), 1.0, 0, n * c, profile.d_in,
                                      profile.d_out, h * w, ctx.sptr)
        else:
            ctx.lib.depth_measure(_ptr(t), _ptr(W32), _ptr(band_w), _ptr(out), n * c, profile.d_in, profile.d_out, h * w,
                                  ctx.sptr)
    t.record_stream(ctx.stream)
    return out


class _Measure(torch.autograd.Function):
    """y = W x; the operator is linear, so its backward is the adjoint of the incoming gradient and nothing is saved."""

    @staticmethod
    def forward(ctx, x, profile):
        ctx.profile = profile
        return _launch_measure(profile, x.detach(), adjoint=False)

    @staticmethod
    def backward(ctx, g):
        return _MeasureAdj.apply(g.float(), ctx.profile), None


class _MeasureAdj(torch.autograd.Function):
    """g_x = W^T g_y, whose own backward is the forward operator (double backward of `measure`)."""

    @staticmethod
    def forward(ctx, g, profile):
        ctx.profile = profile
        return _launch_measure(profile, g.detach(), adjoint=True)

    @staticmethod
    def backward(ctx, gg):
        return _Measure.apply(gg.float(), ctx.profile), None


class DataConsistency:
    """Projection of a generated thin volume onto the thick input: `iterations` times x <- x + P (y - W x), with
    x <- clamp(x, lo, hi) between iterations when `clamp=(lo, hi)` is given.  `final='project'` ends on a projection (the
    result is exactly consistent and may leave [lo, hi]); `final='clamp'` ends on a clamp (in range, approximately
    consistent).  The profile (`kind`, `fwhm` or the caller's `matrix`) is built for the (d_in, d_out) of each call and
    cached.  `last_stats`: per plane (n c) of the last call, float64 on the CPU -- sum r^2 before, sum r^2 after, max |r|
    before, max |r| after, clamp applications -- with r = y - W x; it is copied from the device when read, not by the call."""

    def __init__(self, kind="box", fwhm=None, matrix=None, iterations=1, clamp=None, final="project"):
        if matrix is None:
            fwhm = _check_fwhm(_check_kind(kind), fwhm)
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise ValueError(f"iterations must be an integer >= 1, got {iterations!r}")
        if clamp is not None:
            ok = isinstance(clamp, (tuple, list)) and len(clamp) == 2 and all(
                not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v) for v in clamp)
            if not ok or clamp[0] > clamp[1]:
                raise ValueError(f"clamp must be None or (lo, hi) with finite lo <= hi, got {clamp!r}")
            clamp = (float(clamp[0]), float(clamp[1]))
        if final not in ("project", "clamp"):
            raise ValueError(f"final must be 'project' or 'clamp', got {final!r}")
        if final == "clamp" and clamp is None:
            raise ValueError("final='clamp' needs clamp=(lo, hi)")
        self.kind, self.fwhm, self.matrix = kind, fwhm, matrix
        self.iterations, self.clamp, self.final = iterations, clamp, final
        self.clamp_mode = 0 if clamp is None else (2 if final == "clamp" else 1)
        self._profiles: Dict[Tuple[int, int], SliceProfile] = {}
        self._stats_dev: Optional[torch.Tensor] = None

    def profile(self, d_in: int, d_out: int) -> SliceProfile:
        key = (int(d_in), int(d_out))
        if key not in self._profiles:
            self._profiles[key] = SliceProfile(key[0], key[1], self.kind, self.fwhm, self.matrix)
        return self._profiles[key]

    @property
    def last_stats(self) -> Optional[torch.Tensor]:
        return None if self._stats_dev is None else self._stats_dev.cpu()

    def project_(self, volume: torch.Tensor, thick: torch.Tensor) -> torch.Tensor:
        """In place on `volume`, a contiguous fp32 (N, C, d_out, H, W) ROCm tensor; `thick` is (N, C, d_in, H, W)."""
        from .engine import Ctx, _ptr
        if not (torch.is_tensor(volume) and torch.is_tensor(thick) and volume.dim() == 5 and thick.dim() == 5):
            raise ValueError("project_: expected two (N, C, D, H, W) tensors")
        if not volume.is_cuda:
            raise CtsiError("the projection runs on the HIP engine: pass ROCm tensors (there is no CPU path)")
        if volume.dtype != torch.float32 or not volume.is_contiguous():
            raise CtsiError(f"project_ works in place on a contiguous fp32 tensor, got {volume.dtype}, "
                            f"contiguous={volume.is_contiguous()}; use project() for a copy")
        n, c, d_out, h, w = volume.shape
        if tuple(thick.shape[:2]) != (n, c) or tuple(thick.shape[3:]) != (h, w):
            raise ValueError(f"volume {tuple(volume.shape)} and thick {tuple(thick.shape)} differ outside depth")
        prof = self.profile(int(thick.shape[2]), d_out)
        y = thick.detach().to(device=volume.device, dtype=torch.float32).contiguous()
        ctx = Ctx.get(volume.device)
        lib = ctx.lib
        W32, P32, band_w, band_p = prof.device_tables(volume.device)
        lo, hi = self.clamp if self.clamp is not None else (0.0, 0.0)
        planes, hw = n * c, h * w
        with ctx.scope():
            partials = torch.empty(lib.depth_project_blocks(planes, hw) * 5, dtype=torch.float64, device=volume.device)
            stats = torch.empty((planes, 5), dtype=torch.float64, device=volume.device)
            lib.depth_project(_ptr(volume), _ptr(y), _ptr(W32), _ptr(P32), _ptr(band_w), _ptr(band_p), self.iterations,
                              lo, hi, self.clamp_mode, _ptr(partials), planes, prof.d_in, d_out, hw, ctx.sptr)
            lib.depth_project_finalize(_ptr(partials), _ptr(stats), planes, hw, prof.d_in, ctx.sptr)
        for t in (volume, y):
            t.record_stream(ctx.stream)
        self._stats_dev = stats
        return volume

    def project(self, volume: torch.Tensor, thick: torch.Tensor) -> torch.Tensor:
        """The projected volume as a new fp32 tensor."""
        if not torch.is_tensor(volume):
            raise ValueError("project: expected a tensor")
        return self.project_(volume.detach().to(torch.float32).contiguous().clone(), thick)


def check_data_consistency(value):
    """What `model.data_consistency` / `sampler.data_consistency` accept: a DataConsistency or None (ValueError otherwise)."""
    if value is not None and not isinstance(value, DataConsistency):
        raise ValueError(f"data_consistency must be None or a DataConsistency, got {type(value).__name__}")
    return value


def data_consistency_from_config(config) -> Optional[DataConsistency]:
    """The additive top-level section `data_consistency: {enabled: true, kind, fwhm, iterations, clamp: [lo, hi], final}`; read
    only when `enabled` is a real `true`.  Bad values raise ValueError."""
    sec = config.get("data_consistency", None)
    if not isinstance(sec, dict) or sec.get("enabled", False) is not True:
        return None
    unknown = set(sec) - {"enabled", "kind", "fwhm", "iterations", "clamp", "final"}
    if unknown:
        raise ValueError(f"data_consistency: unknown key(s) {sorted(unknown)}")
    clamp = sec.get("clamp", None)
    return DataConsistency(kind=sec.get("kind", "box"), fwhm=sec.get("fwhm", None), iterations=sec.get("iterations", 1),
                           clamp=tuple(clamp) if isinstance(clamp, list) else clamp, final=sec.get("final", "project"))


def refuse_depth_sharding(*modules, feature=None):
    """Data consistency refuses depth-sharded generation: a column spans ranks.  `feature` names another caller that needs
    whole volumes on one rank (generate_ensemble) in the message."""
    if any(getattr(m, "depth_shard_comm", None) is not None for m in modules if m is not None):
        if feature is not None:
            raise CtsiError(f"{feature} does not support depth sharding (depth_shard_comm): each rank holds a depth slab, "
                            f"not a volume; drop the communicator")
        raise CtsiError("data_consistency does not support depth sharding (depth_shard_comm): a depth column spans ranks and "
                        "the projection needs whole columns; drop the communicator or set data_consistency = None")
