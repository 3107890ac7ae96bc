"""Latent-space window fusion (MultiDiffusion, Bar-Tal et al. 2023): the overlapping windows of a stitched
volume share ONE latent.  Per U-Net evaluation the network runs on all windows as one batch, its outputs are blended into one
full-size prediction with Gaussian weights normalised to a partition of unity, the sampler update runs on the full latent,
and the new network input is cut back into the windows -- all inside the captured step (csrc/window_fuse.hip).

This module holds the host side: the per-axis weight tables, the latent geometry of a stitched volume, and the step program
whose network shape (windows) differs from its state shape (full latent).  sampler.run_sampler_fused drives it.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from .engine import Act, Ctx, _ptr
from .engine_x3 import unet_program
from .lib import CtsiError

FUSIONS = ("pixel", "latent")
DECODES = ("full", "windows")


def check_fusion(fusion, decode) -> Tuple[str, str]:
    """Validate sample_with_stitching's `fusion` / `decode` (ValueError otherwise).  `decode` belongs to fusion='latent' (None:
    its default, 'full'); returns (fusion, decode) with decode None under 'pixel'."""
    if not isinstance(fusion, str) or fusion not in FUSIONS:
        raise ValueError(f"unknown fusion {fusion!r}: expected one of {FUSIONS}")
    if decode is not None and (not isinstance(decode, str) or decode not in DECODES):
        raise ValueError(f"unknown decode {decode!r}: expected one of {DECODES}")
    if fusion == "pixel":
        if decode is not None:
            raise ValueError("decode= belongs to fusion='latent': fusion='pixel' decodes every window's own sample")
        return fusion, None
    return fusion, decode or "full"


class AxisTable(NamedTuple):
    """The windows over every position of one axis (axis_table): K = the largest cover count."""
    count: np.ndarray       # (P,) int32 windows covering position p
    index: np.ndarray       # (P, K) int32 their indices into `starts`, ascending
    offset: np.ndarray      # (P, K) int32 p - start
    weight: np.ndarray      # (P, K) float64 w(p - s_k) / sum_j w(p - s_j); entries past `count` are 0


def axis_table(full: int, size: int, starts: Sequence[int]) -> AxisTable:
    """The blend table of one axis: windows of `size` at `starts` over [0, full), weighted by the stitching window
    (sampler._axis_window(size), the fp32 values) normalised in float64 to sum to 1 at every position."""
    from .sampler import _axis_window
    starts = [int(s) for s in starts]
    if not starts or any(s < 0 or s + size > full for s in starts) or sorted(set(starts)) != starts:
        raise CtsiError(f"window starts {starts} of size {size} do not lie, ascending, inside an axis of {full}")
    w = _axis_window(size).double().numpy()
    cover = [[k for k, s in enumerate(starts) if s <= p < s + size] for p in range(full)]
    if not all(cover):
        raise CtsiError(f"windows of size {size} at {starts} leave positions of an axis of {full} uncovered")
    K = max(len(c) for c in cover)
    count = np.array([len(c) for c in cover], dtype=np.int32)
    index = np.zeros((full, K), dtype=np.int32)
    offset = np.zeros((full, K), dtype=np.int32)
    weight = np.zeros((full, K), dtype=np.float64)
    for p, c in enumerate(cover):
        raw = np.array([w[p - starts[k]] for k in c], dtype=np.float64)
        index[p, :len(c)] = c
        offset[p, :len(c)] = [p - starts[k] for k in c]
        weight[p, :len(c)] = raw / raw.sum()
    return AxisTable(count, index, offset, weight)


def pack_tables(tables: Sequence[AxisTable]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tables of the three axes as ctsi_window_blend reads them: (int32 [per axis: counts, indices, offsets], fp32 [per
    axis: weights, the float64 values rounded once])."""
    ti = np.concatenate([np.concatenate([t.count.ravel(), t.index.ravel(), t.offset.ravel()]) for t in tables])
    tw = np.concatenate([t.weight.ravel() for t in tables])
    return torch.from_numpy(ti.astype(np.int32)), torch.from_numpy(tw).to(torch.float32)


class FuseGeometry(NamedTuple):
    """The latent geometry of one stitched volume (stitch_geometry)."""
    pixel_windows: List[Tuple[int, int, int]]      # (ds, hs, ws) of every window in the thick volume, product order
    full: Tuple[int, int, int]                      # latent (D, H, W) of the whole target volume
    win: Tuple[int, int, int]                       # latent (td, lh, lw) of one window
    starts: List[Tuple[int, int, int]]              # latent start of every window, same order
    factor: int                                     # in-plane pixels per latent voxel


def stitch_geometry(vae, volume_shape, patch_size, target_patch_size, stride) -> FuseGeometry:
    """Windows of sample_with_stitching (sampler._window_starts per axis, product order ds, hs, ws) in latent coordinates:
    depth factor 1, in-plane factor f from vae.get_latent_shape.  Every in-plane size and start must be a multiple of f."""
    from .sampler import _window_starts
    b, c, d_thick, hf, wf = [int(v) for v in volume_shape]
    pd, ph, pw = [int(v) for v in patch_size]
    td = int(target_patch_size[0])
    ratio = td / pd
    d_thin = int(d_thick * ratio)
    lat = vae.get_latent_shape((b, c, td, ph, pw))
    f = ph // lat[3] if lat[3] else 0
    hs_all, ws_all = _window_starts(hf, ph, stride[1]), _window_starts(wf, pw, stride[2])
    bad = [v for v in (hf, wf, ph, pw, *hs_all, *ws_all) if f <= 0 or v % f]
    if bad or pw // f != lat[4]:
        raise CtsiError(f"fusion='latent' needs the volume (h, w)=({hf},{wf}), the patch (h, w)=({ph},{pw}) and every window "
                        f"start (h: {hs_all}, w: {ws_all}) to be multiples of the VAE's in-plane factor {f or 4}: {bad} are not; "
                        "choose such a stride and sizes, or use fusion='pixel'")
    ds_all = _window_starts(d_thick, pd, stride[0])
    pix = [(ds, hs, ws) for ds in ds_all for hs in hs_all for ws in ws_all]
    return FuseGeometry(pix, (d_thin, hf // f, wf // f), (td, ph // f, pw // f),
                        [(int(ds * ratio), hs // f, ws // f) for ds, hs, ws in pix], f)


def axis_starts(starts: Sequence[Sequence[int]]) -> Tuple[List[int], List[int], List[int]]:
    """The per-axis start lists of a product-ordered window list (CtsiError when it is not one)."""
    axes = tuple(sorted({int(s[a]) for s in starts}) for a in range(3))
    if [tuple(int(v) for v in s) for s in starts] != [(d, h, w) for d in axes[0] for h in axes[1] for w in axes[2]]:
        raise CtsiError("latent window fusion needs the windows as a product grid in (d, h, w) order: the blend weights are "
                        "normalised per axis")
    return axes


class _WindowFused:
    """Mixed in before a U-Net step program class (fused_program): the network runs on `nw` windows per sample -- row
    (g nw + k) n + b for window k of sample b in guidance half g -- while z, eps, hist, noise, the nonfinite table and
    z_ncdhw() / eps_ncdhw() have the full latent's shape.  The head's fp32 output goes to `win_out`; ctsi_window_blend writes
    `eps` from it ahead of everything add_sampler_step puts behind the network, and ctsi_window_gather cuts `zin_full`, the
    network input the update writes, back into the z half of the window rows (both guidance halves: it stands where
    ctsi_cfg_mirror stands in the plain program).  Timestep rows: one per (evaluation, network row), all equal."""

    def __init__(self, ctx: Ctx, unet, n: int, full, win, starts, max_rows: int, attention_mode="fast", guided: bool = False,
                 rescale: bool = False, prediction: str = "epsilon"):
        if getattr(unet, "learn_sigma", False):
            raise CtsiError("latent window fusion does not support a learn_sigma model: the variance channels of overlapping "
                            "windows have no blend; use fusion='pixel'")
        D, H, W = [int(v) for v in full]
        td, lh, lw = [int(v) for v in win]
        axes = axis_starts(starts)
        self.tables = [axis_table(F, S, st) for F, S, st in zip((D, H, W), (td, lh, lw), axes)]
        self.nwin = tuple(len(a) for a in axes)
        self.nw = nw = len(starts)
        super().__init__(ctx, unet, nw * n, td, lh, lw, max_rows, attention_mode, guided=guided, rescale=rescale,
                         prediction=prediction)
        # the base class left a window-shaped state behind: keep its head output as `win_out`, make the state full-shape
        self.net_n, self.net_nb, self.win = self.n, self.nb, (td, lh, lw)
        self.win_out, window_z = self.eps, self.z
        self.keep = [t for t in self.keep if t is not window_z]
        self.n, self.nb, self.d, self.h, self.w = n, (2 * n if guided else n), D, H, W
        L = self.L
        self.eps = self.persistent((self.nb, D, H, W, L), torch.float32)
        self.z = self.persistent((n, D, H, W, L), torch.float32, zero=True)
        f32 = super()._sampler_zin()[3]
        self.zin_full = self.persistent((n, D, H, W, L), torch.float32 if f32 else torch.bfloat16)
        ti, tw = pack_tables(self.tables)
        self.tab_i = self.persistent(tuple(ti.shape), torch.int32)
        self.tab_w = self.persistent(tuple(tw.shape), torch.float32)
        self.starts = self.persistent((nw, 3), torch.int32)
        self.tab_i.copy_(ti)
        self.tab_w.copy_(tw)
        self.starts.copy_(torch.tensor([[int(v) for v in s] for s in starts], dtype=torch.int32))

    def _sampler_zin(self):
        """The update writes the full-shape network input (L channels per voxel); the gather cuts it into the windows."""
        _, _, es, f32 = super()._sampler_zin()
        return _ptr(self.zin_full), self.L, es, f32

    def _gather_call(self):
        lib, sptr = self.lib, self.ctx.sptr
        dst, dst_ct, _, f32 = super()._sampler_zin()
        fn = lib.window_gather_f32 if f32 else lib.window_gather
        src, st = _ptr(self.zin_full), _ptr(self.starts)
        n, halves, nw, L = self.n, self.nb // self.n, self.nw, self.L
        (D, H, W), (td, lh, lw) = (self.d, self.h, self.w), self.win
        return lambda: fn(src, dst, st, n, halves, nw, D, H, W, td, lh, lw, L, L, dst_ct, sptr)

    def _add_window_gather(self):
        _, _, es, _ = super()._sampler_zin()
        td, lh, lw = self.win
        self._emit(self._gather_call(), "window.gather", nbytes=2.0 * self.net_nb * td * lh * lw * self.L * es,
                   audit=dict(kind="window_gather", src=self.zin_full, zin=self.xin, starts=self.starts, n=self.n,
                              halves=self.nb // self.n, nw=self.nw, L=self.L, full=(self.d, self.h, self.w), win=self.win))

    def _add_window_blend(self):
        lib, sptr = self.lib, self.ctx.sptr
        wp, ep, ip, fp = _ptr(self.win_out), _ptr(self.eps), _ptr(self.tab_i), _ptr(self.tab_w)
        n, halves, L = self.n, self.nb // self.n, self.L
        (D, H, W), (td, lh, lw), (nd, nh, nx) = (self.d, self.h, self.w), self.win, self.nwin
        kd, kh, kw = (t.index.shape[1] for t in self.tables)
        self._emit(lambda: lib.window_blend(wp, ep, ip, fp, n, halves, nd, nh, nx, D, H, W, td, lh, lw, L, kd, kh, kw, sptr),
                   "window.blend", nbytes=4.0 * L * (self.net_nb * td * lh * lw + self.nb * D * H * W),
                   audit=dict(kind="window_blend", win=self.win_out, out=self.eps, tables=self.tables, tab_i=self.tab_i,
                              tab_w=self.tab_w, n=n, halves=halves, nwin=self.nwin, L=L, full=(D, H, W), win_dims=self.win))

    def _zin_act(self) -> Act:
        return Act(self.zin_full, self.n, self.L, self.d, self.h, self.w)

    def _add_input_fanout(self):
        self._add_window_gather()          # both guidance halves read the one full-shape input: no mirror

    def add_sampler_step(self, kind: str, with_noise: bool, update_form: str = "eps", learned_variance: bool = False):
        """engine.UNetProgram.add_sampler_step on the full shape, with the blend ahead of it; the gather is its
        _add_input_fanout, between the update and the step-counter increment."""
        if learned_variance:
            raise CtsiError("internal: latent window fusion has no learned-variance step")
        self._add_window_blend()
        super().add_sampler_step(kind, with_noise, update_form)

    def load_latents(self, z_ncdhw, cond_ncdhw):
        """`z_ncdhw`: the full latent (n, L, D, H, W); `cond_ncdhw`: the windows' conditioning latents (nw n, L, td, lh, lw),
        window-major, loaded once into the conditional rows (the null rows of a guided program stay zero)."""
        lib, sptr = self.lib, self.ctx.sptr
        n, L, D, H, W = self.n, self.L, self.d, self.h, self.w
        td, lh, lw = self.win
        _, _, _, f32 = super()._sampler_zin()
        if z_ncdhw is not None:
            if tuple(z_ncdhw.shape) != (n, L, D, H, W):
                raise CtsiError(f"the fused program holds a full latent of shape {(n, L, D, H, W)}, got {tuple(z_ncdhw.shape)}")
            z = z_ncdhw.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
            lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), _ptr(self.z), n, L, D, H, W, sptr)
            if f32:
                lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), _ptr(self.zin_full), n, L, D, H, W, sptr)
            else:
                lib.ncdhw_f32_to_ndhwc_bf16(_ptr(z), _ptr(self.zin_full), n, L, D, H, W, L, 0, sptr)
            self._gather_call()()
            z.record_stream(self.ctx.stream)
        if cond_ncdhw is not None:
            if tuple(cond_ncdhw.shape) != (self.net_n, L, td, lh, lw):
                raise CtsiError(f"the fused program takes the windows' conditioning as {(self.net_n, L, td, lh, lw)}, got "
                                f"{tuple(cond_ncdhw.shape)}")
            cnd = cond_ncdhw.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
            if f32:
                lib.ncdhw_f32_to_ndhwc_f32(_ptr(cnd), _ptr(self.xin2.t), self.net_n, L, td, lh, lw, sptr)
            else:
                lib.ncdhw_f32_to_ndhwc_bf16(_ptr(cnd), self.xin.ip, self.net_n, L, td, lh, lw, 2 * L, L, sptr)
            cnd.record_stream(self.ctx.stream)


_FUSED: Dict[str, type] = {}


def fused_program(precision: str) -> type:
    """The window-fused step program class of an inference precision: _WindowFused over engine_x3.unet_program(precision)."""
    if precision not in _FUSED:
        base = unet_program(precision)
        _FUSED[precision] = type("Fused" + base.__name__, (_WindowFused, base), {"__doc__": _WindowFused.__doc__})
    return _FUSED[precision]
