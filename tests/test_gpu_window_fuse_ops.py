"""GPU: the two kernels of latent window fusion (csrc/window_fuse.hip) through the C ABI.

ctsi_window_gather / _f32 are pure copies: torch.equal with torch slicing.  ctsi_window_blend is compared with a float64
restatement built from the host tables; per element the error must stay within (K + 8) 2^-24 max_k |out_k|, K the number of
windows over the voxel: five roundings in the weight product (three table entries rounded to fp32, two multiplications), K in
the accumulation (one fma per window), three of slack for the kernel's operation order."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
WF = importlib.import_module("video-to-video-diffusion_amd.window_fuse")
U24 = 2.0 ** -24

# (full, window, per-axis starts): the feature's test geometry (irregular last start along H, three-fold overlap along W, 18
# windows, up to 12 over one voxel); one window that is the whole volume; a volume past 2048 blocks (the grid-stride loop)
GEO = dict(
    test=((18, 8, 6), (12, 4, 4), ([0, 6], [0, 3, 4], [0, 1, 2])),
    single=((5, 6, 7), (5, 6, 7), ([0], [0], [0])),
    stride=((64, 48, 48), (32, 32, 32), ([0, 32], [0, 16], [0, 16])),
)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _starts(axes):
    return [(d, h, w) for d in axes[0] for h in axes[1] for w in axes[2]]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


@pytest.fixture(scope="module")
def ctx():
    return E.Ctx.get(torch.device(DEV))


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
def _gather(ctx, src, dst, starts, batch, halves, full, win, L, f32):
    st = torch.tensor(starts, dtype=torch.int32, device=DEV)
    fn = ctx.lib.window_gather_f32 if f32 else ctx.lib.window_gather
    with ctx.scope():
        fn(_ptr(src), _ptr(dst), _ptr(st), batch, halves, len(starts), *full, *win, L, src.shape[-1], dst.shape[-1], ctx.sptr)
    torch.cuda.synchronize()


@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("dtype,L,src_ct,dst_ct", [(torch.bfloat16, 8, 8, 16), (torch.bfloat16, 8, 16, 16),
                                                   (torch.float32, 8, 8, 8), (torch.float32, 4, 4, 8),
                                                   (torch.bfloat16, 4, 4, 8), (torch.bfloat16, 6, 6, 12),
                                                   (torch.bfloat16, 3, 3, 6), (torch.float32, 3, 3, 3)],
                         ids=["bf16-16B", "bf16-16B-pitched", "f32-16B", "f32-16B-pitched", "bf16-8B", "bf16-4B", "bf16-2B",
                              "f32-4B"])
@pytest.mark.parametrize("geo", ["test", "stride"])
def test_gather_is_torch_slicing(ctx, geo, dtype, L, src_ct, dst_ct, halves):
    full, win, axes = GEO[geo]
    starts, B = _starts(axes), 2
    nw = len(starts)
    src = _randn((B, *full, src_ct), 1).to(dtype).to(DEV)
    dst0 = _randn((halves * nw * B, *win, dst_ct), 2).to(dtype).to(DEV)
    dst = dst0.clone()
    _gather(ctx, src, dst, starts, B, halves, full, win, L, dtype == torch.float32)
    want = dst0.clone()
    for g in range(halves):
        for k, (sd, sh, sw) in enumerate(starts):
            for b in range(B):
                want[(g * nw + k) * B + b, ..., :L] = src[b, sd:sd + win[0], sh:sh + win[1], sw:sw + win[2], :L]
    assert torch.equal(dst.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))       # the other channels included


# ---------------------------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------------------------
def _tables(full, win, axes):
    return [WF.axis_table(f, s, st) for f, s, st in zip(full, win, axes)]


def _window_weights(t, nwin, size):
    """(nwin, size) float64: the table's weight of window k at its position o."""
    out = np.zeros((nwin, size))
    for p in range(t.count.shape[0]):
        for j in range(int(t.count[p])):
            out[t.index[p, j], t.offset[p, j]] = t.weight[p, j]
    return torch.from_numpy(out)


def _blend(ctx, win_t, out, tables, batch, halves, full, win, axes):
    ti, tw = WF.pack_tables(tables)
    ti, tw = ti.to(DEV), tw.to(DEV)
    kk = [t.index.shape[1] for t in tables]
    with ctx.scope():
        ctx.lib.window_blend(_ptr(win_t), _ptr(out), _ptr(ti), _ptr(tw), batch, halves, *[len(a) for a in axes], *full, *win,
                             win_t.shape[-1], *kk, ctx.sptr)
    torch.cuda.synchronize()
    return out


def _restate(win_t, tables, batch, halves, full, win, axes):
    """float64: (sum_k wd wh ww out_k, K = windows over the voxel, max_k |out_k|), all of the full shape."""
    starts, nw = _starts(axes), len(_starts(axes))
    wts = [_window_weights(t, len(a), s) for t, a, s in zip(tables, axes, win)]
    Cc = win_t.shape[-1]
    ref = torch.zeros(halves * batch, *full, Cc, dtype=torch.float64)
    amax = torch.zeros_like(ref)
    K = torch.zeros(*full, dtype=torch.float64)
    x = win_t.double().cpu()
    for k, (sd, sh, sw) in enumerate(starts):
        kd, kh, kw = k // (len(axes[1]) * len(axes[2])), (k // len(axes[2])) % len(axes[1]), k % len(axes[2])
        wgt = (wts[0][kd][:, None, None] * wts[1][kh][None, :, None] * wts[2][kw][None, None, :])[..., None]
        sl = (slice(sd, sd + win[0]), slice(sh, sh + win[1]), slice(sw, sw + win[2]))
        K[sl] += 1
        for g in range(halves):
            for b in range(batch):
                o = x[(g * nw + k) * batch + b]
                ref[(g * batch + b, *sl)] += wgt * o
                amax[(g * batch + b, *sl)] = torch.maximum(amax[(g * batch + b, *sl)], o.abs())
    return ref, K, amax


def _check(tag, got, ref, K, amax):
    err = (got.double().cpu() - ref).abs()
    bound = (K[None, ..., None] + 8) * U24 * amax
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{tag}: max |err| / ((K + 8) 2^-24 max|out|) = {ratio:.3f}, K max {int(K.max())}")
    assert bool((err <= bound).all()), ratio


@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("Cc", [8, 16])
@pytest.mark.parametrize("geo", ["test", "stride"])
def test_blend_against_float64(ctx, geo, Cc, halves):
    full, win, axes = GEO[geo]
    B = 2 if geo == "test" else 1
    nw = len(_starts(axes))
    tables = _tables(full, win, axes)
    win_t = (_randn((halves * nw * B, *win, Cc), 3) * 3.0).to(DEV)
    out = torch.full((halves * B, *full, Cc), float("nan"), device=DEV)          # poisoned: every element must be written
    _blend(ctx, win_t, out, tables, B, halves, full, win, axes)
    assert bool(torch.isfinite(out).all())
    ref, K, amax = _restate(win_t, tables, B, halves, full, win, axes)
    if geo == "test":
        assert int(K.max()) == 12
    _check(f"blend[{geo}, C={Cc}, halves={halves}]", out, ref, K, amax)
    again = _blend(ctx, win_t, torch.full_like(out, float("nan")), tables, B, halves, full, win, axes)
    assert torch.equal(out, again)                                                # run to run: bit identical


@pytest.mark.parametrize("Cc", [8, 16])
def test_blend_is_a_partition_of_unity(ctx, Cc):
    """Every window holds the restriction of one global field: the blend returns the field."""
    full, win, axes = GEO["test"]
    starts, B = _starts(axes), 2
    nw = len(starts)
    tables = _tables(full, win, axes)
    field = (_randn((B, *full, Cc), 4) * 2.0 + 0.5)
    win_t = torch.empty(nw * B, *win, Cc)
    for k, (sd, sh, sw) in enumerate(starts):
        win_t[k * B:(k + 1) * B] = field[:, sd:sd + win[0], sh:sh + win[1], sw:sw + win[2]]
    out = _blend(ctx, win_t.to(DEV), torch.full((B, *full, Cc), float("nan"), device=DEV), tables, B, 1, full, win, axes)
    _, K, _ = _restate(win_t, tables, B, 1, full, win, axes)
    _check(f"partition of unity[C={Cc}]", out, field.double(), K, field.double().abs())


@pytest.mark.parametrize("Cc", [8, 16])
def test_a_single_window_is_returned_bit_for_bit(ctx, Cc):
    full, win, axes = GEO["single"]
    tables = _tables(full, win, axes)
    assert all((t.weight == 1.0).all() for t in tables)
    win_t = _randn((2 * 2, *win, Cc), 5).to(DEV)            # two samples, both guidance halves
    out = _blend(ctx, win_t, torch.full((4, *full, Cc), float("nan"), device=DEV), tables, 2, 2, full, win, axes)
    assert torch.equal(out, win_t)
