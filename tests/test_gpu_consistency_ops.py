"""GPU: the depth-consistency kernels (csrc/depth_consistency.hip) against float64 restatements.

Inputs: x = tanh of a formula field, y = clamp(W x_other + 0.02 noise, -1, 1).  Shapes, the smallest that reach each path:
(planes 3, 2 -> 12, 5 x 7) ragged, unaligned, scalar; (2, 8 -> 48, 16 x 16) the 16-byte path; (1, 3 -> 8, 4 x 20) fractional box
weights; (1, 50 -> 300, 8 x 24) the 32-wide tile of deep volumes; an x offset by 4 bytes into its storage (scalar path on an
aligned shape); d_in = d_out - 1 and d_in = 1.

Yardstick: a kernel's error against float64 is at most 2 x the error of the same sequence evaluated by torch in fp32 on the
device (the 2 x is for a different summation order, nothing else) plus one fp32 ulp of the largest value.  Exactness (clamp
modes 0 and 1): max |y - W x_out|, in float64 on the fp32 output, by the same rule.  The statistics table equals float64 values
computed from the kernel's own input and output to 1e-12 relative: the kernel sums the exact fp64 products ascending along
depth, and so does the restatement here.  The clamp count is exact, plane by plane, against the float64 restatement (how many
of its values come within 1e-6 of a bound is printed: an fp32 decision could differ only there, and does not at these inputs).
A clamp range that excludes 0 on the ragged shape checks that the zero padding of the last tile stays out of the statistics."""
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import formula_input, formula_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
E = importlib.import_module("video-to-video-diffusion_amd.engine")

BOX, G15 = dict(kind="box"), dict(kind="gaussian", fwhm=1.5)
# id -> (planes, d_in, d_out, h, w, offset x by one float)
SHAPES = {"ragged-2to12": (3, 2, 12, 5, 7, False), "vec-8to48": (2, 8, 48, 16, 16, False), "frac-3to8": (1, 3, 8, 4, 20, False),
          "deep-50to300": (1, 50, 300, 8, 24, False), "offset-8to48": (2, 8, 48, 16, 16, True),
          "dminus1-7to8": (1, 7, 8, 3, 5, False), "one-1to4": (1, 1, 4, 3, 5, False)}
CASES = [(s, n) for s in SHAPES for n in ("box", "gauss1.5") if not (n == "gauss1.5" and s in ("dminus1-7to8", "one-1to4"))]
LO, HI = -0.875, 0.875          # exact in fp32: the kernel and the float64 restatement clamp at the same value


def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


_CACHE = {}


def case(shape_id, prof_name):
    """(profile, x fp32 device, y fp32 device): built once per case and left unchanged."""
    key = (shape_id, prof_name)
    if key not in _CACHE:
        planes, d_in, d_out, h, w, offset = SHAPES[shape_id]
        prof = CS.SliceProfile(d_in, d_out, **(BOX if prof_name == "box" else G15))
        seed = 100 + 7 * sorted(SHAPES).index(shape_id)
        x = torch.tanh(formula_input((planes, 1, d_out, h, w), seed))
        other = torch.tanh(formula_input((planes, 1, d_out, h, w), seed + 1)).double()
        y = (torch.einsum("kj,ncjhw->nckhw", torch.from_numpy(prof.W), other)
             + 0.02 * formula_noise(seed, (planes, 1, d_in, h, w)).double()).clamp(-1, 1).float().contiguous()
        if offset:          # one float into a larger storage: 4-byte aligned only
            buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)
            buf[1:] = x.reshape(-1).to(DEV)
            xd = buf[1:].view(x.shape)
            assert xd.data_ptr() % 16 == 4
        else:
            xd = x.to(DEV)
        _CACHE[key] = (prof, xd, y.to(DEV))
        assert xd.is_contiguous() and _CACHE[key][2].is_contiguous()      # the launchers below pass raw pointers
    return _CACHE[key]


def clone_like(x, src=None):
    """A copy of src (default: of x itself) with the alignment of x: the offset case stays 4 bytes off."""
    src = x if src is None else src
    if x.data_ptr() % 16 == 0:
        out = src.clone()
    else:
        buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=x.device)
        buf[1:] = src.reshape(-1)
        out = buf[1:].view(x.shape)
    assert out.data_ptr() % 16 == x.data_ptr() % 16 and out.is_contiguous()
    return out


def launch_measure(prof, x):
    ctx = E.Ctx.get(x.device)
    n, c, d, h, w = x.shape
    W32, _, bw, _ = prof.device_tables(x.device)
    out = torch.empty((n, c, prof.d_in, h, w), dtype=torch.float32, device=x.device)
    with ctx.scope():
        ctx.lib.depth_measure(E._ptr(x), E._ptr(W32), E._ptr(bw), E._ptr(out), n * c, prof.d_in, prof.d_out, h * w, ctx.sptr)
    return out


def launch_adj(prof, g, gx, scale, accumulate):
    ctx = E.Ctx.get(g.device)
    n, c, d, h, w = g.shape
    W32, _, bw, _ = prof.device_tables(g.device)
    with ctx.scope():
        ctx.lib.depth_measure_adj(E._ptr(g), E._ptr(W32), E._ptr(bw), E._ptr(gx), float(scale), int(accumulate), n * c, prof.d_in,
                                  prof.d_out, h * w, ctx.sptr)
    return gx


def launch_project(prof, x, y, iters, mode, stats=True, lo=None, hi=None):
    """In place on x; returns the (planes, 5) float64 table (None without statistics)."""
    ctx = E.Ctx.get(x.device)
    n, c, d, h, w = x.shape
    W32, P32, bw, bp = prof.device_tables(x.device)
    planes, hw = n * c, h * w
    lo, hi = LO if lo is None else lo, HI if hi is None else hi
    partials = table = None
    if stats:
        partials = torch.empty(ctx.lib.depth_project_blocks(planes, hw) * 5, dtype=torch.float64, device=x.device)
        table = torch.empty((planes, 5), dtype=torch.float64, device=x.device)
    with ctx.scope():
        ctx.lib.depth_project(E._ptr(x), E._ptr(y), E._ptr(W32), E._ptr(P32), E._ptr(bw), E._ptr(bp), iters, lo, hi, mode,
                              E._ptr(partials), planes, prof.d_in, prof.d_out, hw, ctx.sptr)
        if stats:
            ctx.lib.depth_project_finalize(E._ptr(partials), E._ptr(table), planes, hw, prof.d_in, ctx.sptr)
    torch.cuda.synchronize()
    return table


def mv(M, v):
    """M (a, b) applied along depth of v (n, c, b, h, w), in v's dtype and on v's device."""
    return torch.einsum("ab,ncbhw->ncahw", M.to(device=v.device, dtype=v.dtype), v)


def project_sequence(W, P, x, y, iters, mode, lo=None, hi=None):
    """The kernel's sequence restated in the dtype of x: returns (x_out, per plane the number of clamp applications that
    changed a voxel (float64, CPU), number of voxels that came within 1e-6 of a bound at a clamp)."""
    lo, hi = LO if lo is None else lo, HI if hi is None else hi
    clamped, near = torch.zeros(x.shape[0] * x.shape[1], dtype=torch.float64), 0
    for it in range(iters):
        x = x + mv(P, y - mv(W, x))
        if mode != 0 and (it + 1 < iters or mode == 2):
            clamped += ((x < lo) | (x > hi)).sum(dim=(2, 3, 4)).reshape(-1).double().cpu()
            near += int((((x - lo).abs() < 1e-6) | ((x - hi).abs() < 1e-6)).sum())
            x = x.clamp(lo, hi)
    return x, clamped, near


def sequential_residual(W32, x, y):
    """y - W x in float64 with the sum taken ascending along depth, one exact product at a time: the kernel's statistics order."""
    W = torch.from_numpy(W32).double()
    xd, acc = x.double().cpu(), torch.zeros(y.shape, dtype=torch.float64)
    for j in range(W.shape[1]):
        acc = acc + W[:, j].view(1, 1, -1, 1, 1) * xd[:, :, j:j + 1]
    return y.double().cpu() - acc


def check_2x(tag, got, ref64, torch32):
    e_k = float((got.double() - ref64).abs().max())
    e_t = float((torch32.double() - ref64).abs().max())
    bound = 2.0 * e_t + ulp32(float(ref64.abs().max()))
    print(f"  {tag}: kernel {e_k:.3e}  torch-fp32 {e_t:.3e}  bound {bound:.3e}")
    assert e_k <= bound, (tag, e_k, e_t, bound)
    return bound


@pytest.mark.parametrize("shape_id,prof_name", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_measure_and_adjoint(shape_id, prof_name):
    prof, x, y = case(shape_id, prof_name)
    W32 = torch.from_numpy(prof.W32)
    g = y * 0.5 + 0.25              # any field of y's shape serves as the incoming gradient
    print(f"\n[{shape_id} {prof_name}] measure / adjoint")
    m = launch_measure(prof, x)
    torch.cuda.synchronize()
    b_y = check_2x("measure", m, mv(W32.double(), x.double()), mv(W32, x))
    gx = launch_adj(prof, g, clone_like(x, torch.zeros_like(x)), 1.0, 0)     # (the offset case writes a misaligned g_x)
    torch.cuda.synchronize()
    ref_gx = mv(W32.double().t(), g.double())
    b_gx = check_2x("measure_adj", gx, ref_gx, mv(W32.t(), g))
    # adjoint identity on the kernel outputs, in float64.  It is exact for exact outputs; the outputs carry independent
    # rounding errors of at most b_y / b_gx per element (the elementwise bounds above), which add up in an inner product as a
    # root sum of squares: |<e, g>| <~ b ||g||_2.  A band off by one moves whole elements by ~0.1 and misses this by orders.
    a, b = float((m.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
    bound = float(g.double().norm()) * b_y + float(x.double().norm()) * b_gx
    print(f"  <W x, g> = {a:.9f}  <x, W^T g> = {b:.9f}  |difference| {abs(a - b):.3e}  bound {bound:.3e}")
    assert abs(a - b) <= bound
    # scale and accumulate
    base = clone_like(x, x * 0.75 - 0.1)
    acc = launch_adj(prof, g, clone_like(base), 0.5, 1)
    torch.cuda.synchronize()
    check_2x("measure_adj scale 0.5 accumulate", acc, base.double() + 0.5 * ref_gx, base + 0.5 * mv(W32.t(), g))
    sc = launch_adj(prof, g, clone_like(base), -2.0, 0)
    torch.cuda.synchronize()
    check_2x("measure_adj scale -2 overwrite", sc, -2.0 * ref_gx, -2.0 * mv(W32.t(), g))


@pytest.mark.parametrize("shape_id,prof_name", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_project(shape_id, prof_name):
    prof, x, y = case(shape_id, prof_name)
    W32, P32, W64 = torch.from_numpy(prof.W32), torch.from_numpy(prof.P32), torch.from_numpy(prof.W)
    x_before = x.clone()
    for iters in (1, 3):
        for mode in (0, 1, 2):
            tag = f"{shape_id} {prof_name} iters {iters} mode {mode}"
            print(f"\n[{tag}]")
            out = clone_like(x)
            table = launch_project(prof, out, y, iters, mode).cpu()
            ref64, n_clamped, n_near = project_sequence(W32.double(), P32.double(), x.double(), y.double(), iters, mode)
            t32, _, _ = project_sequence(W32, P32, x, y, iters, mode)
            check_2x("project", out, ref64, t32)
            if mode in (0, 1):        # ends on a projection: exactly consistent, judged against the float64 profile
                q_k = float((y.double() - mv(W64, out.double())).abs().max())
                q_t = float((y.double() - mv(W64, t32.double())).abs().max())
                bound = 2.0 * q_t + ulp32(float(out.abs().max()))
                print(f"  exactness max|y - W x_out|: kernel {q_k:.3e}  torch-fp32 {q_t:.3e}  bound {bound:.3e}")
                assert q_k <= bound
            else:
                assert float(out.min()) >= LO and float(out.max()) <= HI
            # the statistics table, from the kernel's own input and output
            r0, r1 = sequential_residual(prof.W32, x, y), sequential_residual(prof.W32, out, y)
            want = torch.stack([r0.pow(2).sum(dim=(2, 3, 4)).reshape(-1), r1.pow(2).sum(dim=(2, 3, 4)).reshape(-1),
                                r0.abs().amax(dim=(2, 3, 4)).reshape(-1), r1.abs().amax(dim=(2, 3, 4)).reshape(-1)], dim=1)
            rel = ((table[:, :4] - want).abs() / want.abs().clamp_min(1e-300)).max()
            n_clamped_planes, n_clamped = n_clamped, int(n_clamped.sum())
            print(f"  stats: rms before {float(want[:, 0].sum() / r0.numel()) ** 0.5:.3e} after "
                  f"{float(want[:, 1].sum() / r1.numel()) ** 0.5:.3e}  max before {float(want[:, 2].max()):.3e} after "
                  f"{float(want[:, 3].max()):.3e}  table rel err {float(rel):.2e}  clamped {int(table[:, 4].sum())} "
                  f"(float64 {n_clamped}, within 1e-6 of a bound {n_near})")
            assert float(rel) <= 1e-12
            assert torch.equal(table[:, 4], n_clamped_planes)         # exact, plane by plane
            if mode == 0:
                assert int(table[:, 4].sum()) == 0
            assert float(want[:, 0].sum()) > float(want[:, 1].sum())
            # a second run: the same bits, statistics included; without statistics the same volume
            again = clone_like(x)
            table2 = launch_project(prof, again, y, iters, mode).cpu()
            assert torch.equal(again, out) and torch.equal(table2.view(torch.int64), table.view(torch.int64))
            plain = clone_like(x)
            launch_project(prof, plain, y, iters, mode, stats=False)
            assert torch.equal(plain, out)
    assert torch.equal(x, x_before)


@pytest.mark.parametrize("iters", [1, 3])
def test_ragged_tile_padding_stays_out_of_the_statistics(iters):
    """Clamp range (0.25, 0.875), ending on the clamp, on the 5 x 7 planes: the last tile's padded positions are staged as 0,
    which this range does not contain.  They must count neither as clamped voxels nor in the residual of the output."""
    prof, x, y = case("ragged-2to12", "box")
    lo, hi = 0.25, 0.875
    out = x.clone()
    table = launch_project(prof, out, y, iters, 2, lo=lo, hi=hi).cpu()
    W32, P32 = torch.from_numpy(prof.W32), torch.from_numpy(prof.P32)
    ref64, counts, near = project_sequence(W32.double(), P32.double(), x.double(), y.double(), iters, 2, lo, hi)
    t32, _, _ = project_sequence(W32, P32, x, y, iters, 2, lo, hi)
    print(f"\n[ragged clamp (0.25, 0.875) iters {iters}]")
    check_2x("project", out, ref64, t32)
    assert float(out.min()) >= lo and float(out.max()) <= hi
    r0, r1 = sequential_residual(prof.W32, x, y), sequential_residual(prof.W32, out, y)
    want = torch.stack([r0.pow(2).sum(dim=(2, 3, 4)).reshape(-1), r1.pow(2).sum(dim=(2, 3, 4)).reshape(-1),
                        r0.abs().amax(dim=(2, 3, 4)).reshape(-1), r1.abs().amax(dim=(2, 3, 4)).reshape(-1)], dim=1)
    rel = ((table[:, :4] - want).abs() / want.abs()).max()
    print(f"  stats table rel err {float(rel):.2e}  clamped {table[:, 4].tolist()} (float64 {counts.tolist()}, near a bound {near})")
    assert float(rel) <= 1e-12 and torch.equal(table[:, 4], counts)


def test_data_consistency_object():
    """DataConsistency.project / project_ are the kernel with the object's settings; last_stats is the finalised table."""
    prof, x, y = case("vec-8to48", "box")
    for kw, mode, iters in ((dict(), 0, 1), (dict(iterations=3, clamp=(LO, HI)), 1, 3),
                            (dict(iterations=2, clamp=(LO, HI), final="clamp"), 2, 2)):
        dc = CS.DataConsistency(**kw)
        want = x.clone()
        table = launch_project(prof, want, y, iters, mode)
        got = dc.project(x, y)
        assert got.data_ptr() != x.data_ptr() and torch.equal(got, want)
        assert torch.equal(dc.last_stats, table.cpu()) and dc.last_stats.device.type == "cpu"
        inplace = x.clone()
        assert dc.project_(inplace, y) is inplace and torch.equal(inplace, want)
    with pytest.raises(ValueError, match="differ outside depth"):
        CS.DataConsistency().project(x, y[:, :, :, :8])
    with pytest.raises(importlib.import_module("video-to-video-diffusion_amd.lib").CtsiError, match="contiguous fp32"):
        CS.DataConsistency().project_(x.transpose(3, 4), y)
