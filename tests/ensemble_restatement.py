"""The ensemble kernels' arithmetic restated with torch: the sequential Welford recurrence of
csrc/ensemble.hip in the dtype of its input, the float64 two-pass statistics it is judged against, and the bounds.

Yardsticks (tests/test_gpu_ensemble_ops.py, tests/test_gpu_ensemble.py), all against float64 two-pass statistics of the same fp32
members, per element:
  mean  |kernel - ref| <= 2 max|members.mean(0) in torch fp32 - ref| + one fp32 ulp of the float64 mean at that element;
  std   |kernel - ref| <= 2 max|this file's recurrence in torch fp32 - ref| + one fp32 ulp of max_k |x_k| over the tensor.
An fp32 running mean bounds what any fp32 Welford can resolve, so the recurrence itself is the yardstick of the std; torch's own
`std` keeps a wider accumulator and is not comparable."""
import numpy as np
import torch


def welford(members: torch.Tensor, seen: int = 0, mean=None, m2=None):
    """(mean, m2) after folding members[0], members[1], ... (dim 0) into the state over `seen` earlier members, every
    operation rounded in the members' dtype: k = seen + r + 1, d = x - mean, mean += d / k, m2 += d (x - mean).  Member 1
    sets mean = x, m2 = 0."""
    for r in range(members.shape[0]):
        x = members[r]
        if seen + r == 0:
            mean, m2 = x.clone(), torch.zeros_like(x)
            continue
        k = torch.tensor(float(seen + r + 1), dtype=x.dtype, device=x.device)
        d = x - mean
        mean = mean + d / k
        m2 = m2 + d * (x - mean)
    return mean, m2


def std_of(m2: torch.Tensor, members: int, unbiased: bool = True) -> torch.Tensor:
    """sqrt(max(m2, 0) / (members - unbiased)) in m2's dtype, 0 for one member."""
    if members == 1:
        return torch.zeros_like(m2)
    denom = torch.tensor(float(members - (1 if unbiased else 0)), dtype=m2.dtype, device=m2.device)
    return torch.sqrt(torch.where(m2 < 0, torch.zeros_like(m2), m2) / denom)


def two_pass(members: torch.Tensor, unbiased: bool = True):
    """float64 (mean, std) over dim 0, two passes."""
    x = members.double()
    k = x.shape[0]
    mean = x.sum(0) / k
    if k == 1:
        return mean, torch.zeros_like(mean)
    return mean, torch.sqrt(((x - mean) ** 2).sum(0) / (k - (1 if unbiased else 0)))


def ulp32(t: torch.Tensor) -> torch.Tensor:
    """One fp32 ulp at |t| (float64 tensor in, float64 tensor out)."""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def check_mean_std(tag, mean, std, members, unbiased=True, log=print):
    """Assert the two yardsticks of the module docstring for a kernel's (mean, std) of `members` (K, ...); returns the two
    ratios (largest error over its bound), which are printed first."""
    ref_mean, ref_std = two_pass(members, unbiased)
    k = members.shape[0]
    e_torch = float((members.mean(0).double() - ref_mean).abs().max())
    bound_mean = 2.0 * e_torch + ulp32(ref_mean)
    err_mean = (mean.double() - ref_mean).abs()
    w_mean, w_m2 = welford(members)
    e_rest = float((std_of(w_m2, k, unbiased).double() - ref_std).abs().max())
    bound_std = 2.0 * e_rest + float(np.spacing(np.float32(float(members.abs().max()))))
    err_std = (std.double() - ref_std).abs()
    r_mean, r_std = float((err_mean / bound_mean).max()), float(err_std.max()) / bound_std
    log(f"  {tag}: mean err {float(err_mean.max()):.3e} (torch fp32 {e_torch:.3e}) ratio {r_mean:.3f} | std err "
        f"{float(err_std.max()):.3e} (recurrence in torch fp32 {e_rest:.3e}) bound {bound_std:.3e} ratio {r_std:.3f}")
    assert r_mean <= 1.0, (tag, "mean", r_mean)
    assert r_std <= 1.0, (tag, "std", r_std)
    return r_mean, r_std
