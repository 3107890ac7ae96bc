"""Float64 restatement of classifier-free guidance, the specification the guidance tests hold the
engine to:

    eps_g = eps_u + s (eps_c - eps_u)
    eps   = phi eps_g std_b(eps_c) / std_b(eps_g) + (1 - phi) eps_g

std_b: per sample over (L, d, h, w), unbiased (torch.std's default), in float64; the factor is 1 where std_b(eps_g) == 0;
phi == 0 takes no statistics.  Plain torch on whatever device the inputs live; no engine code."""
import torch


def std_b(x: torch.Tensor) -> torch.Tensor:
    """Per-sample unbiased standard deviation in float64, shape (n,)."""
    return x.double().reshape(x.shape[0], -1).std(dim=1)


def guide(eps_c: torch.Tensor, eps_u: torch.Tensor, s: float) -> torch.Tensor:
    c, u = eps_c.double(), eps_u.double()
    return u + float(s) * (c - u)


def rescale_factor(eps_c: torch.Tensor, eps_g: torch.Tensor) -> torch.Tensor:
    """std_b(eps_c) / std_b(eps_g), 1 where std_b(eps_g) == 0; shape (n,)."""
    sc, sg = std_b(eps_c), std_b(eps_g)
    return torch.where(sg == 0, torch.ones_like(sg), sc / torch.where(sg == 0, torch.ones_like(sg), sg))


def cfg_eps(eps_c: torch.Tensor, eps_u: torch.Tensor, s: float, phi: float = 0.0) -> torch.Tensor:
    """The guided (and for phi > 0 rescaled) noise prediction, float64."""
    g = guide(eps_c, eps_u, s)
    if float(phi) == 0.0:
        return g
    f = rescale_factor(eps_c, g).reshape(-1, *([1] * (g.dim() - 1)))
    return float(phi) * g * f + (1.0 - float(phi)) * g


def magnitude(eps_c: torch.Tensor, eps_u: torch.Tensor, s: float) -> torch.Tensor:
    """|s| (|eps_c| + |eps_u|) + |eps_u|: what the fp32 roundings of eps_u + s (eps_c - eps_u) are relative to."""
    c, u = eps_c.double().abs(), eps_u.double().abs()
    return abs(float(s)) * (c + u) + u
