"""A compact, machine-independent fingerprint of a gradient tensor, so that reference gradients can be stored as small
golden vectors: tensors of at most FULL elements are kept whole; larger ones become K projections onto fixed
pseudo-random directions (the sin-hash of oracle.ref_ops._hash_uniform: no RNG state, no imports) plus their L2 norm.  Two gradients whose sketches
agree to a relative L2 of e agree in every stored direction to that precision."""
import torch

FULL, K = 512, 48


def _hash_uniform(numel: int, key: float) -> torch.Tensor:
    i = torch.arange(numel, dtype=torch.float64)
    v = torch.sin(i * 12.9898 + key) * 43758.5453
    return v - torch.floor(v)


def grad_sketch(g: torch.Tensor, index: int) -> torch.Tensor:
    """float64 sketch of gradient `g`, the `index`-th parameter in named_parameters() order."""
    v = g.detach().reshape(-1).double().cpu()
    if v.numel() <= FULL:
        return v
    p = (2.0 * _hash_uniform(K * v.numel(), 1000.0 + 7.31 * index) - 1.0).reshape(K, v.numel())
    return torch.cat([p @ v, v.norm().reshape(1)])
