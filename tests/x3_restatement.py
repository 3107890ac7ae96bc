"""The bf16x3 arithmetic restated in torch (a helper, not a test).

split(t): hi = bf16(t) round-to-nearest-even, lo = bf16(t - hi), both returned in t's dtype.  For an fp32 t the subtraction
is exact in fp32; the tests feed float64 copies of fp32 tensors, where it is exact a fortiori.

conv3d_x3 / conv_transpose3d_x3: xh wh + xh wl + xl wh, each a convolution in the caller's dtype (float64 in the tests, so
what remains is the split's own error); bias added once.  `terms=1` keeps xh wh only (single-term bf16), `terms=4` adds
xl wl.

x3_oracle(): a context manager that replaces the oracle's `R.F` by a namespace forwarding everything to
torch.nn.functional except conv3d and conv_transpose3d, which evaluate the split products; `R.F` is restored on exit.
"""
import contextlib
import types

import torch
import torch.nn.functional as F

from oracle import ref_ops as R


def split(t: torch.Tensor):
    hi = t.to(torch.bfloat16).to(t.dtype)
    lo = (t - hi).to(torch.bfloat16).to(t.dtype)
    return hi, lo


def _x3(fn, x, w, bias, terms, kw):
    xh, xl = split(x)
    wh, wl = split(w)
    y = fn(xh, wh, None, **kw)
    if terms >= 3:
        y = y + (fn(xh, wl, None, **kw) + fn(xl, wh, None, **kw))
    if terms >= 4:
        y = y + fn(xl, wl, None, **kw)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1, 1)
    return y


def conv3d_x3(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1, terms=3):
    return _x3(F.conv3d, x, w, bias, terms, dict(stride=stride, padding=padding, dilation=dilation, groups=groups))


def conv_transpose3d_x3(x, w, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1, terms=3):
    return _x3(F.conv_transpose3d, x, w, bias, terms,
               dict(stride=stride, padding=padding, output_padding=output_padding, groups=groups, dilation=dilation))


class _Shim(types.SimpleNamespace):
    def __getattr__(self, name):          # everything but the two convolutions
        return getattr(F, name)


@contextlib.contextmanager
def x3_oracle(terms: int = 3):
    shim = _Shim(conv3d=lambda *a, **k: conv3d_x3(*a, terms=terms, **k),
                 conv_transpose3d=lambda *a, **k: conv_transpose3d_x3(*a, terms=terms, **k))
    old = R.F
    R.F = shim
    try:
        yield shim
    finally:
        R.F = old
