"""Exact non-uniform DFTs with every option of the HIP transforms, in plain float64 / complex128 torch on the CPU.

    type1:  f[k] = sum_n c_n                 exp(isign * 2 pi i h k.(x_n - xcen))
    type2:  c_n  = sum_k (f * mode_scale)[k] exp(isign * 2 pi i h k.(x_n - xcen))

Per axis k runs over -(n // 2) .. (n - 1) // 2.  modeord = 0 stores it in that order, modeord = 1 in FFT order
(0 .. (n - 1) // 2, then -(n // 2) .. -1).  Shapes are per-axis tuples, batches lead.  The phases are built from this
definition for every option -- no conjugation or shift identity of oracle/efgp_oracle.py is used, those identities are what
tests/test_nudft_reference_host.py checks.  Chunked over the points as the oracle is.
"""
import math

import torch

_RD = torch.float64
_CD = torch.complex128


def mode_numbers(n, modeord):
    """The integer k stored at each slot of an axis of n modes."""
    n = int(n)
    if modeord:
        return torch.cat([torch.arange(0, (n - 1) // 2 + 1), torch.arange(-(n // 2), 0)]).to(_RD)
    return torch.arange(-(n // 2), (n - 1) // 2 + 1).to(_RD)


def _points(x, xcen):
    x = torch.as_tensor(x, dtype=_RD)
    if x.ndim == 1:
        x = x[:, None]
    if xcen is not None:
        x = x - torch.as_tensor([float(v) for v in xcen], dtype=_RD)[None, :]
    return x


def _tables(x, h, shape, isign, modeord):
    """Per axis (n_points, n_modes): exp(isign * 2 pi i h k x)."""
    tabs = []
    for a, n in enumerate(shape):
        ang = (float(isign) * 2.0 * math.pi * float(h)) * x[:, a, None] * mode_numbers(n, modeord)[None, :]
        tabs.append(torch.complex(torch.cos(ang), torch.sin(ang)))
    return tabs


def type1(x, h, c, shape, isign=-1, modeord=0, xcen=None, chunk=1 << 13):
    """c (N,) or (B, N), real or complex -> (B?, *shape) complex128."""
    assert isign in (-1, 1)
    x = _points(x, xcen)
    shape = tuple(int(m) for m in shape)
    assert x.shape[1] == len(shape)
    c = torch.as_tensor(c)
    batched = c.ndim > 1
    cc = c.reshape(-1, x.shape[0]).to(_CD)
    out = torch.zeros((cc.shape[0],) + shape, dtype=_CD)
    for lo in range(0, x.shape[0], chunk):
        t = _tables(x[lo:lo + chunk], h, shape, isign, modeord)
        cb = cc[:, lo:lo + chunk]
        if len(shape) == 1:
            out += cb @ t[0]
        elif len(shape) == 2:
            out += torch.einsum("bnk,nl->bkl", cb[:, :, None] * t[0][None], t[1])
        else:
            out += torch.einsum("bnkl,nm->bklm", (cb[:, :, None] * t[0][None])[:, :, :, None] * t[1][None, :, None, :], t[2])
    return out if batched else out[0]


def type2(x, h, f, shape, isign=+1, modeord=0, xcen=None, mode_scale=None, chunk=1 << 13):
    """f (prod,) | (*shape) | (B, ...) -> (N,) | (B, N) complex128; mode_scale (prod,) | (*shape) multiplies every row of f."""
    assert isign in (-1, 1)
    x = _points(x, xcen)
    shape = tuple(int(m) for m in shape)
    assert x.shape[1] == len(shape)
    f = torch.as_tensor(f).to(_CD)
    batched = not (f.ndim == 1 or tuple(f.shape) == shape)
    ff = f.reshape((-1,) + shape)
    if mode_scale is not None:
        ff = ff * torch.as_tensor(mode_scale).to(_CD).reshape((1,) + shape)
    out = torch.empty((ff.shape[0], x.shape[0]), dtype=_CD)
    for lo in range(0, x.shape[0], chunk):
        hi = min(x.shape[0], lo + chunk)
        t = _tables(x[lo:hi], h, shape, isign, modeord)
        if len(shape) == 1:
            out[:, lo:hi] = ff @ t[0].T
        elif len(shape) == 2:
            out[:, lo:hi] = torch.einsum("bnl,nl->bn", torch.einsum("bkl,nk->bnl", ff, t[0]), t[1])
        else:
            g = torch.einsum("bklm,nm->bnkl", ff, t[2])
            out[:, lo:hi] = torch.einsum("bnk,nk->bn", torch.einsum("bnkl,nl->bnk", g, t[1]), t[0])
    return out if batched else out[0]
