"""The raster transform (csrc/raster_dft.hip) and its slab plan (csrc/raster_plan_host.cpp), restated in float64 torch on the CPU.

    out[b, j0..] = Re sum_k (f[b,k] * mode_scale[k]) exp(isign 2 pi i sum_a h[a] k_a (axes[a][j_a] - xcen[a]))

One phase table per axis from `_nudft.mode_numbers`, one einsum over all of them: the separation the kernels rely on, and nothing
of how they stage it.  `plan` restates the planner field by field.
"""
import math

import torch

from _nudft import mode_numbers
from _nudft import type2 as _nudft_type2

_RD = torch.float64
_CD = torch.complex128

TILE = 16                    # rows of a slab come in whole output tiles
KSTEP = 4                    # the tables are padded to the K of the f64 matrix instruction
DEFAULT_WORKSPACE = 256 << 20
MAX_MODES, MAX_AXIS, MAX_BATCH = 1 << 20, (1 << 31) - 1, 1 << 16


def tables(axes, h, shape, isign=+1, modeord=0, xcen=None):
    """Per axis (n_axis, n_modes) complex128: exp(isign 2 pi i h_a k (x - xcen_a))."""
    d = len(shape)
    hs = [float(v) for v in h] if hasattr(h, "__len__") else [float(h)] * d
    tabs = []
    for a in range(d):
        x = torch.as_tensor(axes[a], dtype=_RD) - (0.0 if xcen is None else float(xcen[a]))
        ang = (float(isign) * 2.0 * math.pi * hs[a]) * x[:, None] * mode_numbers(shape[a], modeord)[None, :]
        tabs.append(torch.complex(torch.cos(ang), torch.sin(ang)))
    return tabs


def type2(axes, h, f, shape, isign=+1, modeord=0, xcen=None, mode_scale=None):
    """f (prod,) | (*shape) | (B, ...) -> float64 (*n_axis) | (B, *n_axis)."""
    shape = tuple(int(m) for m in shape)
    f = torch.as_tensor(f).to(_CD)
    batched = not (f.ndim == 1 or tuple(f.shape) == shape)
    ff = f.reshape((-1,) + shape)
    if mode_scale is not None:
        ff = ff * torch.as_tensor(mode_scale).to(_CD).reshape((1,) + shape)
    t = tables(axes, h, shape, isign, modeord, xcen)
    spec = {1: "bk,ik->bi", 2: "bkl,ik,jl->bij", 3: "bklm,ik,jl,nm->bijn"}[len(shape)]
    out = torch.einsum(spec, ff, *t).real.contiguous()
    return out if batched else out[0]


def meshgrid_points(axes):
    """(prod n_axis, d) coordinates of the raster in row-major ("ij") order."""
    return torch.stack(torch.meshgrid(*[torch.as_tensor(a, dtype=_RD) for a in axes], indexing="ij"), dim=-1).reshape(-1, len(axes))


def plan(n_modes, n_axis, nbatch=1, max_workspace_bytes=0):
    """The planner's fields as a dict, or None where it refuses the case."""
    d = len(n_modes)
    if not (1 <= d <= 3 and len(n_axis) == d and 1 <= nbatch <= MAX_BATCH and max_workspace_bytes >= 0):
        return None
    if any(not 1 <= m <= MAX_MODES for m in n_modes) or any(not 1 <= n <= MAX_AXIS for n in n_axis):
        return None
    kpad = [-(-m // KSTEP) * KSTEP for m in n_modes]
    table_bytes = sum(2 * 8 * n * k for n, k in zip(n_axis, kpad))
    row_bytes = 0
    if d == 1:
        table_bytes += 16 * nbatch * kpad[0]
    elif d == 2:
        row_bytes = 16 * nbatch * kpad[1]
    else:
        row_bytes = 16 * nbatch * (n_modes[1] * n_modes[2] + n_axis[1] * kpad[2])
    cap = max_workspace_bytes or DEFAULT_WORKSPACE
    least = table_bytes + TILE * row_bytes
    if least >= 1 << 62 or cap < least:
        return None
    slab_rows = -(-n_axis[0] // TILE) * TILE
    if row_bytes:
        slab_rows = min(slab_rows, (cap - table_bytes) // row_bytes // TILE * TILE)
    return dict(Kpad=tuple(kpad), table_bytes=table_bytes, row_bytes=row_bytes, slab_rows=slab_rows, slabs=-(-n_axis[0] // slab_rows),
                workspace_bytes=table_bytes + slab_rows * row_bytes, least_bytes=least)


def make_case(shape, n_axis, hrel, seed, nbatch=1, scale=True, center=True, phase=70.0):
    """Seeded inputs with h_a (n_a // 2) max|x - xcen| <= phase on every axis; unsorted axes with one duplicate."""
    g = torch.Generator().manual_seed(seed)
    d = len(shape)
    h0 = 0.37
    hs = tuple(h0 * r for r in hrel)
    xcen = tuple(0.3 * (a + 1) * (-1) ** a for a in range(d)) if center else None
    axes = []
    for a in range(d):
        reach = phase / (hs[a] * max(1, shape[a] // 2))
        x = (torch.rand(n_axis[a], dtype=torch.float64, generator=g) * 2 - 1) * reach
        if n_axis[a] > 2:
            x[-1] = x[0]                               # a duplicate coordinate
        axes.append(x + (xcen[a] if center else 0.0))
    f = torch.complex(torch.randn((nbatch,) + tuple(shape), dtype=torch.float64, generator=g),
                      torch.randn((nbatch,) + tuple(shape), dtype=torch.float64, generator=g))
    sc = torch.complex(torch.rand(shape, dtype=torch.float64, generator=g) + 0.5,
                       torch.randn(shape, dtype=torch.float64, generator=g)) if scale else None
    return axes, hs, xcen, f, sc


def exact(axes, hs, f, shape, isign, modeord, xcen, mode_scale):
    """_nudft_type2 at the meshgrid points -> real (B, *n_axis) and sum_k |f_k scale_k| per row.  Axis a is rescaled by the
    power of two hs[a] / hs[0] (exact), since the exact sums take one spacing."""
    ratio = [hs[a] / hs[0] for a in range(len(shape))]
    assert all(math.log2(r).is_integer() for r in ratio)
    pts = meshgrid_points([torch.as_tensor(x, dtype=torch.float64) * r for x, r in zip(axes, ratio)])
    xc = None if xcen is None else [c * r for c, r in zip(xcen, ratio)]
    ff = f.reshape((-1,) + tuple(shape))
    val = _nudft_type2(pts, hs[0], ff, shape, isign=isign, modeord=modeord, xcen=xc, mode_scale=mode_scale)
    mag = (ff if mode_scale is None else ff * mode_scale[None]).abs().reshape(ff.shape[0], -1).sum(dim=1)
    return val.real.reshape((ff.shape[0],) + tuple(len(x) for x in axes)), mag
