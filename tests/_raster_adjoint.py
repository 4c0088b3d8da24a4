"""The raster type-1 transform (csrc/raster_adjoint.hip) and its slab plan (plan_raster_type1 in csrc/raster_plan_host.cpp), restated
on the CPU.

    out[b, k] = sum_j values[b, j] cell_scale[j] exp(isign 2 pi i sum_a h[a] k_a (axes[a][j_a] - xcen[a]))

`exact` is tests/_nudft.type1 at the meshgrid points over the cells whose scale is not zero; `plan` restates the planner field by
field.  CHUNK is the kernel's reduction chunk over the leading raster axis, SEGMENT the cells of the last axis per GEMM segment.
"""
import math

import torch

from _nudft import type1 as _nudft_type1
from _raster import DEFAULT_WORKSPACE, KSTEP, MAX_AXIS, MAX_BATCH, MAX_MODES, TILE, make_case, meshgrid_points

CHUNK = 16
SEGMENT = 256                # cells of the last raster axis per GEMM segment


def plan(n_modes, n_axis, nbatch=1, max_workspace_bytes=0):
    """The type-1 planner's fields as a dict, or None where it refuses the case."""
    d = len(n_modes)
    if not (1 <= d <= 3 and len(n_axis) == d and 1 <= nbatch <= MAX_BATCH and max_workspace_bytes >= 0):
        return None
    if any(not 1 <= m <= MAX_MODES for m in n_modes) or any(not 1 <= n <= MAX_AXIS for n in n_axis):
        return None
    kpad = [-(-m // KSTEP) * KSTEP for m in n_modes]
    table_bytes = sum(2 * 8 * n * k for n, k in zip(n_axis, kpad))
    modes = math.prod(n_modes)
    # per row of the leading axis: T1 (and T2) complex, and 16 bytes of partial sums per mode and chunk of CHUNK = 16 rows
    # plus one copy of the GEMM's output per segment where the last axis has more than one
    segs = -(-n_axis[-1] // SEGMENT)
    segs = segs if segs > 1 else 0
    row_bytes = 0
    if d == 1:
        table_bytes += 16 * nbatch * segs * n_modes[0]
    elif d == 2:
        row_bytes = nbatch * (16 * (1 + segs) * n_modes[1] + modes)
    else:
        row_bytes = nbatch * (16 * ((1 + segs) * n_axis[1] * n_modes[2] + n_modes[1] * n_modes[2]) + modes)
    cap = max_workspace_bytes or DEFAULT_WORKSPACE
    least = table_bytes + TILE * row_bytes
    if least >= 1 << 62 or cap < least:
        return None
    slab_rows = -(-n_axis[0] // TILE) * TILE
    if row_bytes:
        slab_rows = min(slab_rows, (cap - table_bytes) // row_bytes // TILE * TILE)
    return dict(Kpad=tuple(kpad), table_bytes=table_bytes, row_bytes=row_bytes, slab_rows=slab_rows, slabs=-(-n_axis[0] // slab_rows),
                workspace_bytes=table_bytes + slab_rows * row_bytes, least_bytes=least)


def make_values(shape, n_axis, hrel, seed, nbatch=1, masked=0.0, scaled=False, center=True):
    """Axes, spacings and centre of `_raster.make_case` (phase 70, unsorted axes with a duplicate) with seeded raster values
    (nbatch, *n_axis) and a cell scale: None, or random in [0.5, 1.5) (`scaled`) with a fraction `masked` of exact zeros."""
    axes, hs, xcen, _, _ = make_case(shape, n_axis, hrel, seed=seed, nbatch=1, scale=False, center=center)
    g = torch.Generator().manual_seed(seed + 10_000)
    values = torch.randn((nbatch,) + tuple(n_axis), dtype=torch.float64, generator=g)
    scale = None
    if scaled or masked > 0:
        scale = torch.rand(tuple(n_axis), dtype=torch.float64, generator=g) + 0.5 if scaled else torch.ones(tuple(n_axis), dtype=torch.float64)
        if masked > 0:
            scale = scale * (torch.rand(tuple(n_axis), dtype=torch.float64, generator=g) >= masked)
    return axes, hs, xcen, values, scale


def exact(axes, hs, values, shape, isign, modeord, xcen, scale=None):
    """_nudft.type1 at the meshgrid points over the cells of non-zero scale -> (B, *shape) complex and sum_j |v_j s_j| per row.
    Axis a is rescaled by the power of two hs[a] / hs[0] (exact), since the exact sums take one spacing."""
    ratio = [hs[a] / hs[0] for a in range(len(shape))]
    assert all(math.log2(r).is_integer() for r in ratio)
    pts = meshgrid_points([torch.as_tensor(x, dtype=torch.float64) * r for x, r in zip(axes, ratio)])
    xc = None if xcen is None else [c * r for c, r in zip(xcen, ratio)]
    vv = torch.as_tensor(values, dtype=torch.float64).reshape(-1, pts.shape[0])
    if scale is not None:
        s = torch.as_tensor(scale, dtype=torch.float64).reshape(-1)
        keep = s != 0
        pts, vv = pts[keep], vv[:, keep] * s[keep][None]
    out = _nudft_type1(pts, hs[0], vv, shape, isign=isign, modeord=modeord, xcen=xc)
    return out.reshape((vv.shape[0],) + tuple(shape)), vv.abs().sum(dim=1)
