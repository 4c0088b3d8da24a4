"""The host dispatch of csrc/nufft.hip restated in Python, the named cases of tests/test_gpu_nufft_options.py and their points.

The restated predicates (csrc/nufft_plan_host.cpp: plan_type1, plan_type2, plan_level's per_run rule, make_tile_geom) take the
window of a case from the library's own host functions, so
tests/test_nudft_reference_host.py::test_geometry_of_the_cases can assert on a machine without a GPU that every case lands on the
route it is named for.  LDS per workgroup is 160 KB and the chip has 256 compute units, as on the MI355X.

The library's own planner (csrc/nufft_plan_host.cpp) is held to these functions field by field in tests/test_nufft_plan_host.py,
which hands LDS_BYTES and NUM_CU to the planner's check program.
"""
import math

import torch

LDS_BYTES = 160 * 1024
NUM_CU = 256
ORDER_WINDOW = 4096          # kOrderWindow
G2M_MAX_NF, G2M_MAX_H = 256, 32
DFT_MAX_NF = 128             # small_dft.hip: kDftMaxNf
MFMA_MAX_W, CELL_MAX_W, MAX_BANDS = 8, 8, 256
PAIR_FILL_BYTES = ((160 * 1024 // 16 + 1023) // 1024) * 1024 * 16


def window(nm, tol, dense=False):
    """(nf per axis, W): get_window's rule -- per-axis fine sizes, the width from the smallest upsampling ratio."""
    from efgp_hip import lib
    d = len(nm)
    dense = bool(dense) and d == 2
    nf = tuple(int(lib().efgp_fine_grid_size_nd(int(m), tol, d, int(dense))) for m in nm)
    W = int(lib().efgp_window_width_nd(tol, min(f / m for f, m in zip(nf, nm)), d))
    return nf, W


def _own_fft_supported(nf):
    for n in nf:
        if n < 1 or n > 4096:
            return False
        for r in (2, 3, 5):
            while n % r == 0:
                n //= r
        if n != 1:
            return False
    return True


def tile_geom(nf, W, channels, force_tile=0):
    """make_tile_geom -> (tiles per axis, tile size per axis) or None."""
    d = len(nf)
    cells_max = (LDS_BYTES - 4096) / (8.0 * channels)
    ext = int(math.floor(cells_max ** (1.0 / d)))
    while ext > W and float(ext) ** d > cells_max:
        ext -= 1
    tmax = force_tile if force_tile > 0 else ext - (W - 1)
    if tmax < 1 or (force_tile == 0 and tmax < 2):
        return None
    nt = tuple((n + tmax - 1) // tmax for n in nf)
    T = tuple((n + t - 1) // t for n, t in zip(nf, nt))
    if math.prod(nt) > 16384:
        return None
    return nt, T


def band_rule(nf, N, span_periods, forced=0):
    """plan_level's (band count, band height) or None: bands of at most 1 or 8 fine cells along axis 1, the first height with enough
    points per run -- 192 for one-cell bands, 24 for eight-cell ones; a forced height (1 | 8) from one point per run on.
    span_periods: extent of the points per axis in periods.  (A level the model already holds is not known here.)"""
    span = [s * n for s, n in zip(span_periods, nf)]
    for hb in (1, 8):
        if forced and forced != hb:
            continue
        n = 1
        while span[1] / n > hb - 1e-6 and n <= MAX_BANDS:
            n *= 2
        if n > MAX_BANDS:
            continue
        per_run = N / (n * max(1.0, span[0]))
        if per_run < (1.0 if forced else 192.0 if hb == 1 else 24.0):
            continue
        return n, hb
    return None


def band_level(nf, N, span_periods, forced):
    """band_rule's band count for a forced band height (0: the unforced rule), or None."""
    rule = band_rule(nf, N, span_periods, forced)
    return rule[0] if rule else None


def _after_spread(nm, nf, has_acc, env):
    """transform_fine for a request of the box nm: grid-to-modes, the pruned transform (fused with the accumulator or not), the full FFT."""
    d = len(nm)
    if (d == 2 and "EFGP_NO_GRID_TO_MODES" not in env and max(nf) <= G2M_MAX_NF and all(m // 2 <= G2M_MAX_H for m in nm)):
        return "g2m"
    smaller = any(min(2 * (m // 2) + 1, f) < f for m, f in zip(nm, nf))
    if smaller and _own_fft_supported(nf) and "EFGP_NO_PRUNED_FFT" not in env:
        return "pruned_from_acc" if has_acc and "EFGP_NO_FFT_FROM_ACC" not in env else "pruned"
    return "fft"


def type1_route(nm, tol, N, channels, dense=False, layout_band=0, span_periods=None, env=(), normal=False):
    """(spreader, what follows it) of one type-1 pass: plan_type1.  nm: the (larger) requested box; layout_band: 0 no point layout,
    1 | 8 a layout with that band height forced, -1 a layout and the unforced rule; normal: generated normal strengths."""
    nf, W = window(nm, tol, dense)
    d = len(nm)
    cells = math.prod(nf)
    lds_bytes = channels * cells * 8
    use_lds = lds_bytes <= LDS_BYTES and N > 0
    if (layout_band and d == 2 and W <= MFMA_MAX_W and N >= 32768 and "EFGP_NO_MFMA_SPREAD" not in env
            and band_level(nf, N, span_periods, max(layout_band, 0))):
        return "layout", _after_spread(nm, nf, True, env)
    if ("EFGP_CELLSORT" in env and not normal and d == 2 and W <= CELL_MAX_W and cells <= 16384 and N > 0
            and tile_geom(nf, W, channels, 1)):
        return "cells", _after_spread(nm, nf, False, env)           # (the library also wants degree <= W + 4: not visible from here)
    if not use_lds and N >= 32768 and "EFGP_NO_TILES" not in env and tile_geom(nf, W, channels):
        return "tiles", _after_spread(nm, nf, True, env)
    if not use_lds:
        return "global", _after_spread(nm, nf, False, env)
    use_pad, raw48 = _lds_slabs(nf, W, tol, N, channels, env, normal)[:2]
    return ("lds_pad_raw48" if raw48 else "lds_pad_61" if use_pad else "lds_plain"), _after_spread(nm, nf, False, env)


def _lds_slabs(nf, W, tol, N, channels, env, normal):
    """plan_lds_or_global for a grid inside LDS: (padded rows, 48-bit raw sums, workgroups, points per workgroup)."""
    cells = math.prod(nf)
    lds_bytes = channels * cells * 8
    per_cu = max(1, min(2, LDS_BYTES // max(lds_bytes, 1)))
    nwg = max(1, min(NUM_CU * per_cu, (N + 1023) // 1024))
    per = (N + nwg - 1) // nwg
    pad_bytes = channels * (cells // nf[-1]) * (nf[-1] + W - 1) * 8
    use_pad = pad_bytes + 4608 <= LDS_BYTES and "EFGP_NO_PAD" not in env
    raw48 = use_pad and per * 2.0 ** -47 <= 0.01 * tol and "EFGP_NO_RAW48" not in env and not normal
    return use_pad, raw48, nwg, per


def class_order_wanted(route, d, N, env=()):
    """The plan's bank-balanced processing order: kOrderWindow * 64 points or more, d >= 2, on the padded-row spreaders (type 1)
    or the halo gather that is not the pair gather (type 2).  route: a spreader of type1_route or a gather of type2_route."""
    return (route in ("lds_pad_raw48", "lds_pad_61", "halo") and d >= 2 and N >= ORDER_WINDOW * 64
            and "EFGP_NO_CLASS_ORDER" not in env)


def type2_route(nm, tol, N, B, real_only, dense=False, env=()):
    """(how the fine grid is made, which gather reads it): plan_type2."""
    nf, W = window(nm, tol, dense)
    d = len(nm)
    cells = math.prod(nf)
    direct = (real_only and B == 1 and d == 2 and max(nf) <= DFT_MAX_NF and max(nm) <= 64 and "EFGP_NO_DIRECT_DFT" not in env)
    lds_bytes = cells * (8 if real_only else 16)
    halo = math.prod(f + W - 1 for f in nf) * 8
    use_halo = real_only and halo <= LDS_BYTES and "EFGP_NO_HALO" not in env
    if use_halo:
        lds_bytes = halo
    pair_bytes = 2 * (nf[0] + W - 1) * ((nf[1] + 2 * ((W + 1) // 2) + 1) & ~1) * 8 if d == 2 else 0
    use_pair = use_halo and d == 2 and pair_bytes <= LDS_BYTES and "EFGP_NO_PAIR_GATHER" not in env
    if use_pair:
        lds_bytes = pair_bytes
    use_image = direct and use_pair and pair_bytes <= PAIR_FILL_BYTES and "EFGP_NO_GATHER_IMAGE" not in env
    smaller = any(min(2 * (m // 2) + 1, f) < f for m, f in zip(nm, nf))
    grid = ("image" if use_image else "direct" if direct else
            "pruned" if smaller and _own_fft_supported(nf) and "EFGP_NO_PRUNED_FFT" not in env else "fft")
    use_lds = lds_bytes <= LDS_BYTES
    if not use_lds and N >= 32768 and "EFGP_NO_TILES" not in env and tile_geom(nf, W, 1 if real_only else 2):
        return grid, "tiles"
    return grid, ("pair" if use_pair else "halo" if use_halo else "lds" if use_lds else "l2")


# ---- the points ---------------------------------------------------------------------------------------------------------------
SPAN_PERIODS = (1.2, 1.0 + 2.0 / 70)      # extent of points() per axis in periods: axis 0, every other axis


def edge_coords(period):
    """Both ends of a period and points within half a fine cell of them (cells are period / 32 ... period / 192 wide)."""
    vals = [0.0, period]
    for e in (period / 300, period / 140, period / 70):
        vals += [e, -e, period - e, period + e]
    return torch.tensor(vals, dtype=torch.float64)


_POINTS = {}


def points(d, N, h, xcen=None):
    """-> (x (N, d), number of edge points, slice of the clustered points).  Edge points first: every combination of edge
    coordinates (d = 3: of the six outermost), then an edge coordinate on one axis and random ones on the others.  A quarter of the
    points inside one fine cell, the first two of them equal.  The rest uniform over one period, over 1.2 periods on axis 0 -- the
    set spans more than a period on every axis.  With `xcen` the same set is laid around that centre."""
    key = (d, N, h, None if xcen is None else tuple(xcen))
    if key not in _POINTS:
        g = torch.Generator().manual_seed(4321 + 10 * d + N)
        P = 1.0 / h
        e = edge_coords(P)
        if d == 1:
            special = e[:, None]
        else:
            ee = e if d == 2 else torch.stack([e[0], e[1], e[11], e[12], e[3], e[6]])
            combos = torch.cartesian_prod(*([ee] * d))
            mixed = []
            for a in range(d):
                m = torch.rand(e.numel(), d, generator=g, dtype=torch.float64) * P
                m[:, a] = e
                mixed.append(m)
            special = torch.cat([combos] + mixed)
        n_edge = min(special.shape[0], N)
        n_cl = N // 4
        c0 = torch.rand(1, d, generator=g, dtype=torch.float64) * P
        cluster = c0 + (P / 400) * torch.rand(n_cl, d, generator=g, dtype=torch.float64)
        if n_cl > 1:
            cluster[1] = cluster[0]
        rest = torch.rand(max(N - n_edge - n_cl, 0), d, generator=g, dtype=torch.float64) * P
        if rest.shape[0]:
            rest[:, 0] = rest[:, 0] * 1.2 - 0.1 * P
            rest[0, 0], rest[-1, 0] = -0.1 * P, 1.1 * P          # the extent band_level() is told about
        x = torch.cat([special[:n_edge], cluster, rest])[:N]
        if xcen is not None:
            x = x + torch.tensor([float(v) for v in xcen], dtype=torch.float64)[None, :]
        _POINTS[key] = (x.contiguous(), n_edge, slice(n_edge, n_edge + n_cl))
    return _POINTS[key]


def compared_points(N, n_edge, cluster):
    """Type-2 outputs are compared on every point of a 3000-point case, else on every 11th plus the edge and clustered points."""
    if N <= 3000:
        return torch.arange(N)
    return torch.unique(torch.cat([torch.arange(0, N, 11), torch.arange(n_edge), torch.arange(cluster.start, cluster.stop)]))


# ---- the named cases ----------------------------------------------------------------------------------------------------------
# type 1: name -> (box, tol, N, complex strengths, h, expected (spreader, what follows), extra keywords of type1_route)
TYPE1 = {
    "lds_pad_raw48_real": ((23, 45), 1e-7, 3000, False, 0.5, ("lds_pad_raw48", "g2m"), {}),
    "lds_pad_raw48_cplx": ((23, 45), 1e-7, 3000, True, 0.5, ("lds_pad_raw48", "g2m"), {}),
    "lds_pad_61": ((12, 19), 1e-12, 3000, True, 0.37, ("lds_pad_61", "g2m"), {}),
    "lds_plain": ((40, 33), 1e-9, 3000, True, 0.37, ("lds_plain", "g2m"), {}),
    "global_2d": ((30, 45), 1e-7, 3000, True, 0.5, ("global", "g2m"), {}),
    "global_3d": ((10, 13, 16), 1e-5, 3000, False, 0.37, ("global", "pruned"), {}),
    "tiles_g2m": ((30, 45), 1e-7, 32768, True, 0.5, ("tiles", "g2m"), {}),
    "tiles_pruned": ((45, 70), 1e-7, 32768, False, 0.37, ("tiles", "pruned_from_acc"), {}),
    "tiles_3d": ((21, 12, 9), 1e-6, 32768, False, 0.5, ("tiles", "pruned_from_acc"), {}),
    "cells": ((23, 45), 1e-7, 3000, False, 0.5, ("cells", "g2m"), {"env": ("EFGP_CELLSORT",)}),
    "layout_g2m_band8": ((23, 45), 1e-7, 32768, False, 0.5, ("layout", "g2m"), {"layout_band": 8}),
    "layout_g2m_band1": ((23, 45), 1e-7, 32768, False, 0.5, ("layout", "g2m"), {"layout_band": 1}),
    "layout_pruned_band8": ((45, 70), 1e-7, 32768, False, 0.37, ("layout", "pruned_from_acc"), {"layout_band": 8}),
    # one-cell bands on the 128 x 192 grid: 256 bands x 154 cells of axis 0 need 39,322 points for one point per run
    "layout_pruned_band1": ((45, 70), 1e-7, 40960, False, 0.37, ("layout", "pruned_from_acc"), {"layout_band": 1}),
}

# type 2: name -> (box, tol, N, batch (None: one unbatched row), real_only, h, expected (grid, gather))
TYPE2 = {
    "cplx_lds": ((23, 45), 1e-7, 3000, None, False, 0.5, ("pruned", "lds")),
    "cplx_l2_2d": ((30, 45), 1e-7, 3000, None, False, 0.5, ("pruned", "l2")),
    "cplx_l2_3d": ((10, 13, 16), 1e-5, 3000, None, False, 0.37, ("pruned", "l2")),
    "cplx_tiles_2d": ((30, 45), 1e-7, 32768, None, False, 0.5, ("pruned", "tiles")),
    "cplx_tiles_3d": ((21, 12, 9), 1e-6, 32768, None, False, 0.5, ("pruned", "tiles")),
    "real_pair_fill": ((23, 45), 1e-7, 3000, 2, True, 0.5, ("pruned", "pair")),
    "real_pair_fill_even": ((22, 45), 1e-7, 3000, 2, True, 0.5, ("pruned", "pair")),
    "real_halo_direct": ((33, 40), 1e-7, 3000, None, True, 0.37, ("direct", "halo")),
    "real_halo_fft": ((33, 40), 1e-7, 3000, 2, True, 0.37, ("pruned", "halo")),
    "real_lds_plain": ((40, 70), 1e-7, 3000, None, True, 0.37, ("pruned", "lds")),
    "real_tiles_2d": ((45, 70), 1e-7, 32768, None, True, 0.37, ("pruned", "tiles")),
    "real_tiles_3d": ((21, 12, 9), 1e-6, 32768, None, True, 0.5, ("pruned", "tiles")),
    "real_1d_even": ((36,), 1e-7, 3000, None, True, 0.5, ("pruned", "halo")),
    "real_1d_odd": ((35,), 1e-7, 3000, None, True, 0.5, ("pruned", "halo")),
}
