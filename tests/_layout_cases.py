"""Case builders, restated host rules and references of tests/test_layout_cases_host.py and tests/test_gpu_spread_layout_edges.py:
the MFMA spreader (csrc/spread_mfma.hip) over the sorted point layout (csrc/points_layout.hip) at every window width, both band
heights and every run seam of its batch loop.  Host only (numpy / CPU tensors in float64); nothing here touches the GPU.

Every case is the smallest shape that crosses the seam it is named for, and its builder asserts on `layout_trace` that it does: a
case that stops crossing its seam fails instead of passing for nothing.

Restated here (the window (nf, W) and the band rule come from tests/_nufft_routes.py, the degree from WINDOWS below, which
tests/test_layout_cases_host.py holds to tools/nufft_plan_check.cpp):
  points_layout.hip   chunk_length(N, num_cu) (now csrc/nufft_plan_host.cpp); band = clamp(floor((y - lo1) * nbands / span)), band 0
                      when span == 0; key = band << 56 | top 56 bits of the order-preserving image of x0, stable sort (ties stay in
                      input order); chunks of at most chunk_length points that never cross a band
  spread_mfma.hip     bx = ceil(scale0 (x0 - xcen0) - W/2), by0 = ceil(scale1 (min y of the band - xcen1) - W/2),
                      off = ceil(scale1 (x1 - xcen1) - W/2) - by0 with 0 <= off <= HB (the kernel's LDS rows end at off = HB), a run
                      start wherever bx differs from the point before it inside a chunk (the first point of a chunk opens its tile
                      without a flush), batches of 64 points, MFMA groups of 4
  nufft_plan_host.cpp plan_level's adoption of a level the model already holds (band_rule_held)
Coordinates: X = scale (x - xcen) in fine cells, scale = h nf; u = X - W/2 is the coordinate whose ceil is the first stencil cell.
"""
import math

import numpy as np
import torch

import _nufft_routes as R

MIN_POINTS = 32768                 # plan_level: no layout below
MARGIN = 1e-3                      # designed points keep this many cells from every cell edge
RUN_COUNTS = (1, 2, 3, 4, 5, 59, 60, 61, 63, 64, 65, 67, 127, 128, 129, 191, 193)
NUM_CUS = (256, 304, 128)          # the CU counts the host test traces every builder at (MI355X, MI300X, a half chip)
DENSE_POINTS = 1000                # EFGP_DENSE_POINTS of the dense-window cases

# name -> (box, tol, dense rule, (nf, W, degree)): one window per width and degree arm of spread_mfma.hip's launch_w.  The W + 2 arm
# is reached by W = 2 (the degree search starts at 4), by the dense rule's finer grid (W = 7, degree 9: the fit's 45 x 45 box at
# 6e-8; the 23 x 23 box keeps W = 8 there) and by W = 3, 4, 5, 6 on the minimum grids of a 9 x 9 box.
WINDOWS = {
    "w2": ((23, 23), 1e-1, False, (48, 2, 4)),
    "w3": ((23, 23), 1e-2, False, (64, 3, 4)),
    "w4": ((23, 23), 1e-3, False, (64, 4, 5)),
    "w5": ((23, 23), 1e-4, False, (64, 5, 6)),
    "w6": ((23, 23), 1e-5, False, (64, 6, 7)),
    "w7": ((23, 23), 1e-6, False, (64, 7, 8)),
    "w8": ((23, 23), 1e-7, False, (64, 8, 9)),
    "w8_6e8": ((23, 23), 6e-8, False, (64, 8, 9)),
    "w7_dense": ((45, 45), 6e-8, True, (216, 7, 9)),
    "w3_deg5": ((9, 9), 6e-3, False, (32, 3, 5)),
    "w4_deg6": ((9, 9), 6e-4, False, (32, 4, 6)),
    "w5_deg7": ((9, 9), 3e-5, False, (32, 5, 7)),
    "w6_deg8": ((9, 9), 1.5e-6, True, (36, 6, 8)),
    "w8_box9": ((9, 9), 1e-7, False, (32, 8, 9)),
    "w5_box9": ((9, 9), 1e-4, False, (32, 5, 6)),
    "w8_box45": ((45, 45), 1e-7, False, (128, 8, 9)),
}
WIDTH_WINDOWS = ("w2", "w3", "w4", "w5", "w6", "w7", "w8")
ARM_WINDOWS = ("w7_dense", "w3_deg5", "w4_deg6", "w5_deg7", "w6_deg8")          # the W + 2 arm beyond W = 2


def degree_arm(W, degree):
    """The instantiation launch_w picks: DEG = W + 1, DEG = W + 2, or the run-time Horner loop (DEG = 0)."""
    return "W+1" if degree == W + 1 else "W+2" if degree == W + 2 else "run-time"


# ---- restated host rules ----------------------------------------------------------------------------------------------------------
def chunk_length(N, num_cu):
    waves = num_cu * (24 if N >= 4000000 else 8)
    rounds = max(1, (N + waves * 1536 - 1) // (waves * 1536))
    ln = (N + waves * rounds - 1) // (waves * rounds)
    return max(64, (ln + 63) // 64 * 64)


def enc_f64(v):
    """The order-preserving map double -> uint64 of the sort key."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def band_index(y, nbands):
    lo, hi = float(y.min()), float(y.max())
    span = hi - lo
    inv = nbands / span if span > 0.0 else 0.0
    return np.clip(np.floor((y - lo) * inv), 0, nbands - 1).astype(np.int64)


def band_rule_held(nf, N, span_periods, forced, held=()):
    """plan_level with the levels the model already holds: an eight-cell level takes a held level of twice or four times its band
    count (24 points per run of it or more) instead of sorting the points again."""
    rule = R.band_rule(nf, N, span_periods, forced)
    if rule is None or rule[1] != 8 or rule[0] in held:
        return rule
    n, span0 = rule[0], span_periods[0] * nf[0]
    for f in (2, 4):
        if n * f > R.MAX_BANDS or N / (n * f * max(1.0, span0)) < 24.0:
            break
        if n * f in held:
            return n * f, 8
    return rule


class Trace:
    """What the kernel sees of a point set: `order` (sorted position -> input index), per sorted point its band, first stencil cell
    `bx`, column offset `off`, position `pos` inside its chunk and whether it starts a run there; per chunk (start, count, band)."""

    def masks(self, chunk):
        """The per-batch run-start masks of one chunk, bit l = lane l, as the kernel's ballot gives them."""
        s, n = int(self.chunk_start[chunk]), int(self.chunk_count[chunk])
        flags = self.run_start[s:s + n]
        return [sum(1 << l for l in np.flatnonzero(flags[b0:b0 + 64]).tolist()) for b0 in range(0, n, 64)]

    def chunks(self):
        """[(sorted input indices, per-batch masks)] per chunk."""
        return [(self.order[s:s + n], self.masks(i)) for i, (s, n) in enumerate(zip(self.chunk_start.tolist(), self.chunk_count.tolist()))]

    def run_lengths(self):
        """Lengths of the (band, x cell) runs in sorted order, chunk seams ignored."""
        new = np.ones(self.bx.size, dtype=bool)
        new[1:] = (self.bx[1:] != self.bx[:-1]) | (self.band[1:] != self.band[:-1])
        return np.diff(np.append(np.flatnonzero(new), self.bx.size))

    def seams(self):
        """The seams of the batch loop this point set crosses."""
        pos, st, cnt = self.pos, self.run_start, self.chunk_count
        nstart = np.add.reduceat(st.astype(np.int64), np.flatnonzero(pos % 64 == 0))
        bpos = pos[pos % 64 == 0]
        blen = np.minimum(64, np.repeat(cnt, (cnt + 63) // 64) - bpos)
        later = bpos >= 64
        idle_any = bool(np.any(later & (nstart == 0)))
        idle_full = bool(np.any(later & (nstart == 0) & (blen == 64)))      # the branch-free whole-batch arm behind a first batch
        all_start = bool(np.any((later & (nstart == blen)) | (~later & (nstart == blen - 1) & (blen == 64))))
        last_of_band = np.ones(len(cnt), dtype=bool)
        last_of_band[:-1] = self.chunk_band[1:] != self.chunk_band[:-1]
        first_of_band = np.ones(len(cnt), dtype=bool)
        first_of_band[1:] = self.chunk_band[1:] != self.chunk_band[:-1]
        return {
            "group_k": sorted(set((pos[st] % 4).tolist())),
            "lane0_later_batch": bool(np.any(st & (pos % 64 == 0) & (pos >= 64))),
            "lane63": bool(np.any(st & (pos % 64 == 63))),
            "idle_batch_behind_first": idle_any,
            "idle_full_batch_behind_first": idle_full,
            "every_point_starts": all_start,
            "tails_mod4": sorted(set((cnt % 4).tolist())),
            "one_point_chunk": bool(np.any(cnt == 1)),
            "short_last_chunk": bool(np.any(last_of_band & ~first_of_band & (cnt < self.chunk_len))),
            "batches_per_chunk": int((cnt.max() + 63) // 64),
        }


def layout_trace(x, h, nf, W, nbands, num_cu, xcen=(0.0, 0.0), band_cells=None):
    """The layout of points x (N, 2) on the fine grid nf with window width W, in `nbands` bands, on a chip of num_cu compute units.
    With band_cells the kernel's bound 0 <= off <= band_cells is asserted on every point: beyond it the kernel writes outside its
    LDS rows, so no case may reach the GPU without this check."""
    x = np.ascontiguousarray(x.numpy() if torch.is_tensor(x) else x, dtype=np.float64)
    N = x.shape[0]
    t = Trace()
    band = band_index(x[:, 1], nbands)
    key = (band.astype(np.uint64) << np.uint64(56)) | (enc_f64(x[:, 0]) >> np.uint64(8))
    t.order = np.argsort(key, kind="stable")
    xs = x[t.order]
    t.band = band[t.order]
    t.nbands, t.N, t.W, t.nf = nbands, N, W, tuple(nf)
    t.chunk_len = chunk_length(N, num_cu)
    scale = (h * nf[0], h * nf[1])
    t.u0 = scale[0] * (xs[:, 0] - xcen[0]) - 0.5 * W
    t.u1 = scale[1] * (xs[:, 1] - xcen[1]) - 0.5 * W
    t.bx = np.ceil(t.u0).astype(np.int64)
    counts = np.bincount(t.band, minlength=nbands)
    t.band_count = counts
    band_start = np.concatenate([[0], np.cumsum(counts)])
    band_lo = np.full(nbands, np.inf)
    np.minimum.at(band_lo, t.band, xs[:, 1])
    by0 = np.ceil(scale[1] * (band_lo - xcen[1]) - 0.5 * W)
    t.off = (np.ceil(t.u1) - by0[t.band]).astype(np.int64)
    cs, cc, cb = [], [], []
    for b in range(nbands):
        for s in range(int(band_start[b]), int(band_start[b + 1]), t.chunk_len):
            cs.append(s)
            cc.append(min(t.chunk_len, int(band_start[b + 1]) - s))
            cb.append(b)
    t.chunk_start, t.chunk_count, t.chunk_band = np.array(cs), np.array(cc), np.array(cb)
    t.pos = np.arange(N) - np.repeat(t.chunk_start, t.chunk_count)
    t.run_start = np.zeros(N, dtype=bool)
    t.run_start[1:] = t.bx[1:] != t.bx[:-1]
    t.run_start[t.pos == 0] = False                    # b0 == 0: the chunk's first point sets cur_bx, nothing is flushed
    assert int(t.chunk_count.sum()) == N and np.all(np.diff(t.band) >= 0)
    if band_cells is not None:
        assert t.off.min() >= 0 and t.off.max() <= band_cells, (int(t.off.min()), int(t.off.max()), band_cells)
    return t


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def strengths(N, seed, rows=None, cplx=False):
    """|c| in [0.5, 1.5] with a random sign; complex rows: both parts drawn that way."""
    g = torch.Generator().manual_seed(seed)
    shape = (N,) if rows is None else (rows, N)

    def real():
        return (0.5 + torch.rand(shape, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(torch.float64)
    return torch.complex(real(), real()) if cplx else real()


class Case:
    """One point set on one plan: x (N, 2), grid spacing h, tolerance, mode box nm, plan centre, forced band height, dense rule."""

    def __init__(self, name, x, h, window, band_cells, xcen=None, layout=True, held=(), seed=1):
        nm, tol, dense, (nf, W, degree) = WINDOWS[window]
        self.name, self.window, self.h, self.tol, self.nm, self.dense = name, window, float(h), tol, nm, dense
        self.x = torch.as_tensor(x, dtype=torch.float64).contiguous()
        self.N = self.x.shape[0]
        self.xcen = None if xcen is None else tuple(float(v) for v in xcen)
        self.band_cells, self.nf, self.W, self.degree, self.seed = band_cells, (nf, nf), W, degree, seed
        self.held = tuple(held)
        self.expect_layout = layout
        self.env = {"EFGP_MFMA_BAND_CELLS": str(band_cells)}
        if dense:
            self.env["EFGP_DENSE_POINTS"] = str(DENSE_POINTS)
        assert R.window(nm, tol, dense) == (self.nf, W), (name, R.window(nm, tol, dense))

    def span_periods(self):
        lo, hi = self.x.min(dim=0).values, self.x.max(dim=0).values
        return tuple(float(v) * self.h for v in (hi - lo))

    def rule(self):
        """(bands, band height) of the restated planner, None when the pass does not take the layout."""
        if self.N < MIN_POINTS or self.W > R.MFMA_MAX_W:
            return None
        return band_rule_held(self.nf, self.N, self.span_periods(), self.band_cells, self.held)

    def trace(self, num_cu):
        rule = self.rule()
        assert (rule is not None) == self.expect_layout, (self.name, rule)
        if rule is None:
            return None
        return layout_trace(self.x, self.h, self.nf, self.W, rule[0], num_cu, self.xcen or (0.0, 0.0), band_cells=rule[1])

    def centred(self):
        """The points relative to the plan centre: what the exact sums are taken over."""
        return self.x if self.xcen is None else self.x - torch.tensor(self.xcen, dtype=torch.float64)[None, :]


def _grid(window, h):
    nm, tol, dense, (nf, W, degree) = WINDOWS[window]
    return nf, W, h * nf


def _from_u(u, W, scale, cen=0.0):
    """x with scale (x - cen) - W/2 = u."""
    return cen + (np.asarray(u, dtype=np.float64) + 0.5 * W) / scale


def _inside_cells(g, lo, hi, n):
    """n values uniform in [lo, hi] that keep MARGIN from every integer and every half-integer (the cell edges of even and odd W)."""
    out = np.empty(0)
    while out.size < n:
        v = lo + (hi - lo) * torch.rand(2 * (n - out.size) + 16, generator=g, dtype=torch.float64).numpy()
        d = np.abs(2.0 * v - np.round(2.0 * v)) / 2.0
        out = np.concatenate([out, v[d >= MARGIN]])
    return out[:n]


def uniform_case(name, window, band_cells, h=0.31, extent=(0.9, 0.9), N=MIN_POINTS, xcen=None, seed=11, **kw):
    """Uniform points over `extent` periods per axis around the plan centre."""
    g = torch.Generator().manual_seed(seed)
    P = 1.0 / h
    x = (torch.rand(N, 2, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([extent[0] * P, extent[1] * P], dtype=torch.float64)
    x[0] = torch.tensor([-0.5 * extent[0] * P, -0.5 * extent[1] * P])
    x[1] = torch.tensor([0.5 * extent[0] * P, 0.5 * extent[1] * P])
    if xcen is not None:
        x = x + torch.tensor(xcen, dtype=torch.float64)[None, :]
    return Case(name, x, h, window, band_cells, xcen=xcen, seed=seed, **kw)


def width_case(window, band_cells):
    """A. one window width and band height: uniform points over 0.9 periods -- over half a period on the dense rule's 216-cell grid,
    where one-cell bands otherwise leave less than the one point per run a forced level asks for."""
    nf = WINDOWS[window][3][0]
    ext = 0.9 if nf <= 64 else 0.5
    return uniform_case(f"widths_{window}_hb{band_cells}", window, band_cells, extent=(ext, ext), seed=11 + nf)


# B. run seams ----------------------------------------------------------------------------------------------------------------------
def seam_points(num_cu, wrap=False):
    """The smallest N whose chunks hold two batches (chunk_length 128: more than 64 * 8 * num_cu points), or with `wrap` the smallest
    at which band_key_kernel's num_cu * 16 workgroups of 256 threads wrap their grid-stride loop (chunks of nine batches); + 300."""
    return (num_cu * 16 * 256 if wrap else num_cu * 8 * 64 + 1) + 300


def run_seam_case(window, band_cells, num_cu, wrap=False, h=0.31, seed=5):
    """Designed runs: every (band, x cell) run has a prescribed count, RUN_COUNTS cycled (each band starts the cycle one further, band 1
    opens with 64, 63: a run start at lane 0 of a second batch and one at lane 63), the last cell of a band takes the rest of the
    band.  Band totals are 1, 2, 3 and 67 past a multiple of the chunk length, so the tails leave 1, 2 and 3 points of a group of
    four, one chunk has a single point and a band ends in a short chunk."""
    nf, W, scale = _grid(window, h)
    N = seam_points(num_cu, wrap)
    L = chunk_length(N, num_cu)
    assert L >= 128 and (not wrap or L == 576)
    g = torch.Generator().manual_seed(seed + W + band_cells)
    ncx = nf - 8                                     # x cells in use: less than a period
    sv = 30.0 if nf == 32 else 44.0                  # y extent in cells: 4 | 8 bands of 7.5 | 5.5 cells, 32 | 64 of less than one
    nb = 1
    while sv / nb > band_cells - 1e-6:
        nb *= 2
    v0 = -0.5 * sv + 0.3
    total = [(N // nb) // L * L + r for r in (1, 2, 3, 67)] + [(N // nb) // L * L + 5] * (nb - 4)
    total[-1] = N - sum(total[:-1])
    assert min(total) > 0
    us, vs, want = [], [], []
    for b in range(nb):
        left, cyc = total[b], list(RUN_COUNTS[b % len(RUN_COUNTS):] + RUN_COUNTS[:b % len(RUN_COUNTS)])
        if b == 1:
            cyc = [64, 63] + cyc
        runs = []
        for m in range(ncx):
            c = cyc[m % len(cyc)]
            if m == ncx - 1 or left - c < 1:
                runs.append(left)
                break
            runs.append(c)
            left -= c
        for m, c in enumerate(runs):
            cell = m - ncx // 2                      # u in (cell - 1, cell)
            us.append(_inside_cells(g, cell - 1 + MARGIN, cell - MARGIN, c))
            vs.append(_inside_cells(g, v0 + b * sv / nb + MARGIN, v0 + (b + 1) * sv / nb - MARGIN, c))
        want += runs
    u, v = np.concatenate(us), np.concatenate(vs)
    v[0], v[-1] = v0, v0 + sv                        # the extent the bands are cut from
    perm = torch.randperm(N, generator=g).numpy()
    x = np.stack([_from_u(u, W, scale), _from_u(v, W, scale)], axis=1)[perm]
    case = Case(f"seams_{window}_hb{band_cells}" + ("_wrap" if wrap else ""), x, h, window, band_cells, seed=seed)
    case.want_runs = want
    return case


def check_run_seams(case, num_cu, wrap=False):
    t = case.trace(num_cu)
    assert t.run_lengths().tolist() == case.want_runs, case.name
    frac = np.abs(t.u0 - np.round(t.u0))
    assert frac.min() >= 0.5 * MARGIN, case.name
    s = t.seams()
    assert t.chunk_len >= 128 and s["group_k"] == [0, 1, 2, 3], (case.name, s)
    assert s["lane0_later_batch"] and s["lane63"] and s["idle_full_batch_behind_first"], (case.name, s)
    assert {1, 2, 3} <= set(s["tails_mod4"]) and s["one_point_chunk"] and s["short_last_chunk"], (case.name, s)
    if wrap:
        assert case.N > num_cu * 16 * 256 and s["batches_per_chunk"] == 9, (case.name, s)
    return t


# C. band geometry ------------------------------------------------------------------------------------------------------------------
def band_edge_case(band_cells, window="w8_box9", nb=2, h=0.31, seed=21):
    """Bands of band_cells - 0.01 cells whose lowest point sits at cell fraction 0.95 (u1 = j + 0.95): its stencil starts at the
    band's first column, off = 0, and the highest point's at off = band_cells, the last LDS row the kernel owns."""
    nf, W, scale = _grid(window, h)
    g = torch.Generator().manual_seed(seed + band_cells)
    N, H = MIN_POINTS, band_cells - 0.01
    v0 = -math.floor(0.5 * nb * H) - 0.05
    b = torch.randint(0, nb, (N,), generator=g).numpy()
    v = v0 + b * H + 1e-6 + (H - 2e-6) * torch.rand(N, generator=g, dtype=torch.float64).numpy()
    for k in range(nb):
        v[2 * k], v[2 * k + 1] = v0 + k * H + 1e-6, v0 + (k + 1) * H - 1e-6
    v[0], v[2 * nb - 1] = v0, v0 + nb * H
    u = _inside_cells(g, -0.4 * nf, 0.4 * nf, N)
    case = Case(f"band_edge_hb{band_cells}", np.stack([_from_u(u, W, scale), _from_u(v, W, scale)], axis=1), h, window, band_cells, seed=seed)
    case.want_bands = nb
    return case


def check_band_edge(case, num_cu):
    t = case.trace(num_cu)
    assert t.nbands == case.want_bands and t.off.min() == 0 and t.off.max() == case.band_cells, (case.name, t.nbands, t.off.min(), t.off.max())
    return t


# bands -> (window, forced height, y extent in cells): 64 is the first count on band_key_kernel's per-point LDS-atomic arm, 256 is
# kMaxBands (its 200 cells are 1.6 periods of the 128-cell grid), 512 would be needed for 300 cells at one cell per band
BAND_COUNTS = {1: ("w8_box9", 8, 6.5), 2: ("w8_box9", 8, 12.5), 64: ("w8", 1, 40.5), 256: ("w8_box45", 1, 200.5), 512: ("w8_box45", 1, 300.5)}


def band_count_case(nb, h=0.31, seed=31):
    window, hb, cells = BAND_COUNTS[nb]
    nf, W, scale = _grid(window, h)
    case = uniform_case(f"bands_{nb}", window, hb, h=h, extent=(0.8, cells / nf), seed=seed + nb, layout=nb <= R.MAX_BANDS)
    case.want_bands = nb if nb <= R.MAX_BANDS else None
    return case


def check_band_count(case, num_cu):
    t = case.trace(num_cu)
    assert (t.nbands if t else None) == case.want_bands, case.name
    return t


def two_grid_cases(h=0.31, seed=41):
    """One point set under two plans whose eight-cell band counts differ by a factor two (the 23 x 23 box on 64 cells, the 45 x 45
    box on 128): -> (coarse alone, fine, coarse when the model already holds the fine plan's level)."""
    coarse = uniform_case("two_grids_coarse_first", "w8", 8, h=h, extent=(0.8, 0.4), seed=seed)
    fine = Case("two_grids_fine", coarse.x, h, "w8_box45", 8, seed=seed)
    adopted = Case("two_grids_coarse_second", coarse.x, h, "w8", 8, seed=seed, held=(fine.rule()[0],))
    return coarse, fine, adopted


def check_two_grids(cases, num_cu):
    coarse, fine, adopted = cases
    assert fine.rule()[0] == 2 * coarse.rule()[0] and adopted.rule() == fine.rule(), (coarse.rule(), fine.rule(), adopted.rule())
    return [c.trace(num_cu) for c in cases]


# D. wraps --------------------------------------------------------------------------------------------------------------------------
def wrap_case(window, band_cells, h=0.31, xcen=None, seed=51):
    """Uniform points over a whole period plus 512 within W/2 cells of each end of it on either axis: their stencils reach across
    the ends of the period and across cell 0 of the grid."""
    nf, W, scale = _grid(window, h)
    g = torch.Generator().manual_seed(seed + W)
    N = MIN_POINTS
    X = (torch.rand(N, 2, generator=g, dtype=torch.float64).numpy() - 0.5) * (nf - 2e-3)
    for a in range(2):
        for k, end in enumerate((-0.5 * nf, 0.5 * nf)):
            rows = slice(512 * (2 * a + k), 512 * (2 * a + k + 1))
            X[rows, a] = end - np.sign(end) * (1e-3 + (0.5 * W - 2e-3) * torch.rand(512, generator=g, dtype=torch.float64).numpy())
    x = X / scale
    if xcen is not None:
        x = x + np.asarray(xcen)[None, :]
    return Case(f"wrap_{window}_hb{band_cells}" + ("_xcen" if xcen is not None else ""), x, h, window, band_cells, xcen=xcen, seed=seed)


def check_wrap(case, num_cu):
    t = case.trace(num_cu)
    nf, W = case.nf[0], case.W
    for u in (t.u0, t.u1):
        first = np.ceil(u).astype(np.int64)
        assert np.any((first < 0) & (first + W - 1 >= 0)), case.name                               # across cell 0: pos_mod wraps
        # the two ends of the period are the same cells of the grid: stencils of points at either end meet there
        ends = [first[u + 0.5 * W < -0.5 * nf + 0.5 * W], first[u + 0.5 * W > 0.5 * nf - 0.5 * W]]
        cells = [set(((f[:, None] + np.arange(W)[None, :]) % nf).reshape(-1).tolist()) for f in ends]
        assert min(len(f) for f in ends) >= 256 and cells[0] & cells[1], case.name
    return t


# E. degenerate point sets ----------------------------------------------------------------------------------------------------------
def line_case(axis, band_cells, window="w8", h=0.31, seed=61):
    """All points on one line: axis 0 -- horizontal, the y span is 0 and the level is one band with band_lo == band_hi; axis 1 --
    vertical, every key of a band ties and each band is a single run in input order."""
    case = uniform_case(f"line_axis{axis}_hb{band_cells}", window, band_cells, h=h, seed=seed + axis)
    x = case.x.clone()
    x[:, 1 - axis] = 0.1234 / h
    return Case(case.name, x, h, window, band_cells, seed=seed)


def check_line(case, num_cu, axis):
    t = case.trace(num_cu)
    if axis == 0:
        assert t.nbands == 1 and t.off.min() == 0 and t.off.max() == 0, case.name
    else:
        assert len(t.run_lengths()) == int((t.band_count > 0).sum()) and not t.run_start.any(), case.name
        for b in range(t.nbands):                                    # ties stay in input order
            o = t.order[t.band == b]
            assert np.all(np.diff(o) > 0), case.name
    return t


def identical_case(window, band_cells, h=0.31, seed=71):
    """All N points identical: one chunk list of a single run; the exact sums are (sum c) * phase, the ones channel N * phase -- the
    worst same-sign pile-up on single cells of the int64 grid."""
    x = np.tile(np.array([[0.1234 / h, -0.3711 / h]]), (MIN_POINTS, 1))
    return Case(f"identical_{window}_hb{band_cells}", x, h, window, band_cells, seed=seed)


def check_identical(case, num_cu):
    t = case.trace(num_cu)
    assert t.nbands == 1 and len(t.run_lengths()) == 1 and not t.run_start.any(), case.name
    return t


def clumps_case(window="w8", h=0.31, seed=81):
    """Two clumps of half a cell at opposite corners of the box under one-cell bands: all bands but the first and the last are empty."""
    nf, W, scale = _grid(window, h)
    g = torch.Generator().manual_seed(seed)
    N = MIN_POINTS
    X = 0.5 * torch.rand(N, 2, generator=g, dtype=torch.float64).numpy()
    X[: N // 2] += -0.4 * nf
    X[N // 2:] += 0.4 * nf - 0.5
    X = X[torch.randperm(N, generator=g).numpy()]
    return Case("clumps_hb1", X / scale, h, window, 1, seed=seed)


def check_clumps(case, num_cu):
    t = case.trace(num_cu)
    assert t.nbands >= 32 and int((t.band_count > 0).sum()) == 2 and t.band_count[0] > 0 and t.band_count[-1] > 0, (case.name, t.nbands)
    return t


def cell_edge_case(window, band_cells, seed=91):
    """Points exactly on fine-cell edges in both axes: h = 0.5 on the 32-cell grid makes scale = 16 a power of two, the lattice
    x = (k + W/2) / 16 makes u = X - W/2 the exact integer k for odd and even W: ceil(u) = u, the s = -1 end of the Horner range.
    The lowest and highest lattice rows are the extent: y == lo is band 0, y == hi clamps to the last band."""
    h = 0.5
    nf, W, scale = _grid(window, h)
    assert nf == 32 and scale == 16.0
    g = torch.Generator().manual_seed(seed + W)
    k = torch.randint(-14, 15, (MIN_POINTS, 2), generator=g).numpy().astype(np.float64)
    k[0], k[1] = (-14, -14), (14, 14)
    x = _from_u(k, W, scale)
    assert np.all(scale * x - 0.5 * W == k)
    return Case(f"cell_edges_{window}_hb{band_cells}", x, h, window, band_cells, seed=seed)


def check_cell_edges(case, num_cu):
    t = case.trace(num_cu)
    assert np.all(t.u0 == np.round(t.u0)) and np.all(t.u1 == np.round(t.u1)), case.name
    y = case.x[:, 1].numpy()
    b = band_index(y, t.nbands)
    assert b[y == y.min()].max() == 0 and b[y == y.max()].min() == t.nbands - 1, case.name
    span = y.max() - y.min()
    assert math.floor(span * (t.nbands / span)) >= t.nbands - 1 and np.count_nonzero(y == y.max()) > 1          # y == hi: the clamp acts
    return t


def alternating_case(band_cells, window="w8_box9", seed=101):
    """Pairs x and nextafter(x) that straddle an x-cell edge (u exactly an integer, and one ulp above it).  x has zero low mantissa
    bits, so the 56-bit keys of a pair tie and the stable sort keeps the input order, which alternates the two: the sorted order
    alternates cells and every point of a batch starts a run."""
    h = 0.5
    nf, W, scale = _grid(window, h)
    assert scale == 16.0
    g = torch.Generator().manual_seed(seed)
    N, sites, levels = MIN_POINTS, 4, 64
    pair = np.arange(N) // 2
    ka = 5.0 + 2.0 * (pair % sites)                               # u of the lower point: 5, 7, 9, 11 (x positive; no cell shared by two sites)
    xa = _from_u(ka, W, scale)
    xb = np.nextafter(xa, np.inf)
    x0 = np.where(np.arange(N) % 2 == 0, xa, xb)
    lev = (pair // sites) % levels
    y = (-0.8 + 1.6 * (lev + 0.37) / levels)                      # 64 levels over 25.6 cells
    return Case(f"alternating_hb{band_cells}", np.stack([x0, y], axis=1), h, window, band_cells, seed=seed)


def check_alternating(case, num_cu):
    t = case.trace(num_cu)
    x = case.x[:, 0].numpy()
    assert np.all((enc_f64(x[0::2]) >> np.uint64(8)) == (enc_f64(x[1::2]) >> np.uint64(8))) and np.all(x[0::2] < x[1::2]), case.name
    inner = t.pos > 0
    assert np.all(t.run_start[inner]) and t.seams()["every_point_starts"], case.name
    return t


# ---- references -------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case, tag, c):
    """The exact sums of strengths c (rows, N) over the case's points, computed once per (case, tag): oracle.efgp_oracle.nudft_type1
    on the points relative to the plan centre."""
    from oracle import efgp_oracle as O
    key = (case.name, case.N, tag)
    if key not in _REF:
        _REF[key] = O.nudft_type1(case.centred(), case.h, c, case.nm)
    return _REF[key]


def reference_fsum(x, h, c, nm):
    """The same sums by the definition, every phase from mpmath at 50 digits and every mode summed with math.fsum."""
    import mpmath
    mpmath.mp.dps = 50
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(c)
    ks = [list(range(-(n // 2), (n - 1) // 2 + 1)) for n in nm]
    out = np.zeros(tuple(nm), dtype=np.complex128)
    tabs = []
    for a in range(2):
        tab = []
        for xv in x[:, a].tolist():
            base = -2 * mpmath.pi * mpmath.mpf(h) * mpmath.mpf(xv)
            tab.append([mpmath.expj(base * k) for k in ks[a]])
        tabs.append(tab)
    for i in range(nm[0]):
        for j in range(nm[1]):
            terms = [mpmath.mpmathify(complex(c[n])) * tabs[0][n][i] * tabs[1][n][j] for n in range(x.shape[0])]
            out[i, j] = complex(math.fsum(float(t.real) for t in terms), math.fsum(float(t.imag) for t in terms))
    return torch.from_numpy(out)
