"""The MFMA spreader over the sorted point layout (csrc/spread_mfma.hip, csrc/points_layout.hip) held to exact sums at every window
width, both band heights, every strength source and every run seam of its batch loop.  The cases, their asserted seams and the
restated host rules are in tests/_layout_cases.py (checked without a GPU by tests/test_layout_cases_host.py); here every builder's
assertions are repeated at the device's own CU count before anything runs.

Every case makes its plan on a `PointSet` and is held to
  (a) the exact sums (oracle.efgp_oracle.nudft_type1): relative l2 error < 2 tol, the project's contract;
  (b) a plan on the same x, h, tol without a layout: max-abs difference < 1e-3 min|c| (the all-ones channel of a pair: < 1e-3).
      The plain route forms the same windowed sums in fixed point on the same grid with the same window and deconvolution, through
      the LDS-atomic spreader; the two differ by rounding only, while a lost, doubled, mis-celled or mis-paired point moves some
      mode by order |c|.  The bound is derived, not measured; 2 tol alone is blind below W = 5, where one lost point of 32768
      moves the result by less than the tolerance.  The plain plan runs with EFGP_NO_RAW48: at these tolerances it would otherwise
      carry 48-bit raw sums, whose rounding (2^-37 max|c| per contribution, 8e-9 max|c| on a mode, measured) is the plain route's
      own floor and exceeds 1e-3 min|c| for generated normals (min|c| = 2e-5 among 65536 of them); its 61-bit sums are the same
      spreader one step finer;
  (c) itself: two calls on the layout route are bit-equal;
  (d) its route: the restated planner says `layout`, and the result is not bit-equal to the plain route's (nufft.hip falls back to
      the plain route silently when a level cannot be made).
Each case prints W, degree, HB, bands, chunk length, the (a) error as a fraction of 2 tol and the (b) difference.

The run-time-degree arm of launch_w (DEG = 0) has no case: tests/test_layout_cases_host.py scans for a window that reaches it and
finds none.  Non-finite coordinates are not a defined input of this kernel and are not run.
"""
import math

import numpy as np
import pytest
import torch

import _layout_cases as L
import _nufft_routes as R

pytestmark = pytest.mark.gpu

MOVED = 1e-3            # (b): a lost point of strength c moves some mode by order |c|; rounding stays many orders below
WORST = {"a": (0.0, ""), "b": (0.0, "")}


def _num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rel(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


def _diff(a, b):
    return float((a - b).abs().max())


def _note(kind, value, name):
    if value > WORST[kind][0]:
        WORST[kind] = (value, name)


class _Run:
    """A case on the device: the plan on a layout with the targets attached, and the plain plan."""

    def __init__(self, case, monkeypatch, points=None):
        from efgp_hip import NufftPlan, PointSet
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("EFGP_NO_RAW48", "1")        # read by the plain route only (plan_lds_or_global): 61-bit sums, see (b) above
        self.case = case
        self.trace = case.trace(_num_cu())
        self.xd = points.x if points is not None else case.x.cuda()
        self.yd = points.values if points is not None else L.strengths(case.N, case.seed).cuda()      # the attached array itself
        self.y = self.yd.cpu()
        self.pts = points if points is not None else PointSet(self.xd, values=self.yd)
        self.plan = NufftPlan(self.xd, case.h, case.tol, xcen=case.xcen, points=self.pts)
        self.plain = NufftPlan(self.xd, case.h, case.tol, xcen=case.xcen)
        t = self.trace
        self.head = (f"{case.name}: N={case.N} W={case.W} degree={case.degree} ({L.degree_arm(case.W, case.degree)}) HB={case.band_cells} "
                     f"bands={t.nbands if t else 0} chunk_len={t.chunk_len if t else 0}")

    def exact(self, what, got, ref):
        err = _rel(got, ref)
        frac = err / (2 * self.case.tol)
        print(f"{self.head} | {what}: (a) {frac:.3f} of 2 tol")
        _note("a", frac, f"{self.case.name} {what}")
        assert err < 2 * self.case.tol, (self.case.name, what, err)

    def against_plain(self, what, got, plain, cmin, same_route=False):
        d = _diff(got, plain)
        print(f"{self.head} | {what}: (b) {d:.2e} (bound {MOVED * cmin:.2e})")
        _note("b", d / cmin, f"{self.case.name} {what}")
        assert d < MOVED * cmin, (self.case.name, what, d)
        if not same_route:
            assert not torch.equal(got, plain), (self.case.name, what, "bit-equal to the plain route: did the layout run?")

    def pair(self):
        """The fit's (y, 1) pair through the attached sorted copy: (a) (b) (c) (d)."""
        case, nm = self.case, self.case.nm
        Fy, v = self.plan.type1_pair(self.yd, nm, nm)
        Fy2, v2 = self.plan.type1_pair(self.yd, nm, nm)
        assert torch.equal(Fy, Fy2) and torch.equal(v, v2), case.name
        ref = L.reference(case, "pair", torch.stack([self.y, torch.ones_like(self.y)]))
        self.exact("pair y", Fy, ref[0])
        self.exact("pair 1", v, ref[1])
        Fy0, v0 = self.plain.type1_pair(self.yd, nm, nm)
        layout = self.trace is not None
        self.against_plain("pair y", Fy, Fy0, 0.5, same_route=not layout)
        self.against_plain("pair 1", v, v0, 1.0, same_route=not layout)
        return Fy, v

    def rows(self):
        """Three real rows through the permutation -- a pair grid and a lone one-channel row: (a) on the first and the lone row,
        (b) (c) on all."""
        case, nm = self.case, self.case.nm
        Z = L.strengths(case.N, case.seed + 1, rows=3)
        Zd = Z.cuda()
        out = self.plan.type1(Zd, nm)
        assert torch.equal(out, self.plan.type1(Zd, nm)), case.name
        ref = L.reference(case, "rows", Z[[0, 2]])
        self.exact("row 0", out[0], ref[0])
        self.exact("lone row", out[2], ref[1])
        self.against_plain("real rows", out, self.plain.type1(Zd, nm), 0.5, same_route=self.trace is None)

    def sources(self):
        """One complex row, generated Rademacher rows and generated normals, plain and scaled (the GEN instantiation): (b) against
        the plain plan given the materialised rows, (c)."""
        from efgp_hip import normal_fill, rademacher_fill
        case, nm, dev = self.case, self.case.nm, self.xd.device
        c = L.strengths(case.N, case.seed + 2, cplx=True).cuda()
        out = self.plan.type1(c, nm)
        assert torch.equal(out, self.plan.type1(c, nm)), case.name
        self.against_plain("complex row", out, self.plain.type1(c, nm), 0.5)
        seed, off = 4242 + case.seed, 7
        FR = self.plan.type1_rademacher(seed, 3, nm, index_offset=off)
        assert torch.equal(FR, self.plan.type1_rademacher(seed, 3, nm, index_offset=off)), case.name
        self.against_plain("rademacher", FR, self.plain.type1(rademacher_fill(dev, seed, 3, case.N, index_offset=off), nm), 1.0)
        Zn = normal_fill(dev, seed, 2, case.N, index_offset=off)
        FN = self.plan.type1_normal(seed, 2, nm, index_offset=off)
        assert torch.equal(FN, self.plan.type1_normal(seed, 2, nm, index_offset=off)), case.name
        self.against_plain("normal", FN, self.plain.type1(Zn, nm), float(Zn.abs().min()))
        sc = (0.5 + torch.rand(case.N, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)).cuda()
        FS = self.plan.type1_normal_scaled(seed, 2, nm, sc, index_offset=off)
        assert torch.equal(FS, self.plan.type1_normal_scaled(seed, 2, nm, sc, index_offset=off)), case.name
        Zs = (Zn * sc[None, :]).contiguous()
        self.against_plain("scaled normal", FS, self.plain.type1(Zs, nm), float(Zs.abs().min()))


# ---- A. every width, band height and strength source ----------------------------------------------------------------------------
@pytest.mark.parametrize("band_cells", [8, 1])
@pytest.mark.parametrize("window", L.WIDTH_WINDOWS + L.ARM_WINDOWS)
def test_every_width_and_source(window, band_cells, monkeypatch):
    """W = 2..8 (degree W + 1; W = 2: W + 2) and the W + 2 arm at W = 3..7, the dense-point window of the fit among them, at both
    band heights: the pair and real rows against the exact sums, every other strength source against the plain route."""
    run = _Run(L.width_case(window, band_cells), monkeypatch)
    assert run.trace.nbands >= 4 and run.case.W == L.WINDOWS[window][3][1]
    run.pair()
    run.rows()
    run.sources()


# ---- B. run seams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band_cells", [8, 1])
@pytest.mark.parametrize("window", ["w8", "w5", "w2"])
def test_run_seams(window, band_cells, monkeypatch):
    """Designed runs in chunks of two batches: a run start at each position of a group of four, at lane 0 of a second batch and at
    lane 63, a whole batch without one behind a first batch, tails of 1, 2 and 3 points, a chunk of one point, a band that ends in
    a short chunk (asserted on the trace for this device's CU count)."""
    case = L.run_seam_case(window, band_cells, _num_cu())
    L.check_run_seams(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


def test_run_seams_where_the_key_pass_wraps(monkeypatch):
    """num_cu * 4096 + 300 points: band_key_kernel's num_cu * 16 workgroups no longer cover N and wrap their grid-stride loop;
    chunks run nine batches."""
    case = L.run_seam_case("w8_box9", 8, _num_cu(), wrap=True)
    L.check_run_seams(case, _num_cu(), wrap=True)
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


# ---- C. band geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band_cells", [8, 1])
def test_stencils_at_the_last_row_of_a_band(band_cells, monkeypatch):
    case = L.band_edge_case(band_cells)
    L.check_band_edge(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


@pytest.mark.parametrize("nbands", [1, 2, 64, 256])
def test_band_counts(nbands, monkeypatch):
    """One band, two, 64 (the first count on band_key_kernel's per-point LDS-atomic arm) and kMaxBands."""
    case = L.band_count_case(nbands)
    L.check_band_count(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


def test_more_bands_than_a_level_holds_falls_back(monkeypatch):
    """300 cells of axis 1 at one cell per band would need 512 bands: the planner gives no level, the pass takes the plain route and
    still computes the sums."""
    case = L.band_count_case(512)
    assert L.check_band_count(case, _num_cu()) is None
    run = _Run(case, monkeypatch)
    run.pair()


@pytest.mark.parametrize("fine_first", [True, False])
def test_two_grids_on_one_point_set(fine_first, monkeypatch):
    """Two plans on one PointSet whose band counts differ by a factor two.  Fine grid first: the coarse plan then adopts the fine
    plan's level (plan_level's have_level branch) instead of sorting again; coarse grid first: each makes its own."""
    from efgp_hip import PointSet
    coarse, fine, adopted = cases = L.two_grid_cases()
    L.check_two_grids(cases, _num_cu())
    xd = coarse.x.cuda()
    pts = PointSet(xd, values=L.strengths(coarse.N, coarse.seed).cuda())
    order = [fine, adopted] if fine_first else [coarse, fine]
    for case in order:
        run = _Run(case, monkeypatch, points=pts)
        run.pair()
        run.rows()


# ---- D. wraps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band_cells", [8, 1])
@pytest.mark.parametrize("window", ["w8", "w2"])
def test_stencils_across_the_period(window, band_cells, monkeypatch):
    case = L.wrap_case(window, band_cells)
    L.check_wrap(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


def test_plan_centre(monkeypatch):
    """A plan centre that is no multiple of a cell: bx, by0 and off are taken relative to it."""
    case = L.wrap_case("w8", 8, xcen=(0.3137 / 0.31, -0.7291 / 0.31))
    L.check_wrap(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


@pytest.mark.parametrize("window", ["w2", "w8"])
def test_points_over_more_than_a_period(window, monkeypatch):
    case = L.uniform_case(f"span_{window}", window, 8, extent=R.SPAN_PERIODS)
    run = _Run(case, monkeypatch)
    assert run.trace is not None and (case.x[:, 0].max() - case.x[:, 0].min()) * case.h > 1.19
    run.pair()
    run.rows()


# ---- E. degenerate point sets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band_cells", [8, 1])
@pytest.mark.parametrize("axis", [0, 1])
def test_points_on_one_line(axis, band_cells, monkeypatch):
    """Horizontal: the y span is 0, one band with band_lo == band_hi.  Vertical: every key of a band ties, each band is one run."""
    case = L.line_case(axis, band_cells)
    L.check_line(case, _num_cu(), axis)
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


@pytest.mark.parametrize("band_cells", [8, 1])
@pytest.mark.parametrize("window", ["w3", "w8_6e8"])
def test_identical_points(window, band_cells, monkeypatch):
    """All N points identical, tol 1e-2 and 6e-8.  The exact sums are (sum c) * phase (math.fsum of the strengths times the sums of
    one unit point); the ones channel N * phase is the worst same-sign pile-up on single cells of the int64 grid."""
    from oracle import efgp_oracle as O
    case = L.identical_case(window, band_cells)
    L.check_identical(case, _num_cu())
    run = _Run(case, monkeypatch)
    Fy, v = run.pair()
    phase = O.nudft_type1(case.x[:1], case.h, torch.ones(1, dtype=torch.float64), case.nm)
    run.exact("closed form y", Fy, math.fsum(run.y.tolist()) * phase)
    run.exact("closed form 1", v, case.N * phase)
    run.rows()


def test_two_clumps_under_one_cell_bands(monkeypatch):
    case = L.clumps_case()
    L.check_clumps(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


@pytest.mark.parametrize("band_cells", [8, 1])
@pytest.mark.parametrize("window", ["w8_box9", "w5_box9"])
def test_points_on_cell_edges(window, band_cells, monkeypatch):
    """Every point exactly on a fine-cell edge in both axes, for an even and an odd W: the s = -1 end of the Horner range; points
    exactly at lo and at hi, where the band index clamps."""
    case = L.cell_edge_case(window, band_cells)
    L.check_cell_edges(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


@pytest.mark.parametrize("band_cells", [8, 1])
def test_every_point_starts_a_run(band_cells, monkeypatch):
    """Pairs x, nextafter(x) across an x-cell edge with tied keys in alternating input order: the sorted order alternates cells, a
    tile is flushed before every point."""
    case = L.alternating_case(band_cells)
    L.check_alternating(case, _num_cu())
    run = _Run(case, monkeypatch)
    run.pair()
    run.rows()


def test_zz_worst_figures():
    """Last in the file: the worst (a) fraction and the worst (b) difference (in units of the smallest strength) of this run."""
    print(f"worst (a): {WORST['a'][0]:.3f} of 2 tol at {WORST['a'][1]}")
    print(f"worst (b): {WORST['b'][0]:.2e} x min|c| at {WORST['b'][1]}")
    assert np.isfinite(WORST["a"][0]) and np.isfinite(WORST["b"][0])
