"""CPU checks of tests/_layout_cases.py, the cases of tests/test_gpu_spread_layout_edges.py: the window of every case against the
library's planner (tools/nufft_plan_check.cpp), the restated chunk length against the library's, every builder's seams at three
CU counts, and the exact-sum reference against mpmath phases summed with math.fsum.  No GPU.
"""
import numpy as np
import pytest
import torch

import _layout_cases as L
import _nufft_routes as R
from test_nufft_plan_host import plan_check  # noqa: F401  (the session fixture that compiles and runs the planner's check program)


def _line(nm, tol, N, dense, band=8, num_cu=R.NUM_CU, span=(0.9, 0.5)):
    return f"t1 2 {nm[0]} {nm[1]} 1 {tol!r} {N} 2 1 0 {int(dense)} {band} {span[0]} {span[1]} 1 {num_cu} {R.LDS_BYTES}\n"


def test_window_table(plan_check):
    """Every window the GPU cases name, held to the planner: fine grid, width, degree, and the layout route at the planner's minimum
    of 32768 points.  The widths 2..8 are all there; the `degree == W + 2` arm is reached by W = 2 and, beyond what the issue of
    this file knew, by W = 3..7 (small boxes on the 32-cell minimum grid, the dense rule's finer grids).  The dense window of the
    fit (W = 7, degree 9) belongs to the 45 x 45 box; the 23 x 23 box keeps W = 8 under the dense rule."""
    names = list(L.WINDOWS)
    got = plan_check([(_line(L.WINDOWS[n][0], L.WINDOWS[n][1], L.MIN_POINTS, L.WINDOWS[n][2]), ()) for n in names])
    for n, g in zip(names, got):
        nm, tol, dense, (nf, W, degree) = L.WINDOWS[n]
        assert (g["nf"], int(g["W"]), int(g["degree"]), int(g["dense"])) == (f"{nf}x{nf}", W, degree, int(dense)), (n, g)
        assert g["spreader"] == "layout" and R.window(nm, tol, dense) == ((nf, nf), W), n
    assert [L.WINDOWS[n][3][1] for n in L.WIDTH_WINDOWS] == [2, 3, 4, 5, 6, 7, 8]
    arms = {n: L.degree_arm(*L.WINDOWS[n][3][1:]) for n in names}
    assert arms["w2"] == "W+2" and all(arms[n] == "W+1" for n in L.WIDTH_WINDOWS[1:])
    assert all(arms[n] == "W+2" for n in L.ARM_WINDOWS) and sorted(L.WINDOWS[n][3][1] for n in L.ARM_WINDOWS) == [3, 4, 5, 6, 7]
    assert "run-time" not in arms.values()


def test_dense_hook_gives_the_dense_window(plan_check):
    """EFGP_DENSE_POINTS, as the GPU cases set it, turns the dense rule on at 32768 points."""
    nm, tol = L.WINDOWS["w7_dense"][:2]
    line = _line(nm, tol, L.MIN_POINTS, False)
    assert int(plan_check([(line, ())])[0]["dense"]) == 0
    g = plan_check([(line, ("EFGP_DENSE_POINTS",))])[0]          # the fixture sets a switch to "1": dense from one point on
    assert (int(g["dense"]), int(g["W"]), int(g["degree"])) == (1, 7, 9) and L.DENSE_POINTS <= L.MIN_POINTS


def test_no_window_reaches_the_run_time_degree_arm(plan_check):
    """launch_w sends degrees other than W + 1 and W + 2 to the run-time Horner loop (DEG = 0).  A scan of 62 tolerances from 0.5 to
    1.2e-8, eleven boxes from 9 x 9 to 45 x 45 (upsampling ratios 2.1 .. 3.6) and both grid rules finds no window of width <= 8
    with such a degree: the arm is not reachable through the planner at these settings, and no GPU case runs it."""
    tols = [0.5 * 10 ** (-k / 8) for k in range(62)]
    boxes = (9, 10, 12, 14, 17, 20, 23, 28, 33, 40, 45)
    keys = [(b, dense, t) for b in boxes for dense in (False, True) for t in tols]
    got = plan_check([(_line((b, b), t, L.MIN_POINTS, dense), ()) for b, dense, t in keys])
    arms = {}
    for key, g in zip(keys, got):
        W, degree = int(g["W"]), int(g["degree"])
        if W <= R.MFMA_MAX_W:
            arms.setdefault((W, L.degree_arm(W, degree)), key)
    assert {w for w, _ in arms} == set(range(2, 9))
    assert not [a for a in arms if a[1] == "run-time"], arms
    assert {w for w, arm in arms if arm == "W+2"} == {2, 3, 4, 5, 6, 7}


def test_width_nine_leaves_the_layout(plan_check):
    nm = (23, 23)
    g = plan_check([(_line(nm, 1e-9, L.MIN_POINTS, False), ())])[0]
    assert int(g["W"]) > R.MFMA_MAX_W and g["spreader"] != "layout" and int(g["level_bands"]) == 0
    assert R.type1_route(nm, 1e-9, L.MIN_POINTS, 2, layout_band=8, span_periods=(0.9, 0.5))[0] != "layout"


def test_chunk_length_restated(plan_check):
    """The Python chunk_length against the library's (csrc/nufft_plan_host.cpp), at the point counts of the cases and around the
    steps of the rule, for the three CU counts."""
    Ns = [L.MIN_POINTS, 80000, 131072, 131073, 3999999, 4000000, 10000000]
    keys = [(N, cu) for cu in L.NUM_CUS for N in Ns + [L.seam_points(cu), L.seam_points(cu, True), cu * 512, cu * 512 + 1, cu * 8 * 1536 + 1]]
    got = plan_check([(_line((9, 9), 1e-7, N, False, num_cu=cu), ()) for N, cu in keys])
    for (N, cu), g in zip(keys, got):
        assert g["spreader"] == "layout" and int(g["chunk_len"]) == L.chunk_length(N, cu), (N, cu, g["chunk_len"])
    assert L.chunk_length(131072, 256) == 64 and L.chunk_length(131073, 256) == 128 and L.chunk_length(L.seam_points(256, True), 256) == 576


def _band_check(plan_check, case, num_cu):
    """The case's restated level against the planner's, for the case's own extent (the planner's check program takes the extent in
    periods from 0; a level the model already holds is not known to it)."""
    span = case.span_periods()
    g = plan_check([(_line(case.nm, case.tol, case.N, case.dense, band=case.band_cells, num_cu=num_cu, span=span), ())])[0]
    rule = L.band_rule_held(case.nf, case.N, span, case.band_cells)
    assert (g["spreader"] == "layout") == (rule is not None), case.name
    if rule:
        assert (int(g["level_bands"]), int(g["band_cells"])) == rule, case.name


@pytest.mark.parametrize("num_cu", L.NUM_CUS)
def test_builders_cross_their_seams(plan_check, num_cu):
    """Every builder's asserted seams under layout_trace (which also asserts 0 <= off <= HB on every point), and its level against
    the planner."""
    cases = []
    for window in ("w8", "w5", "w2"):
        for hb in (8, 1):
            case = L.run_seam_case(window, hb, num_cu)
            L.check_run_seams(case, num_cu)
            cases.append(case)
    case = L.run_seam_case("w8_box9", 8, num_cu, wrap=True)
    t = L.check_run_seams(case, num_cu, wrap=True)
    assert len(t.masks(1)) == 9 and sum(len(o) for o, _ in t.chunks()) == case.N
    cases.append(case)
    for hb in (8, 1):
        cases.append(L.band_edge_case(hb))
        L.check_band_edge(cases[-1], num_cu)
        for axis in (0, 1):
            cases.append(L.line_case(axis, hb))
            L.check_line(cases[-1], num_cu, axis)
        for window in ("w3", "w8_6e8"):
            cases.append(L.identical_case(window, hb))
            L.check_identical(cases[-1], num_cu)
        for window in ("w8_box9", "w5_box9"):
            cases.append(L.cell_edge_case(window, hb))
            L.check_cell_edges(cases[-1], num_cu)
        cases.append(L.alternating_case(hb))
        L.check_alternating(cases[-1], num_cu)
        for window in ("w8", "w2"):
            cases.append(L.wrap_case(window, hb))
            L.check_wrap(cases[-1], num_cu)
    cases.append(L.wrap_case("w8", 8, xcen=(0.3137 / 0.31, -0.7291 / 0.31)))
    L.check_wrap(cases[-1], num_cu)
    for nb in L.BAND_COUNTS:
        cases.append(L.band_count_case(nb))
        L.check_band_count(cases[-1], num_cu)
    cases.append(L.clumps_case())
    L.check_clumps(cases[-1], num_cu)
    three = L.two_grid_cases()
    L.check_two_grids(three, num_cu)
    cases += list(three[:2])
    for window in L.WIDTH_WINDOWS + L.ARM_WINDOWS:
        for hb in (8, 1):
            cases.append(L.width_case(window, hb))
            assert cases[-1].trace(num_cu) is not None
    for window in ("w2", "w8"):
        cases.append(L.uniform_case(f"span_{window}", window, 8, extent=R.SPAN_PERIODS))
        assert cases[-1].trace(num_cu) is not None
    for case in cases:
        _band_check(plan_check, case, num_cu)


def test_trace_on_a_hand_made_set():
    """layout_trace on twelve points whose layout can be read off: two bands, ties in input order, a run start inside a chunk."""
    #            band 0 (y < 0.5)                                band 1
    x = np.array([[0.30, 0.0], [0.10, 0.2], [0.30, 0.1], [0.11, 0.4], [0.10, 0.3],
                  [0.20, 0.5], [0.05, 1.0], [0.20, 0.9], [0.05, 0.7], [0.90, 0.6], [0.05, 0.8], [0.90, 0.55]])
    t = L.layout_trace(x, 1.0, (10, 10), 2, 2, 256)
    assert t.order.tolist() == [1, 4, 3, 0, 2, 6, 8, 10, 5, 7, 9, 11]
    assert t.band.tolist() == [0] * 5 + [1] * 7 and t.chunk_start.tolist() == [0, 5] and t.chunk_count.tolist() == [5, 7]
    assert t.bx.tolist() == [0, 0, 1, 2, 2, 0, 0, 0, 1, 1, 8, 8]          # ceil(10 x - 1)
    assert t.masks(0) == [0b01100] and t.masks(1) == [0b0101000]
    assert t.off.tolist() == [2, 3, 4, 0, 1, 5, 2, 3, 0, 4, 1, 1]         # ceil(10 y - 1) - by0, by0 = -1 and 4
    assert t.run_lengths().tolist() == [2, 1, 2, 3, 2, 2]


@pytest.mark.parametrize("name", ["seams", "alternating"])
def test_reference_against_mpmath(name):
    """oracle.efgp_oracle.nudft_type1, the reference of the GPU file, on 200 points of two cases against phases from mpmath at 50
    digits summed with math.fsum: float64 phases of arguments up to 2 pi 11 h |x| carry a few 1e-16 each, the sum of 200 terms of
    magnitude <= 1.5 stays below 1e-12."""
    from oracle import efgp_oracle as O
    case = L.run_seam_case("w8", 8, 256) if name == "seams" else L.alternating_case(8)
    idx = torch.arange(0, case.N, case.N // 200)[:200]
    x = case.x[idx]
    for cplx in (False, True):
        c = L.strengths(200, 3, cplx=cplx)
        ref = L.reference_fsum(x.numpy(), case.h, c.numpy(), (5, 4))
        got = O.nudft_type1(x, case.h, c, (5, 4))
        assert float((got - ref).abs().max()) < 1e-12
