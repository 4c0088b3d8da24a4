"""GPU: every route of the non-uniform transforms against the exact sums, across sign, mode order, mode scale, plan centre,
batch and non-cubic mode boxes.

The routes (csrc/nufft.hip) -- type 1: padded LDS slabs with 48-bit raw or 61-bit sums, unpadded LDS slabs, global atomics, LDS
tiles, cell-sorted registers, the MFMA layout; behind them the two-launch grid-to-modes DFT, the pruned FFT (fused with the int64
accumulator or not) and the full FFT.  Type 2: the dense-DFT grid kernel or precorrect_kernel with the pruned / full FFT; the pair,
halo, plain-LDS, L2 and tiled gathers.  Which case takes which route is asserted on the host from the library's own window rules
(tests/test_nudft_reference_host.py::test_geometry_of_the_cases, the restated dispatch in tests/_nufft_routes.py).  Every box is
non-cubic with even and odd axes, so an axis mixed up in a scale, a tile size or a correction table shows.

Reference: tests/_nudft.py (float64 on the CPU, phases from the definition).  Measure and bar are those of tests/test_gpu_nufft.py:
relative l2 error below 2 x tolerance + 1e-13; real-only outputs are judged on the scale of the complex sums they are the real
part of (tools/fuzz_nufft.py).  Points (tests/_nufft_routes.py::points): both ends of a period of every axis and within half a
fine cell of them, a quarter of the points inside one fine cell with duplicates, the rest uniform over more than one period.
Switches are set with monkeypatch and every test makes its own plans: plans cache their binning and class order.
"""
import itertools

import pytest
import torch

import _nudft as E
import _nufft_routes as R

pytestmark = pytest.mark.gpu

SIGN_ORDER = list(itertools.product([-1, +1], [0, 1]))
SIGN_ORDER_SCALE = list(itertools.product([+1, -1], [0, 1], [False, True]))
DEFAULT_AND_FLIPPED_1 = [(-1, 0), (+1, 1)]
DEFAULT_AND_FLIPPED_2 = [(+1, 0), (-1, 1)]


def _bar(tol):
    return 2 * tol + 1e-13


def _rel(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


def _rel_real(out, ref):
    """A real-only output against the complex sums it is the real part of, on their scale."""
    out, ref = out.detach().cpu(), ref.detach().cpu()
    assert out.shape == ref.shape and not out.is_complex()
    return float(torch.linalg.norm((out - ref.real).reshape(-1)) / torch.linalg.norm(ref.reshape(-1)))


def _xcen(d, h):
    """A centre that is no multiple of a fine cell on any axis."""
    return tuple(v / h for v in (0.3137, -0.7291, 0.1733)[:d])


def _strengths(N, cplx, B=None, seed=7):
    g = torch.Generator().manual_seed(seed + N)
    shape = (N,) if B is None else (B, N)
    c = torch.randn(shape, generator=g, dtype=torch.float64)
    return torch.complex(c, torch.randn(shape, generator=g, dtype=torch.float64)) if cplx else c


def _modes(nm, B=None, seed=6):
    g = torch.Generator().manual_seed(seed + 100 * nm[0] + nm[-1])
    shape = tuple(nm) if B is None else (B,) + tuple(nm)
    return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))


def _plan(x, h, tol, xcen=None, layout=False, values=None):
    from efgp_hip import NufftPlan, PointSet
    xd = x.cuda()
    pts = PointSet(xd, values=None if values is None else values.cuda()) if layout else None
    return NufftPlan(xd, h, tol, xcen=xcen, points=pts)


_REF1 = {}


def _ref1(key, x, h, c, nm, isign, modeord, xcen=None):
    """The exact type-1 sums of a case, computed once per (case, sign, order)."""
    key = (key, isign, modeord)
    if key not in _REF1:
        _REF1[key] = E.type1(x, h, c, nm, isign=isign, modeord=modeord, xcen=xcen)
    return _REF1[key]


def _setup1(name, monkeypatch):
    nm, tol, N, cplx, h, _, kw = R.TYPE1[name]
    for v in kw.get("env", ()):
        monkeypatch.setenv(v, "1")
    if kw.get("layout_band"):
        monkeypatch.setenv("EFGP_MFMA_BAND_CELLS", str(kw["layout_band"]))
    x = R.points(len(nm), N, h)[0]
    c = _strengths(N, cplx)
    return nm, tol, N, h, x, c, bool(kw.get("layout_band"))


# ---- type 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("isign,modeord", SIGN_ORDER)
@pytest.mark.parametrize("name", list(R.TYPE1))
def test_type1_route_sign_order(name, isign, modeord, monkeypatch):
    nm, tol, N, h, x, c, layout = _setup1(name, monkeypatch)
    plan = _plan(x, h, tol, layout=layout, values=None if c.is_complex() else c)
    out = plan.type1(c.cuda(), nm, modeord=modeord, isign=isign)
    err = _rel(out, _ref1(name, x, h, c, nm, isign, modeord))
    print(f"\n{name} isign={isign} modeord={modeord}: {err:.2e} (bar {_bar(tol):.1e})")
    assert err < _bar(tol)


@pytest.mark.parametrize("name,env", [("layout_g2m_band8", "EFGP_NO_MFMA_SPREAD"), ("layout_g2m_band1", "EFGP_NO_MFMA_SPREAD"),
                                      ("layout_pruned_band8", "EFGP_NO_MFMA_SPREAD"), ("layout_pruned_band1", "EFGP_NO_MFMA_SPREAD"),
                                      ("cells", "EFGP_CELLSORT")])
def test_layout_and_cell_sorted_routes_are_the_ones_that_run(name, env, monkeypatch):
    """As test_gpu_spread_mfma.py::test_layout_path_is_the_one_that_runs: with the route switched off the same call gives other last
    bits -- another spreader ran.  The spreaders it falls back to and the layout sum exact integers, so two plans on either agree
    bit for bit; the cell-sorted route adds doubles with atomics in arrival order and only has to differ from them."""
    nm, tol, N, h, x, c, layout = _setup1(name, monkeypatch)
    a = _plan(x, h, tol, layout=layout, values=c).type1(c.cuda(), nm)
    if layout:
        assert torch.equal(a, _plan(x, h, tol, layout=layout, values=c).type1(c.cuda(), nm))
    if env == "EFGP_CELLSORT":
        monkeypatch.delenv(env)
    else:
        monkeypatch.setenv(env, "1")
    off = _plan(x, h, tol, layout=layout, values=c).type1(c.cuda(), nm)
    assert torch.equal(off, _plan(x, h, tol, layout=layout, values=c).type1(c.cuda(), nm))
    assert not torch.equal(a, off)
    assert _rel(a, off) < 4 * tol


FAMILY = {      # one route of each family: box, N, h, layout band height
    "lds": ((23, 45), 3000, 0.5, 0),
    "tiles": ((45, 70), 32768, 0.37, 0),
    "layout": ((23, 45), 32768, 0.5, 8),
}


def _family(name, monkeypatch, xcen=False):
    nm, N, h, band = FAMILY[name]
    if band:
        monkeypatch.setenv("EFGP_MFMA_BAND_CELLS", str(band))
    xc = _xcen(len(nm), h) if xcen else None
    return nm, 1e-7, N, h, R.points(len(nm), N, h, xc)[0], xc, bool(band)


@pytest.mark.parametrize("modeord", [0, 1])
@pytest.mark.parametrize("family", list(FAMILY))
def test_type1_three_real_rows(family, modeord, monkeypatch):
    """Three real rows: a pair grid (two rows in the real and imaginary channel, split by Hermitian symmetry, part = 3) and a lone row."""
    nm, tol, N, h, x, _, layout = _family(family, monkeypatch)
    Z = _strengths(N, False, B=3, seed=11)
    out = _plan(x, h, tol, layout=layout).type1(Z.cuda(), nm, modeord=modeord)
    ref = _ref1(("rows3", family), x, h, Z, nm, -1, modeord)
    assert out.shape == ref.shape
    for b in range(3):
        assert _rel(out[b], ref[b]) < _bar(tol), b


@pytest.mark.parametrize("family,N,band", [("global", 3000, 0), ("tiles", 32768, 0), ("layout", 32768, 8)])
@pytest.mark.parametrize("boxes", [((17, 29), (33, 57)), ((33, 57), (17, 29))])
def test_type1_pair_two_boxes(family, N, band, boxes, monkeypatch):
    """The fit's pair (F* y on one box, F* 1 on another) on two non-cubic boxes of different aspect, either one the larger.  The
    two-channel 96 x 128 grid of the larger box is beyond the LDS: global atomics, tiles or the layout."""
    tol, h = 1e-7, 0.37
    assert R.type1_route((33, 57), tol, N, 2, layout_band=band, span_periods=R.SPAN_PERIODS)[0] == family
    if band:
        monkeypatch.setenv("EFGP_MFMA_BAND_CELLS", str(band))
    x = R.points(2, N, h)[0]
    y = _strengths(N, False, seed=13)
    plan = _plan(x, h, tol, layout=bool(band), values=y)
    Fy, v = plan.type1_pair(y.cuda(), boxes[0], boxes[1])
    assert _rel(Fy, _ref1(("pair_y", N, boxes[0]), x, h, y, boxes[0], -1, 0)) < _bar(tol)
    assert _rel(v, _ref1(("pair_1", N, boxes[1]), x, h, torch.ones(N, dtype=torch.float64), boxes[1], -1, 0)) < _bar(tol)


@pytest.mark.parametrize("family", list(FAMILY))
def test_type1_generated_rows_in_fft_order(family, monkeypatch):
    """Rows generated in the spread kernels (three: a pair grid and an odd row) at modeord = 1, against the exact sums of the
    materialised rows."""
    from efgp_hip import normal_fill, rademacher_fill
    nm, tol, N, h, x, _, layout = _family(family, monkeypatch)
    plan = _plan(x, h, tol, layout=layout)
    dev = plan.dev
    seed, off = 20240607, 1000
    Zr = rademacher_fill(dev, seed, 3, N, index_offset=off).cpu()
    Zn = normal_fill(dev, seed, 3, N, index_offset=off).cpu()
    assert set(Zr.unique().tolist()) == {-1.0, 1.0}
    assert _rel(plan.type1_rademacher(seed, 3, nm, index_offset=off, modeord=1), E.type1(x, h, Zr, nm, modeord=1)) < _bar(tol)
    assert _rel(plan.type1_normal(seed, 3, nm, index_offset=off, modeord=1), E.type1(x, h, Zn, nm, modeord=1)) < _bar(tol)


@pytest.mark.parametrize("isign,modeord", DEFAULT_AND_FLIPPED_1)
@pytest.mark.parametrize("family", list(FAMILY))
def test_type1_plan_centre(family, isign, modeord, monkeypatch):
    """A plan centre that is no multiple of a cell, points given relative to it: the spreaders, the tile binning and the layout's
    band geometry each read it."""
    nm, tol, N, h, x, xc, layout = _family(family, monkeypatch, xcen=True)
    c = _strengths(N, True, seed=17)
    out = _plan(x, h, tol, xcen=xc, layout=layout).type1(c.cuda(), nm, modeord=modeord, isign=isign)
    assert _rel(out, _ref1(("xcen", family), x, h, c, nm, isign, modeord, xcen=xc)) < _bar(tol)


def test_type1_tiles_second_pass_runs_the_class_order():
    """65536 points on the tiled 2-D route, twice on one plan: the second pass re-sorts the binned points (tile_class_order_kernel,
    from 16 windows of 4096 points on); the gather then reads the same binning."""
    nm, tol, N, h = (45, 70), 1e-7, 65536, 0.37
    assert R.type1_route(nm, tol, N, 1) == ("tiles", "pruned_from_acc") and R.type2_route(nm, tol, N, 1, True)[1] == "tiles"
    x, n_edge, cluster = R.points(2, N, h)
    c = _strengths(N, False)
    plan = _plan(x, h, tol)
    ref = E.type1(x, h, c, nm)
    first = plan.type1(c.cuda(), nm)
    second = plan.type1(c.cuda(), nm)
    assert _rel(first, ref) < _bar(tol) and _rel(second, ref) < _bar(tol)
    f = _modes(nm)
    sub = R.compared_points(N, n_edge, cluster)
    out = plan.type2(f.cuda(), nm, real_only=True)
    assert _rel_real(out[sub.cuda()], E.type2(x[sub], h, f, nm)) < _bar(tol)


# ---- type 2 ---------------------------------------------------------------------------------------------------------------------
def _check2(x, sub, h, tol, nm, B, real_only, isign, modeord, scaled, xcen=None, plan=None, tag=""):
    f = _modes(nm, B)
    scale = _modes(nm, seed=9) if scaled else None
    plan = plan or _plan(x, h, tol, xcen=xcen)
    out = plan.type2(f.cuda(), nm, modeord=modeord, real_only=real_only, isign=isign,
                     mode_scale=None if scale is None else scale.cuda())
    assert out.shape == ((x.shape[0],) if B is None else (B, x.shape[0]))
    ref = E.type2(x[sub], h, f, nm, isign=isign, modeord=modeord, xcen=xcen, mode_scale=scale)
    got = out[..., sub.cuda()]
    rows = [(got, ref)] if B is None else [(got[b], ref[b]) for b in range(B)]
    for o, r in rows:
        err = _rel_real(o, r) if real_only else _rel(o, r)
        print(f"\n{tag} isign={isign} modeord={modeord} scaled={scaled}: {err:.2e} (bar {_bar(tol):.1e})")
        assert err < _bar(tol)


@pytest.mark.parametrize("isign,modeord,scaled", SIGN_ORDER_SCALE)
@pytest.mark.parametrize("name", list(R.TYPE2))
def test_type2_route_sign_order_scale(name, isign, modeord, scaled):
    nm, tol, N, B, real_only, h, _ = R.TYPE2[name]
    x, n_edge, cluster = R.points(len(nm), N, h)
    _check2(x, R.compared_points(N, n_edge, cluster), h, tol, nm, B, real_only, isign, modeord, scaled, tag=name)


@pytest.mark.parametrize("isign,modeord", DEFAULT_AND_FLIPPED_2)
@pytest.mark.parametrize("name,B", [("real_tiles_2d", None), ("real_pair_fill", 2), ("cplx_tiles_2d", 3)])
def test_type2_plan_centre_and_batch(name, B, isign, modeord):
    """A plan centre on the tiled and the pair route (real outputs), and a batch of three on the tiled route with the centre too."""
    nm, tol, N, _, real_only, h, _ = R.TYPE2[name]
    xc = _xcen(len(nm), h)
    x, n_edge, cluster = R.points(len(nm), N, h, xc)
    _check2(x, R.compared_points(N, n_edge, cluster), h, tol, nm, B, real_only, isign, modeord, True, xcen=xc, tag=name)


def test_type2_batch_of_three_on_the_tiled_route():
    nm, tol, N, _, real_only, h, _ = R.TYPE2["cplx_tiles_2d"]
    x, n_edge, cluster = R.points(len(nm), N, h)
    _check2(x, R.compared_points(N, n_edge, cluster), h, tol, nm, 3, real_only, +1, 0, False, tag="batch 3")


# ---- the dense rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("isign,modeord", DEFAULT_AND_FLIPPED_1)
@pytest.mark.parametrize("nm,N,cplx,band", [((23, 23), 3000, True, 0), ((45, 45), 3000, False, 0), ((45, 45), 32768, False, 8)])
def test_dense_rule_type1(nm, N, cplx, band, isign, modeord, monkeypatch):
    """EFGP_DENSE_POINTS=1 gives a small plan the dense rule's off-ladder grids (90 and 180 cells): padded LDS slabs on 90 x 90,
    global atomics on 180 x 180, and the layout with grid-to-modes on the 180-cell grid."""
    monkeypatch.setenv("EFGP_DENSE_POINTS", "1")
    if band:
        monkeypatch.setenv("EFGP_MFMA_BAND_CELLS", str(band))
    tol, h = 1e-7, 0.5
    x = R.points(2, N, h)[0]
    c = _strengths(N, cplx, seed=19)
    out = _plan(x, h, tol, layout=bool(band)).type1(c.cuda(), nm, modeord=modeord, isign=isign)
    assert _rel(out, _ref1(("dense", nm, N), x, h, c, nm, isign, modeord)) < _bar(tol)


@pytest.mark.parametrize("isign,modeord", DEFAULT_AND_FLIPPED_2)
@pytest.mark.parametrize("nm", [(23, 23), (45, 45)])
@pytest.mark.parametrize("B,real_only", [(None, False), (2, True)])
def test_dense_rule_type2(nm, B, real_only, isign, modeord, monkeypatch):
    monkeypatch.setenv("EFGP_DENSE_POINTS", "1")
    tol, h, N = 1e-7, 0.5, 3000
    x = R.points(2, N, h)[0]
    _check2(x, torch.arange(N), h, tol, nm, B, real_only, isign, modeord, True, tag=f"dense {nm}")


# ---- the fall-back branches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["EFGP_NO_PRUNED_FFT", "EFGP_NO_FFT_FROM_ACC"])
@pytest.mark.parametrize("nm,tol,N,h", [((45, 70), 1e-7, 32768, 0.37), ((21, 12, 9), 1e-6, 32768, 0.5), ((10, 13, 16), 1e-5, 3000, 0.37)])
def test_full_fft_and_unfused_branches(nm, tol, N, h, env, monkeypatch):
    """Without the pruned transform both types run the full FFT (and the deconvolve kernel on the uncropped grid); without the
    fusion the tiled spreader's accumulator is converted by reduce_slabs_kernel before the pruned transform.  Sign and order
    flipped from the defaults."""
    monkeypatch.setenv(env, "1")
    x, n_edge, cluster = R.points(len(nm), N, h)
    c = _strengths(N, True, seed=23)
    plan = _plan(x, h, tol)
    out = plan.type1(c.cuda(), nm, modeord=1, isign=+1)
    assert _rel(out, _ref1(("fallback", nm), x, h, c, nm, +1, 1)) < _bar(tol)
    sub = R.compared_points(N, n_edge, cluster)
    _check2(x, sub, h, tol, nm, None, True, -1, 1, True, plan=plan, tag=env)
    _check2(x, sub, h, tol, nm, None, False, -1, 1, True, plan=plan, tag=env)


def test_unpadded_lds_spreader_by_switch(monkeypatch):
    monkeypatch.setenv("EFGP_NO_PAD", "1")
    nm, tol, N, h = (23, 45), 1e-7, 3000, 0.5
    x = R.points(2, N, h)[0]
    c = _strengths(N, True)
    out = _plan(x, h, tol).type1(c.cuda(), nm, modeord=1, isign=+1)
    assert _rel(out, _ref1("lds_pad_raw48_cplx", x, h, c, nm, +1, 1)) < _bar(tol)


@pytest.mark.parametrize("env,nm,h", [("EFGP_NO_HALO", (33, 40), 0.37), ("EFGP_NO_PAIR_GATHER", (23, 45), 0.5),
                                      ("EFGP_NO_DIRECT_DFT", (33, 40), 0.37), ("EFGP_NO_DIRECT_DFT", (23, 45), 0.5)])
def test_gather_switches(env, nm, h, monkeypatch):
    """One real row: the plain real LDS gather instead of the halo one, the halo gather instead of the pair one, and
    precorrect + FFT instead of the dense-DFT grid kernel (for the halo and for the pair gather's own fill)."""
    monkeypatch.setenv(env, "1")
    tol, N = 1e-7, 3000
    x = R.points(2, N, h)[0]
    _check2(x, torch.arange(N), h, tol, nm, None, True, -1, 1, True, tag=env)
