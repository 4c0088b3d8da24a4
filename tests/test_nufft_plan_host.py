"""CPU check of the host planner of the NUFFT passes (csrc/nufft_plan_host.cpp) through the stand-alone program
tools/nufft_plan_check.cpp: the window, the tile geometry, the layout level and the route of every named case of
tests/test_gpu_nufft_options.py, field by field against their restatement in tests/_nufft_routes.py and against the route tuples
recorded in its case tables.  The drivers of csrc/nufft.hip execute what this planner returns, so a threshold that moves in the
library moves a field here.

The program is compiled once per session without the sanitizer flags (the sanitized build is the tool's documented command line,
run by hand); the compiler is found as efgp_hip/build.py finds it -- without it the library cannot be built either.  The LDS size
and the CU count the restatement assumes are handed to the program with every case.
"""
import os
import subprocess

import pytest

import _nufft_routes as R
from test_gpu_nufft_options import FAMILY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp-quadrature_amd", "csrc")
# the switches block of tests/test_nudft_reference_host.py::test_geometry_of_the_cases, then the other route hooks
HOOK_SETS = [(), ("EFGP_NO_PRUNED_FFT",), ("EFGP_NO_FFT_FROM_ACC",), ("EFGP_NO_PAD",), ("EFGP_NO_HALO",), ("EFGP_NO_PAIR_GATHER",),
             ("EFGP_NO_DIRECT_DFT",), ("EFGP_NO_GRID_TO_MODES",), ("EFGP_NO_TILES",), ("EFGP_NO_RAW48",), ("EFGP_NO_GATHER_IMAGE",),
             ("EFGP_NO_MFMA_SPREAD",), ("EFGP_CELLSORT",)]
FAMILY_TOL = 1e-7            # test_gpu_nufft_options.py::_family
# Routes no case of R.TYPE1 / R.TYPE2 / FAMILY takes without a hook, planned here only (no GPU test runs them under these names).
# The image: one real row on the (23, 45) box, the tuple test_geometry_of_the_cases records for it.  The full FFT: an axis of 2100
# modes has a fine grid beyond the 4096 cells of the in-house transform's line (every smaller grid is pruned: nf >= 2 nm); its
# 1-D grid, one channel or complex, is far inside the LDS and 1000 points per workgroup keep the 48-bit raw sums at 1e-7.
EXTRA1 = {"fft_beyond_own_fft": ((2100,), 1e-7, 3000, False, 0.5, ("lds_pad_raw48", "fft"), {})}
EXTRA2 = {"real_image": ((23, 45), 1e-7, 3000, None, True, 0.5, ("image", "pair")),
          "fft_beyond_own_fft": ((2100,), 1e-7, 3000, None, False, 0.5, ("fft", "lds"))}


def _pad3(v, fill=1):
    return " ".join(str(x) for x in tuple(v) + (fill,) * (3 - len(v)))


def _line(kind, nm, tol, N, chan, batch=1, normal=False, dense=False, layout=0):
    return (f"{kind} {len(nm)} {_pad3(nm)} {tol!r} {N} {int(chan)} {batch} {int(normal)} {int(dense)} {layout} "
            f"{_pad3(R.SPAN_PERIODS[:1] + R.SPAN_PERIODS[1:] * 2)} {R.NUM_CU} {R.LDS_BYTES}\n")


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nufft_plan_check") / "nufft_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I/opt/rocm/include", os.path.join(ROOT, "tools", "nufft_plan_check.cpp"),
           os.path.join(CSRC, "nufft_plan_host.cpp"), os.path.join(CSRC, "es_kernel.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)

    def run(lines, hooks=()):
        """lines: (case line, the case's own switches) -> one dict of the printed fields per case.  One process per set of switches."""
        out = [None] * len(lines)
        for own in sorted({tuple(own) for _, own in lines}):
            env = {k: v for k, v in os.environ.items() if not k.startswith("EFGP_")}
            env.update({h: "1" for h in tuple(hooks) + own})
            idx = [i for i, (_, o) in enumerate(lines) if tuple(o) == own]
            res = subprocess.run([exe], input="".join(lines[i][0] for i in idx), env=env, check=True, capture_output=True, text=True)
            got = res.stdout.splitlines()
            assert len(got) == len(idx), res.stderr
            for i, g in zip(idx, got):
                out[i] = dict(field.split("=", 1) for field in g.split())
        return out

    return run


def _axes(text):
    return tuple(int(f) for f in text.split("x"))


AFTER = {"g2m_from_acc": "g2m", "g2m": "g2m", "pruned_from_acc": "pruned_from_acc", "pruned": "pruned", "fft": "fft"}


def _span(d):
    return (R.SPAN_PERIODS[:1] + R.SPAN_PERIODS[1:] * 2)[:d]


def _check1(tag, g, nm, tol, N, chan, want, env, layout=0, normal=False, dense=False):
    """One planned type-1 pass against the route `want` and the restated window, tile geometry, level, slabs and class order."""
    nf, W = R.window(nm, tol, dense)
    assert (_axes(g["nf"]), int(g["W"])) == (nf, W), tag
    got = (g["spreader"], AFTER[g["after"]])
    assert got == want, (tag, got)
    assert (g["after"] == "g2m_from_acc") == (want == ("layout", "g2m")), tag           # only the layout hands its accumulator over
    if want[0] in ("tiles", "cells"):
        assert (_axes(g["tile_nt"]), _axes(g["tile_T"])) == R.tile_geom(nf, W, chan, 1 if want[0] == "cells" else 0), tag
    if want[0] == "layout":
        assert (int(g["level_bands"]), int(g["band_cells"])) == R.band_rule(nf, N, _span(len(nm)), max(layout, 0)), tag
        assert (int(g["sum_bits"]), int(g["sum_points"])) == (61, N), tag
    if want[0].startswith("lds"):
        use_pad, raw48, nwg, per = R._lds_slabs(nf, W, tol, N, chan, env, normal)
        assert (int(g["nwg"]), int(g["nslab"]), int(g["per"])) == (nwg, nwg, per), tag
        assert (int(g["sum_bits"]), int(g["sum_points"])) == ((46, per) if raw48 else (61, N)), tag
    assert bool(int(g["class_order"])) == R.class_order_wanted(want[0], len(nm), N, env), tag
    if want[1] == "g2m":
        assert int(g["g2m_two_launch"]) == 1 and _axes(g["g2m_h"]) == tuple(m // 2 for m in nm), tag
    if want[1].startswith("pruned"):
        assert _axes(g["nc"]) == tuple(min(2 * (m // 2) + 1, f) for m, f in zip(nm, nf)), tag


def _check2(tag, g, nm, tol, N, B, real_only, want, env, dense=False):
    nf, W = R.window(nm, tol, dense)
    assert (_axes(g["nf"]), int(g["W"])) == (nf, W), tag
    got = (g["grid"], g["gather"])
    assert got == want, (tag, got)
    if want[1] == "tiles":
        assert (_axes(g["tile_nt"]), _axes(g["tile_T"])) == R.tile_geom(nf, W, 1 if real_only else 2), tag
    assert bool(int(g["class_order"])) == R.class_order_wanted(want[1], len(nm), N, env), tag
    if want[0] == "pruned":
        assert _axes(g["nc"]) == tuple(min(2 * (m // 2) + 1, f) for m, f in zip(nm, nf)), tag
    cells = 1
    for f in nf:
        cells *= f
    assert int(g["fine_bytes"]) == max(B * cells * 16, int(g["pair_bytes"]) if want[0] == "image" else 0), tag


def _type1_lines(table):
    return [(_line("t1", nm, tol, N, 2 if cplx else 1, layout=kw.get("layout_band", 0)), kw.get("env", ()))
            for nm, tol, N, cplx, h, _, kw in table.values()]


def _type2_lines(table):
    return [(_line("t2", nm, tol, N, real_only, batch=B or 1), ()) for nm, tol, N, B, real_only, h, _ in table.values()]


FAMILY_VARIANTS = [(chan, normal) for chan in (1, 2) for normal in (False, True)]      # real rows, pair grids / complex; generated normals


def _family_lines():
    return [(_line("t1", nm, FAMILY_TOL, N, chan, normal=normal, layout=band), ())
            for nm, N, h, band in FAMILY.values() for chan, normal in FAMILY_VARIANTS]


@pytest.mark.parametrize("hooks", HOOK_SETS, ids=[h[0] if h else "no_hook" for h in HOOK_SETS])
def test_named_cases_are_planned_as_restated(plan_check, hooks):
    assert len(R.TYPE1) == 14 and len(R.TYPE2) == 14 and len(FAMILY) == 3
    for table in (R.TYPE1, EXTRA1):
        for (name, (nm, tol, N, cplx, h, expect, kw)), g in zip(table.items(), plan_check(_type1_lines(table), hooks)):
            env = tuple(kw.get("env", ())) + hooks
            args = dict(layout_band=kw.get("layout_band", 0), span_periods=R.SPAN_PERIODS, env=env)
            want = R.type1_route(nm, tol, N, 2 if cplx else 1, **args)
            if not hooks:
                assert want == expect, name                     # the recorded tuple, not only what the restatement says today
            _check1((name, hooks), g, nm, tol, N, 2 if cplx else 1, want, env, layout=kw.get("layout_band", 0))
    for table in (R.TYPE2, EXTRA2):
        for (name, (nm, tol, N, B, real_only, h, expect)), g in zip(table.items(), plan_check(_type2_lines(table), hooks)):
            want = R.type2_route(nm, tol, N, B or 1, real_only, env=hooks)
            if not hooks:
                assert want == expect, name
            _check2((name, hooks), g, nm, tol, N, B or 1, real_only, want, hooks)
    got = iter(plan_check(_family_lines(), hooks))
    for name, (nm, N, h, band) in FAMILY.items():
        for chan, normal in FAMILY_VARIANTS:
            g = next(got)
            want = R.type1_route(nm, FAMILY_TOL, N, chan, layout_band=band, span_periods=R.SPAN_PERIODS, env=hooks, normal=normal)
            if not hooks:
                assert want[0].startswith(name), (name, chan, normal, want)
            _check1((name, chan, normal, hooks), g, nm, FAMILY_TOL, N, chan, want, hooks, layout=band, normal=normal)


def test_generated_normals_keep_61_bit_sums(plan_check):
    """The `normal` flag: the LDS family's box takes 48-bit raw sums for strengths from memory and 61-bit sums for generated
    normals, and the cell-sorted route is not taken for them."""
    nm, N, h, band = FAMILY["lds"]
    for chan in (1, 2):
        assert R.type1_route(nm, FAMILY_TOL, N, chan)[0] == "lds_pad_raw48"
        assert R.type1_route(nm, FAMILY_TOL, N, chan, normal=True)[0] == "lds_pad_61"
        assert R.type1_route(nm, FAMILY_TOL, N, chan, env=("EFGP_CELLSORT",))[0] == "cells"
        assert R.type1_route(nm, FAMILY_TOL, N, chan, env=("EFGP_CELLSORT",), normal=True)[0] == "lds_pad_61"
    g = plan_check([(_line("t1", nm, FAMILY_TOL, N, 1, normal=True), ("EFGP_CELLSORT",))])[0]
    assert g["spreader"] == "lds_pad_61"


def test_unforced_band_rule_and_class_order(plan_check):
    """Rules no named case sits on, planner against restatement: the 192 / 24 points per run of an unforced layout, and the class
    order from 64 windows of points on (padded rows; the halo gather that is not the pair gather; never in 1-D)."""
    nf = (64, 128)
    # 128 x 1.03 cells of axis 1 make 256 one-cell bands or 32 eight-cell ones over 76.8 cells of axis 0: 192 points per run of the
    # first need 3.8 million points, 24 per run of the second 58,983
    assert R.band_rule(nf, 4000000, R.SPAN_PERIODS) == (256, 1) and R.band_rule(nf, 3700000, R.SPAN_PERIODS) == (32, 8)
    assert R.band_rule(nf, 65536, R.SPAN_PERIODS) == (32, 8) and R.band_rule(nf, 58000, R.SPAN_PERIODS) is None
    lines = [(_line("t1", (23, 45), 1e-7, N, 1, layout=-1), ()) for N in (58000, 65536, 3700000)]
    got = plan_check(lines, ("EFGP_NO_DENSE_SIGMA",))
    assert [(g["spreader"], int(g["level_bands"]), int(g["band_cells"])) for g in got[1:]] == [("layout", 32, 8)] * 2
    below = R.type1_route((23, 45), 1e-7, 58000, 1, layout_band=-1, span_periods=R.SPAN_PERIODS)[0]
    assert below != "layout" and got[0]["spreader"] == below and int(got[0]["level_bands"]) == 0
    got = plan_check([(_line("t1", (23, 45), 1e-7, 4000000, 1, layout=-1), ())], ("EFGP_NO_DENSE_SIGMA",))[0]
    assert (got["spreader"], int(got["level_bands"]), int(got["band_cells"])) == ("layout", 256, 1)

    many = R.ORDER_WINDOW * 64
    cases = [("t1", (23, 45), many, 1, True), ("t1", (23, 45), many - 1, 1, False), ("t1", (36,), many, 1, False),
             ("t2", (33, 40), many, 1, True), ("t2", (33, 40), many - 1, 1, False), ("t2", (23, 45), many, 1, False), ("t2", (36,), many, 1, False)]
    got = plan_check([(_line(kind, nm, 1e-7, N, chan, batch=2 if kind == "t2" else 1), ()) for kind, nm, N, chan, _ in cases])
    for (kind, nm, N, chan, want), g in zip(cases, got):
        route = g["spreader"] if kind == "t1" else g["gather"]
        assert route == (R.type1_route(nm, 1e-7, N, chan)[0] if kind == "t1" else R.type2_route(nm, 1e-7, N, 2, True)[1]), (kind, nm, N)
        assert bool(int(g["class_order"])) == want == R.class_order_wanted(route, len(nm), N), (kind, nm, N)


def _named_routes(hooks=()):
    """name -> route of every named case (R.TYPE1, R.TYPE2, FAMILY) and of the extra ones, by the restatement."""
    out = {}
    for table in (R.TYPE1, EXTRA1):
        for name, (nm, tol, N, cplx, h, _, kw) in table.items():
            out["1:" + name] = R.type1_route(nm, tol, N, 2 if cplx else 1, layout_band=kw.get("layout_band", 0), span_periods=R.SPAN_PERIODS,
                                             env=tuple(kw.get("env", ())) + tuple(hooks))
    for table in (R.TYPE2, EXTRA2):
        for name, (nm, tol, N, B, real_only, h, _) in table.items():
            out["2:" + name] = R.type2_route(nm, tol, N, B or 1, real_only, env=hooks)
    for name, (nm, N, h, band) in FAMILY.items():
        for chan, normal in FAMILY_VARIANTS:
            out[f"f:{name}:{chan}:{int(normal)}"] = R.type1_route(nm, FAMILY_TOL, N, chan, layout_band=band, span_periods=R.SPAN_PERIODS,
                                                                  env=hooks, normal=normal)
    return out


def test_the_hooks_move_the_named_cases():
    """The hook sets are not idle on the case list: each changes the route of at least one case.  EFGP_NO_GATHER_IMAGE moves the
    extra case `real_image` only -- no case of R.TYPE2 takes the image."""
    base = _named_routes()
    for hooks in HOOK_SETS[1:]:
        moved = [n for n, r in _named_routes(hooks).items() if r != base[n]]
        assert moved, hooks
        if hooks != ("EFGP_NO_GATHER_IMAGE",):
            assert any("fft_beyond" not in n and "real_image" not in n for n in moved), hooks
        else:
            assert moved == ["2:real_image"]


def test_every_terminal_route_is_reached(plan_check):
    """Every spreader, follow-up, grid source and gather the planner can return is reached without a hook: by the named cases, but
    for the cell-sorted spreader (opt-in: its case sets EFGP_CELLSORT), the gather's image and the full FFT (the extra cases)."""
    named1 = plan_check(_type1_lines(R.TYPE1) + _family_lines())
    named2 = plan_check(_type2_lines(R.TYPE2))
    spreaders = {"layout", "cells", "tiles", "lds_pad_raw48", "lds_pad_61", "lds_plain", "global"}
    no_switch = [g for g, (_, own) in zip(named1, _type1_lines(R.TYPE1) + _family_lines()) if not own]
    assert {g["spreader"] for g in no_switch} == spreaders - {"cells"} and {g["spreader"] for g in named1} == spreaders
    assert {g["after"] for g in named1} == {"g2m_from_acc", "g2m", "pruned_from_acc", "pruned"}
    assert {g["grid"] for g in named2} == {"direct", "pruned"}
    assert {g["gather"] for g in named2} == {"tiles", "pair", "halo", "lds", "l2"}
    extra1, extra2 = plan_check(_type1_lines(EXTRA1)), plan_check(_type2_lines(EXTRA2))
    assert {g["after"] for g in extra1} == {"fft"} and {g["grid"] for g in extra2} == {"image", "fft"}
