"""CPU checks of the raster transform's restatement (tests/_raster.py), of its C ABI declarations and of the host planner
(csrc/raster_plan_host.cpp) through the stand-alone program tools/raster_plan_check.cpp.

The program is compiled once per session without the sanitizer flags (the sanitized build is the tool's documented command line,
run by hand); the compiler is found as efgp_hip/build.py finds it.
"""
import math
import os
import subprocess

import pytest
import torch

import _nudft
import _raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp-quadrature_amd", "csrc")

# mode box -> raster; per-axis h as power-of-two multiples of the first (the exact sums take one h: the axes are rescaled exactly)
RESTATEMENT_CASES = [
    ((67,), (33,), (1.0,)),
    ((1,), (1,), (1.0,)),
    ((4,), (16,), (1.0,)),
    ((23, 5), (17, 15), (1.0, 0.5)),
    ((16, 3), (1, 33), (1.0, 1.0)),
    ((2, 64), (48, 16), (1.0, 2.0)),
    ((7, 4, 9), (5, 17, 3), (1.0, 0.5, 2.0)),
    ((1, 2, 3), (16, 1, 2), (1.0, 1.0, 1.0)),
    ((13, 13, 13), (20, 9, 33), (1.0, 1.0, 0.25)),
]


@pytest.mark.parametrize("modeord", [0, 1])
@pytest.mark.parametrize("case", range(len(RESTATEMENT_CASES)))
def test_restatement_matches_the_exact_sums(case, modeord):
    """Both sides take sines of angles up to 2 pi 70 = 440 built from three rounded factors: 3 * 2^-53 * 440 = 1.5e-13 per term, axis
    and side, 9e-13 sum |f| for three axes and two sides.  Bound 1e-12 sum |f|."""
    shape, n_axis, hrel = RESTATEMENT_CASES[case]
    isign = -1 if case % 2 else 1
    axes, hs, xcen, f, sc = _raster.make_case(shape, n_axis, hrel, seed=100 + case, nbatch=2, scale=bool(case % 3), center=bool(case % 2 == 0))
    got = _raster.type2(axes, hs, f, shape, isign=isign, modeord=modeord, xcen=xcen, mode_scale=sc)
    want, mag = _raster.exact(axes, hs, f, shape, isign, modeord, xcen, sc)
    assert got.shape == want.shape == (2,) + tuple(n_axis)
    err = ((got - want).abs().reshape(2, -1).max(dim=1).values / mag).max().item()
    print(f"restatement {shape} -> {n_axis} modeord {modeord}: max err / sum|f| = {err:.2e}")
    assert err <= 1e-12


def test_raster_entries_are_declared():
    import efgp_hip
    import importlib
    L = importlib.import_module("efgp_hip.lib")
    names = efgp_hip.declared_symbols()
    for name in ("efgp_raster_type2", "efgp_raster_plan"):
        assert name in names
        assert name in L._SIGNATURES


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("raster_plan_check") / "raster_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I/opt/rocm/include", os.path.join(ROOT, "tools", "raster_plan_check.cpp"),
           os.path.join(CSRC, "raster_plan_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)

    def run(cases):
        """cases: (n_modes, n_axis, nbatch, cap) -> one dict of the printed fields per case."""
        pad = lambda v: " ".join(str(n) for n in tuple(v) + (1,) * (3 - len(v)))
        text = "".join(f"{len(m)} {pad(m)} {pad(n)} {nb} {cap}\n" for m, n, nb, cap in cases)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [dict(field.split("=", 1) for field in line.split()) for line in out]

    return run


def _cap_for(n_modes, n_axis, nbatch, rows):
    """A cap that holds the tables and exactly `rows` slab rows (plus a few bytes that buy nothing)."""
    p = _raster.plan(n_modes, n_axis, nbatch)
    return p["table_bytes"] + rows * p["row_bytes"] + 7


# (mode box, raster, nbatch, cap, slabs expected or None where only the restatement decides, refused)
PLAN_CASES = [
    ((67,), (33,), 1, 0, 1, False),
    ((201,), (257,), 3, 0, 1, False),
    ((4,), (16,), 1, 100, None, True),                                                     # 1-D: the tables alone exceed the cap
    ((23, 5), (50, 15), 1, 0, 1, False),
    ((23, 5), (50, 15), 1, _cap_for((23, 5), (50, 15), 1, 16), 4, False),                 # 16 + 16 + 16 + 2: a short last slab
    ((23, 5), (50, 15), 1, _cap_for((23, 5), (50, 15), 1, 47), 2, False),                 # 47 rows fit, 32 are taken
    ((23, 5), (48, 15), 3, _cap_for((23, 5), (48, 15), 3, 16), 3, False),                 # three full slabs
    ((23, 5), (50, 15), 1, _cap_for((23, 5), (50, 15), 1, 16) - 8, None, True),           # one byte short of a tile row
    ((201, 201), (4096, 4096), 1, 0, 1, False),
    ((201, 201), (4096, 4096), 1, _cap_for((201, 201), (4096, 4096), 1, 16), 256, False),  # many slabs
    ((7, 4, 9), (40, 17, 3), 1, _cap_for((7, 4, 9), (40, 17, 3), 1, 16), 3, False),       # 16 + 16 + 8
    ((7, 4, 9), (40, 17, 3), 2, 0, 1, False),
    ((57, 57, 57), (256, 256, 256), 1, 0, 1, False),
    ((57, 57, 57), (256, 256, 256), 16, 128 << 20, 16, False),
    ((57, 57, 57), (256, 256, 256), 1, 1 << 20, None, True),
    ((13, 13, 13), (20, 9, 33), 3, 1, None, True),
    ((1, 2, 3), (16, 1, 2), 1, 0, 1, False),
    ((1 << 20, 1 << 20, 1 << 20), ((1 << 31) - 1,) * 3, 1 << 16, 0, None, True),          # the largest sizes accepted: no overflow
    ((0, 5), (4, 4), 1, 0, None, True),
    ((5, 5), (4, 0), 1, 0, None, True),
]


def test_planner_matches_its_restatement(plan_check):
    got = plan_check([(m, n, nb, cap) for m, n, nb, cap, _, _ in PLAN_CASES])
    seen = set()
    for (m, n, nb, cap, slabs, refused), g in zip(PLAN_CASES, got):
        want = _raster.plan(m, n, nb, cap)
        assert (want is None) == refused, (m, n, nb, cap)
        assert int(g["ok"]) == (0 if refused else 1), (m, n, nb, cap)
        if refused:
            continue
        assert tuple(int(k) for k in g["Kpad"].split("x")) == want["Kpad"], (m, n)
        for key in ("table_bytes", "row_bytes", "slab_rows", "slabs", "workspace_bytes"):
            assert int(g[key]) == want[key], (m, n, nb, cap, key)
        assert want["slab_rows"] % _raster.TILE == 0 and want["workspace_bytes"] <= (cap or _raster.DEFAULT_WORKSPACE)
        if slabs is not None:
            assert want["slabs"] == slabs, (m, n, nb, cap)
        seen.add(min(want["slabs"], 5))
        if want["slabs"] > 1 and n[0] % want["slab_rows"]:
            seen.add("short")
    assert {1, 3, 5, "short"} <= seen                 # 1, 3 and many slabs, and a short last slab


def test_refusal_names_the_bytes_needed():
    """The library's own entry (host only, no device touched) refuses a small cap as ValueError with the bytes it needs."""
    from efgp_hip import ops
    want = _raster.plan((23, 5), (50, 15), 1)
    with pytest.raises(ValueError, match=str(want["least_bytes"])):
        ops.raster_plan((50, 15), (23, 5), 1, want["least_bytes"] - 1)
    ok = ops.raster_plan((50, 15), (23, 5), 1, want["least_bytes"])
    assert ok == dict(slab_rows=16, slabs=4, workspace_bytes=want["least_bytes"])
