"""CPU checks of the raster type-1 planner (plan_raster_type1 in csrc/raster_plan_host.cpp): through the stand-alone program
tools/raster_type1_plan_check.cpp and through the library's host-only entry efgp_raster_type1_plan, against the restatement
tests/_raster_adjoint.py::plan.

The program is compiled once per session without the sanitizer flags (the sanitized build is the tool's documented command line,
run by hand); the compiler is found as efgp_hip/build.py finds it.
"""
import os
import subprocess

import pytest

import _raster
import _raster_adjoint as _ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp-quadrature_amd", "csrc")


def test_type1_entries_are_declared():
    import efgp_hip
    import importlib
    L = importlib.import_module("efgp_hip.lib")
    names = efgp_hip.declared_symbols()
    for name in ("efgp_raster_type1", "efgp_raster_type1_plan"):
        assert name in names
        assert name in L._SIGNATURES
        assert hasattr(efgp_hip.lib(), name)


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("raster_type1_plan_check") / "raster_type1_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I/opt/rocm/include",
           os.path.join(ROOT, "tools", "raster_type1_plan_check.cpp"), os.path.join(CSRC, "raster_plan_host.cpp"), "-o", exe]
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
    p = _ra.plan(n_modes, n_axis, nbatch)
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
    ((23, 23), (4096, 4096), 1, 0, 1, False),
    ((45, 45), (4096, 4096), 1, _cap_for((45, 45), (4096, 4096), 1, 16), 256, False),     # many slabs
    ((7, 4, 9), (40, 17, 3), 1, _cap_for((7, 4, 9), (40, 17, 3), 1, 16), 3, False),       # 16 + 16 + 8
    ((7, 4, 9), (40, 17, 3), 2, 0, 1, False),
    ((57, 57, 57), (256, 256, 256), 1, 0, 1, False),
    ((57, 57, 57), (256, 256, 256), 16, 128 << 20, None, False),
    ((57, 57, 57), (256, 256, 256), 1, 1 << 20, None, True),
    ((13, 13, 13), (20, 9, 33), 3, 1, None, True),
    ((1, 2, 3), (16, 1, 2), 1, 0, 1, False),
    ((1 << 20, 1 << 20, 1 << 20), ((1 << 31) - 1,) * 3, 1 << 16, 0, None, True),          # the largest sizes accepted: no overflow
    ((1 << 20, 1), ((1 << 31) - 1, 1), 1 << 16, (1 << 62) - 1, None, False),              # ... and a plan near the 62-bit limit
    ((0, 5), (4, 4), 1, 0, None, True),
    ((5, 5), (4, 0), 1, 0, None, True),
]


def test_planner_matches_its_restatement(plan_check):
    from efgp_hip import ops
    got = plan_check([(m, n, nb, cap) for m, n, nb, cap, _, _ in PLAN_CASES])
    seen = set()
    for (m, n, nb, cap, slabs, refused), g in zip(PLAN_CASES, got):
        want = _ra.plan(m, n, nb, cap)
        assert (want is None) == refused, (m, n, nb, cap)
        assert int(g["ok"]) == (0 if refused else 1), (m, n, nb, cap)
        if refused:
            with pytest.raises(ValueError):
                ops.raster_type1_plan(n, m, nb, cap)
            continue
        assert tuple(int(k) for k in g["Kpad"].split("x")) == want["Kpad"], (m, n)
        for key in ("table_bytes", "row_bytes", "slab_rows", "slabs", "workspace_bytes"):
            assert int(g[key]) == want[key], (m, n, nb, cap, key)
        assert ops.raster_type1_plan(n, m, nb, cap) == {k: want[k] for k in ("slab_rows", "slabs", "workspace_bytes")}
        assert want["slab_rows"] % _raster.TILE == 0 and want["slab_rows"] % _ra.CHUNK == 0
        assert want["workspace_bytes"] <= (cap or _raster.DEFAULT_WORKSPACE)
        assert want["workspace_bytes"] < 1 << 63
        if slabs is not None:
            assert want["slabs"] == slabs, (m, n, nb, cap)
        seen.add(min(want["slabs"], 5))
        if want["slabs"] > 1 and n[0] % want["slab_rows"]:
            seen.add("short")
    assert {1, 3, 5, "short"} <= seen                 # 1, 3 and many slabs, and a short last slab


def test_refusal_names_the_bytes_needed():
    """The library's own entry (host only, no device touched) refuses a small cap as ValueError with the bytes it needs."""
    from efgp_hip import ops
    want = _ra.plan((23, 5), (50, 15), 1)
    with pytest.raises(ValueError, match=str(want["least_bytes"])):
        ops.raster_type1_plan((50, 15), (23, 5), 1, want["least_bytes"] - 1)
    ok = ops.raster_type1_plan((50, 15), (23, 5), 1, want["least_bytes"])
    assert ok == dict(slab_rows=16, slabs=4, workspace_bytes=want["least_bytes"])


def test_type2_planner_is_unchanged_by_the_type1_planner():
    """The two planners share sizes and refusals, not formulas: the type-2 entry still answers its own restatement."""
    from efgp_hip import ops
    for m, n, nb in (((23, 5), (50, 15), 1), ((7, 4, 9), (40, 17, 3), 2)):
        want = _raster.plan(m, n, nb)
        assert ops.raster_plan(n, m, nb) == {k: want[k] for k in ("slab_rows", "slabs", "workspace_bytes")}
