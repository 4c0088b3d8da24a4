"""CPU check of the host planners of the CG paths (csrc/cg_plan_host.cpp) through the stand-alone program tools/cg_plan_check.cpp:
what efgp_toeplitz_create_ex decides for a block, the grid a solve runs on, the kernel the persistent solve picks and the launch
shape of the cooperative solve, field by field against their restatement in tests/_cg_routes.py.

The program is compiled once per session without the sanitizer flags (the sanitized build is the tool's documented command line,
run by hand); the compiler is found as efgp_hip/build.py finds it -- without it the library cannot be built either.
"""
import os
import subprocess

import pytest

import _cg_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gp-quadrature_amd", "csrc")
# the hook sets tests/test_dense_toeplitz_host.py::test_geometry_of_the_cases walks
HOOK_SETS = [(), ("EFGP_NO_CG48",), ("EFGP_NO_CG64_EMBED",), ("EFGP_NO_PERSISTENT_CG",), ("EFGP_NO_CG_COOP",), ("EFGP_NO_CG_LINES",)]
NUM_CU, MAX_LDS = 256, 163840
PICKS = {"herm48": "herm48", "herm64": "herm64", "line1d": "line1d", "2d64": "fast64", "generic": "generic"}


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cg_plan_check") / "cg_plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I/opt/rocm/include", os.path.join(ROOT, "tools", "cg_plan_check.cpp"),
           os.path.join(CSRC, "cg_plan_host.cpp"), os.path.join(CSRC, "es_kernel.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)

    def run(cases, hooks=()):
        """cases: (ns, hermitian, nbatch) -> one dict of the printed fields per case."""
        env = {k: v for k, v in os.environ.items() if not k.startswith("EFGP_")}
        env.update({h: "1" for h in hooks})
        text = "".join(f"{len(ns)} {' '.join(str(n) for n in tuple(ns) + (1,) * (3 - len(ns)))} {int(herm)} {nb} {NUM_CU} {MAX_LDS}\n"
                       for ns, herm, nb in cases)
        out = subprocess.run([exe], input=text, env=env, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [dict(field.split("=", 1) for field in line.split()) for line in out]

    return run


def _grid(text):
    return tuple(int(f) for f in text.split("x"))


def _coop(text):
    return {k: int(v) for k, v in (kv.split(":") for kv in text.split(","))}


@pytest.mark.parametrize("hooks", HOOK_SETS, ids=[h[0] if h else "no_hook" for h in HOOK_SETS])
def test_named_cases_are_planned_as_restated(plan_check, hooks):
    names = list(R.CASES)
    assert len(names) == 46
    got = plan_check([(R.CASES[nm][0], R.CASES[nm][1], 1) for nm in names], hooks)
    for nm, g in zip(names, got):
        ns, herm, _ = R.CASES[nm]
        op = R.operator(ns, hooks)
        assert _grid(g["F"]) == op["F"], nm
        for key in ("persistent_ok", "cg64", "h48", "lines_ok", "lines3_ok"):
            assert bool(int(g[key])) == bool(op[key]), (nm, key)
        assert (_grid(g["coop_grid"]) if "coop_grid" in g else None) == op["coop_grid"], nm
        assert _grid(g["cg_shape"]) == R.cg_shape(ns, herm, hooks), nm
        kernel, grid = R.route(ns, herm, hooks)
        if kernel in PICKS:
            assert g["pick"] == PICKS[kernel], nm
            pick_grid = _grid(g["pick_grid"])
            if kernel == "herm48":
                assert grid == (48, 48) == _grid(g["cg_shape"]) and pick_grid == (64, 64), nm
            elif kernel == "generic":
                assert grid == tuple(f for f in pick_grid if f > 1), nm
            else:
                assert grid == pick_grid, nm
        else:
            assert "pick" not in g, nm
        # the Lanczos mode of the same block (efgp_lanczos): line1d and the Hermitian kernels are barred
        lz_kernel = R.route(ns, herm, hooks, lanczos=True)[0]
        if lz_kernel in PICKS:
            assert lz_kernel in ("2d64", "generic") and g["lz_pick"] == PICKS[lz_kernel], nm
        else:
            assert "lz_pick" not in g and kernel not in PICKS, nm
        if kernel in ("coop", "coop_herm"):
            shape = _coop(g["coop"])
            assert shape["ok"] == 1 and shape["herm"] == (kernel == "coop_herm") and _grid(g["coop_grid"]) == grid, nm


def test_the_hooks_move_the_named_cases():
    """The hook sets are not idle on the case list: each changes the route of at least one case."""
    for hooks in HOOK_SETS[1:]:
        assert any(R.route(ns, herm, hooks) != R.route(ns, herm) for ns, herm, _ in R.CASES.values()), hooks


# the smallest shapes (by n0 n1 systems) that reach each cooperative kernel at 256 CUs and 163,840 B of LDS:
# (block, systems, Hermitian) -> (Hermitian kernel, vector entries per thread, grid, workgroups per system)
COOP_KERNELS = {
    ((33, 33), 1, False): (0, 4, (96, 96), 12),
    ((85, 129), 11, False): (0, 8, (192, 384), 12),
    ((33, 33), 86, False): (0, 8, (96, 96), 1),
    ((33, 33), 1, True): (1, 4, (96, 96), 6),
    ((43, 129), 43, True): (1, 8, (96, 384), 3),
    ((33, 33), 86, True): (1, 4, (96, 96), 1),
    ((47, 47), 86, True): (1, 8, (96, 96), 1),
}


def test_every_cooperative_kernel_is_reached(plan_check):
    cases = list(COOP_KERNELS)
    for (ns, nb, herm), g in zip(cases, plan_check([(ns, herm, nb) for ns, nb, herm in cases])):
        want_herm, ks, grid, G = COOP_KERNELS[(ns, nb, herm)]
        shape = _coop(g["coop"])
        assert shape["ok"] == 1 and (shape["herm"], shape["ks"], shape["G"]) == (want_herm, ks, G), (ns, nb, herm, shape)
        assert _grid(g["coop_grid"]) == grid == R.cg_shape(ns, herm), (ns, nb, herm)
    # the one combination without a kernel: the general solve, one workgroup per system, 4 entries per thread
    assert {(h, ks, G == 1) for h, ks, _, G in COOP_KERNELS.values()} == {(h, ks, solo) for h in (0, 1) for ks in (4, 8) for solo in (False, True)} - {(0, 4, True)}
