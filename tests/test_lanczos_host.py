"""CPU checks of the Lanczos references (tests/_lanczos.py): what tests/test_gpu_lanczos.py asks of the kernels is made a fact about
the references alone first.

Three constructions of the same recurrence -- the dense matrix in f64, the dense matrix in 80-bit, the oracle's FFT product in f64 --
are held to each other step by step (the compared prefix must be at least min(6, K) long), their 25-step Gauss-Lanczos quadrature to
the exact z^H log(A) z from eigh of the dense matrix (1e-13 relative), and the breakdown cases must break at the same step in all
three with the last beta ten times under the threshold.

Measured when this was written (every case, both variants, one +-1 and one complex probe): all K = min(12, M) steps agree below
1e-12, except on 3d_1x1x9 whose last two of nine steps -- the ones before the Krylov space is exhausted -- move by up to 1e-4;
quadrature against the exact value at most 8e-15.

Breakdown.  The threshold beta < 1e-12 is absolute and the recurrence amplifies rounding as the Krylov space runs out, so the f64
references take the break only where it comes within about three steps.  Measured: ws = 0 on (8, 8) breaks at step 1 with beta
exactly 0; ws non-zero at one mode of (8, 8) and of (20, 30) at step 2; (2,) at 2; (3,) and (1, 1, 3) at 3, every last beta below
3e-14.  Not used: (2, 2) breaks at step 4 with a last beta of up to 8e-14 and (2, 3) at step 6 with 4e-13, inside the threshold by
less than the factor of ten; rank-3 ws on (2, 3, 5) breaks at 4 with 3e-14, no better; with rank-4 ws on (700,) one of two probes
runs all ten steps in f64 (beta 4e-8 at step 10) where the 80-bit recurrence breaks at step 5.  That f64 Lanczos misses a break
more than about three steps in is a property of the reference project's rule, which the kernel copies: none of the latter may be
used to assert `taken`.
"""
import math

import numpy as np
import pytest
import torch

import _cg_routes as R
import _dense_toeplitz as D
import _lanczos as L


@pytest.fixture(autouse=True)
def _serial():
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def _two_probes(ns):
    z = L.probes(ns)
    return {"pm1": z[0], "complex": z[2]}


@pytest.mark.parametrize("name", list(L.CASES))
def test_references_agree_on_a_prefix(name):
    ns, _ = L.CASES[name]
    s = D.system(ns)
    K = min(L.STEPS, math.prod(ns))
    for variant in (0, 1):
        A = L.matrix(ns, variant)
        for kind, z in _two_probes(ns).items():
            r = L.references(A, s, variant, z, K)
            print(f"\n{name} variant {variant} {kind}: taken {r['f64'][3]} {r['fft'][3]} {r['ld'][3]}, prefix {r['prefix']} of {K}, "
                  f"max d on it {r['d'][:r['prefix']].max():.1e}, max d {r['d'].max():.1e}")
            assert r["prefix"] >= min(6, K), (name, variant, kind, r["d"])
            for key in ("f64", "fft", "ld"):
                assert float(r[key][2]) == pytest.approx(float((z.abs() ** 2).sum()), rel=1e-14)


@pytest.mark.parametrize("name", list(L.CASES))
def test_quadrature_equals_the_exact_quadratic_form(name):
    ns, _ = L.CASES[name]
    s = D.system(ns)
    M = math.prod(ns)
    for variant in (0, 1):
        A = L.matrix(ns, variant)
        for kind, z in _two_probes(ns).items():
            f64 = L.lanczos_dense(A, z, L.QUAD_STEPS)
            fft = L.lanczos_fft(s, variant, z, L.QUAD_STEPS)
            qd, qf = L.quadrature(*f64[:3]), L.quadrature(*fft[:3])
            # blocks above EIGH_MAX: the dense recurrence's own quadrature stands in for eigh of the dense matrix
            exact = L.exact_quadratic_form(L.eigen(ns, variant), z) if M <= L.EIGH_MAX else qd
            print(f"\n{name} variant {variant} {kind}: exact {exact:.15g}, dense {abs(qd - exact) / abs(exact):.1e}, "
                  f"FFT {abs(qf - exact) / abs(exact):.1e} ({f64[3]}, {fft[3]} steps)")
            assert abs(qd - exact) <= 1e-13 * abs(exact) and abs(qf - exact) <= 1e-13 * abs(exact)


@pytest.mark.parametrize("name", list(L.BREAKDOWN))
def test_breakdown_cases_qualify(name):
    """Variant 1 only: the threshold is absolute, and at sigma^2 = 150 variant 0 does not reach it reliably."""
    ns, ws_key, taken = L.BREAKDOWN[name]
    s = D.system(ns)
    A = L.matrix(ns, 1, ws_key)
    ws = L.weights(ns, ws_key)
    for kind, z in zip(("pm1", "pm1", "complex", "complex"), L.probes(ns)):      # the four rows tests/test_gpu_lanczos.py runs
        r = L.references(A, s, 1, z, 10, ws)
        last = [float(r[k][1][-1]) for k in ("f64", "fft", "ld")]
        print(f"\n{name} {kind}: taken {[r[k][3] for k in ('f64', 'fft', 'ld')]}, last beta {last}")
        assert [r[k][3] for k in ("f64", "fft", "ld")] == [taken] * 3
        assert max(last) < 1e-13
        assert r["prefix"] == taken                                # d_k is relative to |alpha_k|: the last beta, pure rounding, passes it
        if ws_key == "zero" and kind == "pm1":                     # A = I and q = z / 8: every operation is exact
            assert last == [0.0, 0.0, 0.0] and float(r["f64"][0][0]) == 1.0


def test_full_ws_runs_all_steps_on_the_breakdown_blocks():
    """The other side of the breakdown tests: the system's own ws on (8, 8) and (20, 30) does not break in 10 steps."""
    for ns in ((8, 8), (20, 30)):
        z = L.probes(ns)[0]
        assert L.lanczos_dense(L.matrix(ns, 1), z, 10)[3] == 10
        assert L.lanczos_fft(D.system(ns), 1, z, 10)[3] == 10


def test_lanczos_routes():
    """Lanczos bars line1d, herm64 and herm48: 1-D blocks and odd squares run the general kernels, whatever the promise."""
    assert {n: k for n, (_, k) in L.CASES.items()} == L.ROUTES
    for name, (ns, kernel) in L.CASES.items():
        for herm in (False, True):
            assert R.route(ns, herm, lanczos=True)[0] == kernel == L.ROUTES[name], name
    assert len({ns for ns, _ in L.CASES.values()}) == len(L.CASES) == 33
    # every dense block is either a case or refused
    assert {ns for ns, _, _ in R.DENSE.values()} == {ns for ns, _ in L.CASES.values()} | {ns for nm, ns in L.REFUSED.items() if nm in R.DENSE}
    for name, ns in L.REFUSED.items():
        assert not R.single_launch_solves(ns), name
        assert R.route(ns, lanczos=True)[0] not in ("generic", "2d64"), name
    # the moves, side by side with the solve's routes
    assert [R.route((n,))[0] for n in (3, 255)] == ["line1d", "line1d"] and [R.route((n,), lanczos=True)[0] for n in (3, 255)] == ["generic"] * 2
    assert [R.route((n, n), True)[0] for n in (23, 25, 31)] == ["herm48", "herm64", "herm64"]
    assert [R.route((n, n), True, lanczos=True) for n in (23, 25, 31)] == [("2d64", (64, 64))] * 3
    assert [R.route((n, n), lanczos=True, env=("EFGP_NO_CG64",))[0] for n in (8, 23, 24, 32)] == ["generic"] * 4
    assert R.route((8, 8), lanczos=True, env=("EFGP_NO_CG64_EMBED",)) == ("generic", (16, 16))
    assert R.route((8, 8), lanczos=True, env=("EFGP_NO_PERSISTENT_CG",))[0] == "multi_fft"


def test_quadrature_of_a_diagonal_matrix():
    """The two definitions on a matrix whose answer is known: A = diag(1..5), z = ones: sum log k."""
    A = torch.diag(torch.arange(1.0, 6.0, dtype=torch.float64)).to(torch.complex128)
    z = torch.ones(5, dtype=torch.complex128)
    want = sum(math.log(k) for k in range(1, 6))
    al, be, n2, taken = L.lanczos_dense(A, z, 5)
    assert taken == 5 and float(n2) == 5.0
    assert L.quadrature(al, be, n2) == pytest.approx(want, rel=1e-13)
    assert L.exact_quadratic_form(A, z) == pytest.approx(want, rel=1e-14)
    assert np.allclose(L.lanczos_dense(A, z, 5, np.clongdouble)[0].astype(np.float64), al, rtol=1e-13)
