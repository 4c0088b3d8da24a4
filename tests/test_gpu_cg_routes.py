"""GPU: every route of the CG solves (csrc/cg_persistent.hip, csrc/cg_herm.hip, csrc/cg_coop2d.hip, csrc/cg_multi.hip; dispatch: csrc/toeplitz_cg.hip) on non-cubic, even and edge blocks, held to a
dense solve.

The reference of the dense cases is the block Toeplitz matrix written down from the definition (tests/_dense_toeplitz.py) -- not
the circulant embedding every kernel and the oracle's Toeplitz use; the oracle's CG loops run on its matrix product.  The cases and
the route each must take are in tests/_cg_routes.py (asserted without a GPU by tests/test_dense_toeplitz_host.py).  Blocks too
large for a dense matrix use the oracle's FFT product, which the host test ties to the dense matrix.

Per case: (a) three forced iterations from a non-zero start, both operators, with and without the Jacobi diagonal, one system and
a batch of three with a zero row, against the same loop on the dense matrix at 1e-12 (the bound between two of the project's own
solvers; the reference's own distance to the FFT product is 3e-15) -- the check that sees a wrong operator; (b) a solve converged
to 1e-8: iteration count within the project's rule, true residual under the dense A below 1.05 tol, distance to
numpy.linalg.solve at most cond(A) * 1.05 tol, per-row counts of a batch equal to cg_batched's.  The systems are conditioned so
that these counts are decided by the system and not by rounding (tests/_dense_toeplitz.py says how that was settled, on the CPU).
"""
import functools
import math

import pytest
import torch

import _cg_routes as R
import _dense_toeplitz as D

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(autouse=True)
def _serial_oracle():
    """One thread: the oracle's stopping point is the same on every host (tests/test_gpu_cg48_mixed.py)."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def _rel(a, b):
    a = a.detach().cpu().reshape(-1)
    b = b.detach().cpu().reshape(-1)
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def _count_rule(ito):
    return 0 if ito < 100 else 1 + ito // 200


@functools.lru_cache(maxsize=None)
def _operator(ns):
    from efgp_hip import ToeplitzOp
    return ToeplitzOp(D.system(ns, False)["v"].cuda())          # v depends on the block only, not on the Hermitian data


@functools.lru_cache(maxsize=2)
def _matrix(name, variant):
    """The reference operator of a case: (u -> A u for (M,) or (B, M), dense A or None).  Held for the case at hand only (the
    tests walk the cases one after the other): a dense matrix of M = 2048 and its transposed copy are 128 MB."""
    from oracle import efgp_oracle as O
    ns, herm, _ = R.CASES[name]
    s = D.system(ns, herm)
    if name in R.DENSE:
        A = D.system_A(ns, herm, variant)
        return D.matvec(A), A
    T = O.Toeplitz(s["v"])
    return (O.make_A_mean if variant == 0 else O.make_A_var)(s["ws"], T, s["sigmasq"]), None


@functools.lru_cache(maxsize=None)
def _forced_reference(name, variant, precond, batched, iters=3):
    from oracle import efgp_oracle as O
    ns, herm, _ = R.CASES[name]
    s = D.system(ns, herm)
    A, _ = _matrix(name, variant)
    diag = s["diag"] if precond else None
    if batched:
        return O.cg_batched(A, s["b"], s["x0"], 1e-30, max_iter=iters, early=False, diag=diag)[0]
    return O.cg_single(A, s["b"][0], s["x0"][0], 1e-30, max_iter=iters, early=False, diag=diag)[0]


@functools.lru_cache(maxsize=None)
def _converged_reference(name):
    """Variant 0 with the Jacobi diagonal from a zero start: (x, iterations) of cg_single on row 0, per-row counts and total of the batch."""
    from oracle import efgp_oracle as O
    ns, herm, _ = R.CASES[name]
    s = D.system(ns, herm)
    A, _ = _matrix(name, 0)
    zero = torch.zeros_like(s["b"])
    x1, it1 = O.cg_single(A, s["b"][0], zero[0], TOL, diag=s["diag"])
    rows = D.row_counts(A, s["b"], TOL, diag=s["diag"])
    return x1, it1, rows


def _solve(name, variant, b, x0, tol, **kw):
    from efgp_hip import cg_solve
    ns, herm, _ = R.CASES[name]
    s = D.system(ns, herm)
    return cg_solve(_operator(ns), s["ws"].cuda(), s["sigmasq"], variant, b.cuda(), None if x0 is None else x0.cuda(), tol,
                    hermitian=herm, **kw)


@pytest.mark.parametrize("name", list(R.CASES))
def test_operator_reports_the_restated_route(name):
    """What the operator can say about the route: its grids and whether it solves in one launch.  WHICH single-launch kernel runs
    (generic, line1d, 2d64, herm64, herm48) is not observable from the operator: the kernel names below are held to the Python
    restatement only, and the solves of the other tests are right on whichever kernel ran.  A moved bound in persistent_cg_launch
    shows here only where it changes a grid."""
    from efgp_hip import lib
    ns, herm, kernel = R.CASES[name]
    op = _operator(ns)
    assert R.route(ns, herm)[0] == kernel
    assert tuple(op.fft_shape) == R.fft_shape(ns) and op.ns == list(ns)
    assert tuple(op.cg_shape(hermitian=herm)) == R.cg_shape(ns, herm)
    assert tuple(op.cg_shape()) == R.cg_shape(ns, False)
    assert op.one_workgroup_per_system == R.one_workgroup_per_system(ns)
    assert bool(lib().efgp_toeplitz_single_launch_solves(op._h)) == R.single_launch_solves(ns)
    assert R.single_launch_solves(ns) == (kernel in ("generic", "line1d", "2d64", "herm64", "herm48"))


SMALL = [n for n in R.CASES if n in R.DENSE or n == "1d_2049"]


@pytest.mark.parametrize("precond", [True, False], ids=["jacobi", "plain"])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_three_forced_iterations_equal_the_dense_cg(name, variant, precond):
    ns, herm, _ = R.CASES[name]
    s = D.system(ns, herm)
    diag = s["diag"].cuda() if precond else None
    x1, it1, _ = _solve(name, variant, s["b"][0], s["x0"][0], 1e-30, max_iter=3, early_stop=False, diag=diag, batched=False)
    xb, itb, rows = _solve(name, variant, s["b"], s["x0"], 1e-30, max_iter=3, early_stop=False, diag=diag, batched=True)
    r1 = _forced_reference(name, variant, precond, False)
    rb = _forced_reference(name, variant, precond, True)
    e1, e0, e2 = _rel(x1, r1), _rel(xb[0], rb[0]), _rel(xb[2], rb[2])
    print(f"\n{name} variant {variant} precond {precond}: single {e1:.2e}, batch rows {e0:.2e} {e2:.2e}")
    assert it1 == 3 and itb == 3 and rows == [3, 3, 3]
    assert e1 < 1e-12 and e0 < 1e-12 and e2 < 1e-12
    assert float(xb[1].abs().max()) == 0.0                        # the zero row stays zero
    assert float(rb[1].abs().max()) == 0.0


@pytest.mark.parametrize("name", SMALL)
def test_converged_solve_against_the_direct_solve(name):
    ns, herm, _ = R.CASES[name]
    s = D.system(ns, herm)
    A, dense = _matrix(name, 0)
    xo, ito, rows_o = _converged_reference(name)
    b0 = s["b"][0]
    xg, itg, _ = _solve(name, 0, b0, None, TOL, diag=s["diag"].cuda(), batched=False)
    xg = xg.cpu()
    res = float(torch.linalg.norm(A(xg) - b0) / torch.linalg.norm(b0))
    print(f"\n{name}: iterations {itg} (oracle {ito}), true residual {res:.2e}, to the oracle's CG {_rel(xg, xo):.2e}")
    assert abs(itg - ito) <= _count_rule(ito), (itg, ito)
    assert res < 1.05 * TOL
    if dense is not None:
        kappa = D.cond(dense)
        err = _rel(xg, D.direct_solve(dense, b0))
        print(f"{name}: cond {kappa:.3g}, distance to the direct solve {err:.2e} (bound {kappa * 1.05 * TOL:.2e})")
        assert err <= kappa * 1.05 * TOL
    xb, itb, rows = _solve(name, 0, s["b"], None, TOL, diag=s["diag"].cuda(), batched=True)
    print(f"{name}: batch rows {rows} (oracle {rows_o}), total {itb}")
    assert rows == rows_o and rows[1] == 1
    assert itb == max(rows_o) + 1                                  # cg.py:243: the batched loop counts its terminating pass
    xb = xb.cpu()
    for r in (0, 2):
        assert float(torch.linalg.norm(A(xb[r]) - s["b"][r]) / torch.linalg.norm(s["b"][r])) < 1.05 * TOL
    assert float(xb[1].abs().max()) == 0.0


@pytest.mark.parametrize("precond", [True, False], ids=["jacobi", "plain"])
@pytest.mark.parametrize("ns", [(8, 64), (3, 7, 9), (256,)], ids=["8x64", "3x7x9", "256"])
def test_fused_mean_system_on_the_generic_kernel(ns, precond):
    """efgp_cg_solve_mean_async on non-cubic blocks of the generic kernel: b_times_ws, diag_scale and zero_x0 against the general
    entry with the materialised tensors, at the bounds of test_fused_mean_system_matches_general_solve, and the dense CG."""
    from efgp_hip import cg_solve, cg_solve_mean_async
    assert R.route(ns, True)[0] == "generic"
    s = D.system(ns, True)                                         # the entry's contract: fy of real data, ws real and even
    ws, fy, sig2 = s["ws"], s["b"][0], s["sigmasq"]
    op = _operator(ns)
    centre = op.v[tuple((L - 1) // 2 for L in op.v.shape)].real     # a view into v on the device
    res = cg_solve_mean_async(op, ws.cuda(), sig2, centre if precond else None, fy.cuda(), TOL)
    assert res is not None
    beta, lazy = res
    rhs = ws * fy
    diag = (float(centre) * ws.abs().pow(2).real + sig2) if precond else None
    xg, itg, _ = cg_solve(op, ws.cuda(), sig2, 0, rhs.cuda(), torch.zeros_like(rhs).cuda(), TOL,
                          diag=diag.cuda() if precond else None, batched=False)
    A = D.matvec(D.system_A(ns, True, 0))
    xo, ito = D.cg_dense(D.system_A(ns, True, 0), rhs, None, TOL, diag=diag)
    print(f"\n{ns} precond {precond}: iterations fused {int(lazy)} general {itg} dense {ito}; fused - general {_rel(beta, xg):.2e}, "
          f"fused - dense {_rel(beta, xo):.2e}")
    assert int(lazy) == itg and _rel(beta, xg) < 1e-13
    assert abs(int(lazy) - ito) <= _count_rule(ito) and _rel(beta, xo) < 1e-7
    assert float(torch.linalg.norm(A(beta.cpu()) - rhs) / torch.linalg.norm(rhs)) < 1.05 * TOL
    assert beta.shape == fy.shape


@pytest.mark.parametrize("name", R.LONG)
def test_long_solve_on_the_ill_conditioned_system(name):
    """One solve per route at sigma^2 = 4 (cond 1e2..3e2, 40 to several hundred iterations).  There the iteration count is not a
    property of the system (tests/_dense_toeplitz.py), so it is printed and only required to stay below the cap; the solution is
    judged on the true residual under the dense A (the oracle's FFT product beyond M = 2048) and the distance to the direct solve."""
    from efgp_hip import cg_solve
    from oracle import efgp_oracle as O
    ns, herm, kernel = R.CASES[name]
    assert R.route(ns, herm)[0] == kernel
    sig = D.LONG_SIGMASQ
    s = D.system(ns, herm, sigmasq=sig)
    b0 = s["b"][0]
    xg, itg, _ = cg_solve(_operator(ns), s["ws"].cuda(), sig, 0, b0.cuda(), None, TOL, diag=s["diag"].cuda(), batched=False, hermitian=herm)
    xg = xg.cpu()
    dense = D.system_A(ns, herm, 0, sig) if math.prod(ns) <= D.DENSE_MAX else None
    A = D.matvec(dense) if dense is not None else O.make_A_mean(s["ws"], O.Toeplitz(s["v"]), sig)
    res = float(torch.linalg.norm(A(xg) - b0) / torch.linalg.norm(b0))
    print(f"\n{name} ({kernel}) at sigma^2 = {sig}: {itg} iterations, true residual {res:.2e}")
    assert 1 < itg < 2 * math.prod(ns)
    assert res < 1.05 * TOL
    if dense is not None:
        kappa = D.cond(dense)
        err = _rel(xg, D.direct_solve(dense, b0))
        print(f"{name}: cond {kappa:.3g}, distance to the direct solve {err:.2e} (bound {kappa * 1.05 * TOL:.2e})")
        assert err <= kappa * 1.05 * TOL


LARGE = {"3d_17x19x33": ("EFGP_NO_CG_LINES", 1e-8), "3d_17x19x33_herm": ("EFGP_NO_CG_LINES", 1e-8),
         "3d_17x18x33_herm": ("EFGP_NO_CG_LINES", 1e-8), "2d_33x40": ("EFGP_NO_CG_COOP", 1e-12)}


@pytest.mark.parametrize("name", list(LARGE))
def test_line_and_cooperative_iterations_on_non_cubic_blocks(name, monkeypatch):
    """Twenty forced iterations of the 3-D line iteration (Hermitian and general; an even axis turns the Hermitian request into
    the general kernels) and of the cooperative 2-D solve with an even axis, against the same solve with the path switched off --
    at the bounds test_line_fft_iteration_3d (1e-8) and test_cooperative_solve_equals_multi_launch_iteration (1e-12) use -- and
    against the oracle's CG; then the true residual of a converged solve under efgp_toeplitz_apply."""
    hook, bound = LARGE[name]
    ns, herm, kernel = R.CASES[name]
    s = D.system(ns, herm)
    op = _operator(ns)
    assert R.route(ns, herm)[0] == kernel and R.route(ns, herm, env=(hook,))[0] in ("multi_fft", "multi_lines2")
    diag = s["diag"].cuda()
    runs = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv(hook, "1")
        runs[off] = (_solve(name, 0, s["b"], s["x0"], 1e-30, max_iter=20, early_stop=False, diag=diag, batched=True),
                     _solve(name, 1, s["b"][0], s["x0"][0], 1e-30, max_iter=20, early_stop=False, batched=False))
    monkeypatch.delenv(hook)
    (xb_on, itb_on, rows_on), (xb_off, itb_off, rows_off) = runs[False][0], runs[True][0]
    (x1_on, it1_on, _), (x1_off, it1_off, _) = runs[False][1], runs[True][1]
    ref1 = _forced_reference(name, 1, False, False, 20)            # the oracle's cg_single on its FFT product: A_var, no diagonal
    e = [_rel(xb_on[0], xb_off[0]), _rel(xb_on[2], xb_off[2]), _rel(x1_on, x1_off), _rel(x1_on, ref1)]
    print(f"\n{name}: path - hook: batch rows {e[0]:.2e} {e[1]:.2e}, A_var single {e[2]:.2e}; A_var single - oracle {e[3]:.2e}")
    assert itb_on == itb_off == 20 and rows_on == rows_off == [20, 20, 20] and it1_on == it1_off == 20
    assert max(e[:3]) < bound
    assert e[3] < 1e-8
    assert float(runs[False][0][0][1].abs().max()) == 0.0
    xg, itg, _ = _solve(name, 0, s["b"][0], None, TOL, diag=diag, batched=False)
    wsd, rhs = s["ws"].cuda(), s["b"][0].cuda()
    Ax = wsd * op.apply(wsd * xg) + s["sigmasq"] * xg
    res = float(torch.linalg.norm(Ax - rhs) / torch.linalg.norm(rhs))
    print(f"{name}: converged in {itg}, true residual under efgp_toeplitz_apply {res:.2e}")
    assert itg < 2 * math.prod(ns) and res < 1.05 * TOL
