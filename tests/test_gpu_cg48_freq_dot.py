"""GPU checks of <p, A p> formed in the row-frequency domain in cg_herm48_kernel (csrc/cg_herm.hip, FREQ_DOT; round 7).

A single 48 x 48 Hermitian solve takes <p, A p> = sigma^2 <p, p> + <ws p, T ws p> from the numbers its per-frequency Toeplitz
products read and produce (Parseval along k1), one phase early, and runs an iteration on three workgroup barriers.  The iteration
it replaces (<p, A p> summed over the modes behind the row transforms D) stays selectable with EFGP_CG48_MODE_DOT=1 and is the
second opinion here, next to the oracle's cg.py restatement.  Rules as in tests/test_gpu_cg48_mixed.py: iteration counts within
1 + it // 200 (Jacobi) or 1 + it // 50 (none), solutions within 100 tol or 1e4 tol.  tests/test_cg48_freq_dot.py is the numpy
statement of the identity.

Shapes: mtot 23 (every group of three rows full), 21 / 13 (the last groups partly / wholly beyond h), 5, 3, 1 (a single mode).
"""
import functools

import pytest
import torch

from test_gpu_cg_hermitian import _herm, _rel, _system

pytestmark = pytest.mark.gpu

SHAPES = [23, 21, 13, 5, 3, 1]
SIG = 0.25
SWITCH = "EFGP_CG48_MODE_DOT"


@pytest.fixture(autouse=True)
def _serial_oracle():
    """One thread: the oracle's stopping point is the same on every host (tests/test_gpu_cg_hermitian.py)."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _case(mtot):
    v, T, ws, fy = _system(mtot, 17)
    centre = float(v[tuple((s - 1) // 2 for s in v.shape)].real)
    return v, T, ws, fy, centre


def _diag(ws, centre, variant):
    d = centre * ws.abs().pow(2).real
    return d + SIG if variant == 0 else d / SIG + 1.0


def _operator(ws, T, variant):
    from oracle import efgp_oracle as O
    return (O.make_A_mean if variant == 0 else O.make_A_var)(ws, T, SIG)


@functools.lru_cache(maxsize=None)
def _oracle_solve(mtot, precond, variant, tol, start_seed=None):
    from oracle import efgp_oracle as O
    v, T, ws, fy, centre = _case(mtot)
    rhs = ws * fy
    x0 = torch.zeros_like(rhs) if start_seed is None else _hermitian_start(mtot, start_seed)
    xo, ito = O.cg_single(_operator(ws, T, variant), rhs, x0, tol, diag=_diag(ws, centre, variant) if precond else None)
    return xo, ito


def _hermitian_start(mtot, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * _herm(torch.complex(torch.randn(mtot, mtot, generator=g, dtype=torch.float64),
                                     torch.randn(mtot, mtot, generator=g, dtype=torch.float64))).reshape(-1)


def _both_arms(monkeypatch, run):
    new = run()
    monkeypatch.setenv(SWITCH, "1")
    par = run()
    monkeypatch.delenv(SWITCH)
    return new, par


def _check(mtot, precond, tol, new, par, oracle):
    (x_new, it_new), (x_par, it_par), (xo, ito) = new, par, oracle
    step = 200 if precond else 50
    xtol = (100 if precond else 1e4) * tol
    print(f"\nmtot {mtot} precond {precond}: iterations frequency {it_new} modes {it_par} oracle {ito}; "
          f"frequency - modes {_rel(x_new, x_par):.2e}, frequency - oracle {_rel(x_new, xo):.2e}")
    assert abs(it_new - it_par) <= 1 + it_par // step, (it_new, it_par)
    assert abs(it_new - ito) <= 1 + ito // step, (it_new, ito)
    assert _rel(x_new, x_par) < xtol
    assert _rel(x_new, xo) < xtol


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", SHAPES)
def test_mean_solve_matches_mode_dot_and_oracle(mtot, precond, monkeypatch):
    """VARIANT 0 through the fit's entry: zero start, right-hand side and Jacobi diagonal formed in the kernel."""
    from efgp_hip import ToeplitzOp, cg_solve_mean_async
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    assert op.cg_shape(hermitian=True) == [48, 48]
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda") if precond else None

    def run():
        beta, lazy = cg_solve_mean_async(op, ws.cuda(), SIG, dscale, fy.cuda(), tol)
        return beta.cpu(), int(lazy)
    new, par = _both_arms(monkeypatch, run)
    _check(mtot, precond, tol, new, par, _oracle_solve(mtot, precond, 0, tol))
    bq = new[0].reshape(mtot, mtot)
    assert torch.equal(torch.flip(bq, dims=(0, 1)).conj()[: mtot // 2], bq[: mtot // 2])


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", SHAPES)
def test_variance_operator_matches_mode_dot_and_oracle(mtot, precond, monkeypatch):
    """VARIANT 1 (ws T ws / sigma^2 + 1): the Toeplitz part of <p, A p> is divided by sigma^2 instead."""
    from efgp_hip import ToeplitzOp, cg_solve
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    rhs = (ws * fy).cuda()
    diag = _diag(ws, centre, 1).cuda() if precond else None

    def run():
        x, it, _ = cg_solve(op, ws.cuda(), SIG, 1, rhs, None, tol, diag=diag, batched=False, hermitian=True)
        return x.cpu(), it
    new, par = _both_arms(monkeypatch, run)
    _check(mtot, precond, tol, new, par, _oracle_solve(mtot, precond, 1, tol))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", [23, 13])
def test_warm_start_from_a_conjugate_even_iterate(mtot, variant, monkeypatch):
    """The first application forms A x0 and drops its <x0, A x0>: nothing stale may be left in the slots the first iteration
    reads."""
    from efgp_hip import ToeplitzOp, cg_solve
    tol = 1e-8
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    rhs = (ws * fy).cuda()
    x0 = _hermitian_start(mtot, 5).cuda()
    diag = _diag(ws, centre, variant).cuda()

    def run():
        x, it, _ = cg_solve(op, ws.cuda(), SIG, variant, rhs, x0, tol, diag=diag, batched=False, hermitian=True)
        return x.cpu(), it
    new, par = _both_arms(monkeypatch, run)
    _check(mtot, True, tol, new, par, _oracle_solve(mtot, True, variant, tol, start_seed=5))


@pytest.mark.parametrize("mtot", [23, 13, 1])
def test_forced_iterations_and_history(mtot, monkeypatch):
    """50 iterations without the stopping test: both arms run all of them, and row 0's |r_i| / |b| of the first ten iterations
    agrees to 1e-10 relative (the two forms of <p, A p> differ by rounding only).  A single mode is solved by its first iteration
    up to the 1e-16 guards in the quotients: the history stands at what they leave (3e-12 |b| here), a difference of two numbers
    near 1, and the arms are held to a few ulp of those: 1e-15 |b|."""
    from efgp_hip import ToeplitzOp, cg_solve_mean_async, cg_residual_history
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda")

    def run():
        with cg_residual_history(op.dev, 64) as rec:
            beta, lazy = cg_solve_mean_async(op, ws.cuda(), SIG, dscale, fy.cuda(), 1e-300, max_iter=50, early_stop=False)
            it = int(lazy)
        return beta.cpu(), it, rec.values()[:10].clone().cpu()
    (x_new, it_new, h_new), (x_par, it_par, h_par) = _both_arms(monkeypatch, run)
    dev = float(((h_new - h_par).abs() / h_par).max())
    print(f"\nmtot {mtot}: iterations {it_new} / {it_par}; history of the first ten iterations differs by {dev:.2e} relative")
    assert it_new == 50 and it_par == 50
    assert bool(torch.isfinite(x_new.real).all()) and bool(torch.isfinite(x_new.imag).all())
    if mtot == 1:
        assert float((h_new - h_par).abs().max()) <= 1e-15
        assert _rel(x_new, x_par) < 1e-14
        return
    assert bool((h_par > 0).all())
    assert dev <= 1e-10


def test_batch_keeps_the_packed_column_kernel(monkeypatch):
    """Three systems: one workgroup each on the packed column transforms; the switch does not reach them (bitwise)."""
    from efgp_hip import ToeplitzOp, cg_solve
    mtot, B = 23, 3
    v, T, ws, b = _system(mtot, 11, rows=B)
    op = ToeplitzOp(v.cuda())

    def run():
        x, it, rows = cg_solve(op, ws.cuda(), 0.3, 0, b.cuda(), None, 1e-9, batched=True, hermitian=True)
        return x.cpu(), list(rows)
    (x_new, rows_new), (x_par, rows_par) = _both_arms(monkeypatch, run)
    assert rows_new == rows_par and min(rows_new) > 0
    assert torch.equal(x_new, x_par)


@pytest.mark.parametrize("switch", [False, True])
def test_refusal_of_a_right_hand_side_that_is_not_conjugate_even(switch, monkeypatch):
    from efgp_hip import ToeplitzOp, cg_solve_async
    mtot = 23
    v, T, ws, b, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    g = torch.Generator().manual_seed(1)
    bad = torch.complex(torch.randn(mtot * mtot, generator=g, dtype=torch.float64), torch.randn(mtot * mtot, generator=g, dtype=torch.float64))
    if switch:
        monkeypatch.setenv(SWITCH, "1")
    x, lazy = cg_solve_async(op, ws.cuda(), SIG, 0, bad.cuda(), torch.zeros_like(bad).cuda(), 1e-8, batched=False, hermitian=True)
    assert lazy.rows_tensor.tolist() == [-2]
    assert bool(torch.isnan(x.real).all())
