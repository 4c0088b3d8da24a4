"""GPU checks of the eight-wave 48 x 48 solve with paired-lag Toeplitz products (cg_herm48_pairs_kernel, csrc/cg_herm.hip;
round 9).

A single 48 x 48 Hermitian solve runs on 512 threads: the row lanes of waves 0-1 as before, the per-frequency Toeplitz products
on the 384 lanes of waves 2-7 from coefficient pairs S(k0, m) = c(k0 - m) + c(k0 + m), Q(k0, m) = c(k0 - m) - c(k0 + m), four
multiply-adds per (k0, m) instead of eight (tests/test_cg48_lag_pairs.py states the arithmetic in numpy).  The 256-thread kernel
with 25 resident lags stays selectable with EFGP_CG48_LAG_COEFFS=1 and is the second opinion here, next to the oracle's cg.py
restatement.  Rules as in tests/test_gpu_cg48_freq_dot.py: iteration counts within 1 + it // 200 (Jacobi) or 1 + it // 50 (none),
solutions within 100 tol or 1e4 tol.

Shapes: mtot 23 (every group full), 21 (the last one-row group beyond h), 13 (every one-row group and half of a two-row group
beyond h), 5, 3, 1 (a single mode).
"""
import math

import pytest
import torch

from test_gpu_cg_hermitian import _rel, _system
from test_gpu_cg48_freq_dot import _case, _diag, _hermitian_start, _oracle_solve

pytestmark = pytest.mark.gpu

SHAPES = [23, 21, 13, 5, 3, 1]
SIG = 0.25
SWITCH = "EFGP_CG48_LAG_COEFFS"


@pytest.fixture(autouse=True)
def _serial_oracle():
    """One thread: the oracle's stopping point is the same on every host (tests/test_gpu_cg_hermitian.py)."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


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
    print(f"\nmtot {mtot} precond {precond}: iterations pairs {it_new} 25 lags {it_par} oracle {ito}; "
          f"pairs - 25 lags {_rel(x_new, x_par):.2e}, pairs - oracle {_rel(x_new, xo):.2e}")
    assert abs(it_new - it_par) <= 1 + it_par // step, (it_new, it_par)
    assert abs(it_new - ito) <= 1 + ito // step, (it_new, ito)
    assert _rel(x_new, x_par) < xtol
    assert _rel(x_new, xo) < xtol


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", SHAPES)
def test_mean_solve_matches_lag_coeffs_and_oracle(mtot, precond, monkeypatch):
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
def test_variance_operator_matches_lag_coeffs_and_oracle(mtot, precond, monkeypatch):
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
    xq = new[0].reshape(mtot, mtot)
    assert torch.equal(torch.flip(xq, dims=(0, 1)).conj()[: mtot // 2], xq[: mtot // 2])


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", [23, 13])
def test_warm_start_from_a_conjugate_even_iterate(mtot, variant, monkeypatch):
    """The first application forms A x0 and drops its <x0, A x0>: every role runs that application's barriers, and nothing stale
    may be left in the slots the first iteration reads."""
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
    agrees to 1e-10 relative (the two forms of the product differ by rounding only).  A single mode: the m = 0 statements are the
    25-lag kernel's and every other coefficient is zero, so the arms are held to 1e-15 |b| as in tests/test_gpu_cg48_freq_dot.py
    (equal bits are expected and printed)."""
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
    print(f"\nmtot {mtot}: iterations {it_new} / {it_par}; history of the first ten iterations differs by {dev:.2e} relative; "
          f"solutions bitwise equal: {torch.equal(x_new, x_par)}")
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


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("mtot", [3, 23])
def test_refusal_of_weights_that_are_not_real(mtot, switch, monkeypatch):
    """One entry of ws with an imaginary part of 1e-3: the row lanes' sum over |Im ws|^2 and |ws[k] - ws[-k]|^2 is positive, and
    both arms refuse -- -2 iterations, every entry of the solution NaN.  The entry sits in a row k0 < 0, which no lane stores: the
    lane that holds its mirror finds it."""
    from efgp_hip import ToeplitzOp, cg_solve_mean_async
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    assert op.cg_shape(hermitian=True) == [48, 48]
    ws_bad = ws.clone()
    ws_bad[1] = ws_bad[1] + 1e-3j
    if switch:
        monkeypatch.setenv(SWITCH, "1")
    beta, lazy = cg_solve_mean_async(op, ws_bad.cuda(), SIG, None, fy.cuda(), 1e-8)
    assert lazy.rows_tensor.tolist() == [-2]
    assert bool(torch.isnan(beta.real).all()) and bool(torch.isnan(beta.imag).all())


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("mtot", [23, 13])
def test_fused_entry_is_bitwise_the_separate_kernels(mtot, switch, monkeypatch):
    """The fused mean solve and the separate launches run identical statements on either arm: ws, iteration count and solution
    agree bit for bit (tests/test_gpu_fused_mean_solve.py holds the default arm on more kernels)."""
    from efgp_hip import ToeplitzOp, cg_solve_mean_async, cg_solve_mean_fused
    from test_gpu_fused_mean_solve import _system as _fsystem, _weights
    if switch:
        monkeypatch.setenv(SWITCH, "1")
    v, fy = _fsystem(mtot, 5)
    vd, fyd = v.cuda(), fy.cuda()
    ell, var, h, sig = 0.2, 1.7, 0.37 / mtot, 0.2
    c0 = (2.0 * math.pi * ell ** 2) * var
    centre = vd[tuple((s - 1) // 2 for s in vd.shape)].real
    ws_ref = _weights(0, 0.0, c0, ell, var, h, mtot)
    op_f = ToeplitzOp(vd, defer_spectra=True)
    res = cg_solve_mean_fused(op_f, 0, 0.0, c0, ell, h, mtot, sig, centre, fyd, 1e-6)
    assert res is not None, "the fused entry declined a deferred 48 x 48 operator"
    beta_f, ws_f, it_f = res
    op_e = ToeplitzOp(vd)
    beta_e, it_e = cg_solve_mean_async(op_e, ws_ref, sig, centre, fyd, 1e-6)
    assert torch.equal(ws_f, ws_ref)
    assert int(it_f) == int(it_e) > 0
    assert torch.equal(beta_f, beta_e)
    g = torch.Generator().manual_seed(9)
    u = torch.complex(torch.randn(2, mtot * mtot, generator=g, dtype=torch.float64),
                      torch.randn(2, mtot * mtot, generator=g, dtype=torch.float64)).cuda()
    assert torch.equal(op_f.apply(u), op_e.apply(u))
