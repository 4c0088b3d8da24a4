"""GPU checks of the per-frequency Toeplitz application of cg_herm48_kernel (csrc/cg_herm.hip, DENSE; round 6).

A single 48 x 48 Hermitian solve applies the operator as row transforms plus, for every row frequency, a 23 x 23 Hermitian
Toeplitz product over k0 with coefficients resident in registers.  The application it replaces (packed column transforms on the
2-D spectrum) stays selectable with EFGP_CG48_FFT2D=1 and is the second opinion here, next to the oracle's cg.py restatement.
Batches (one workgroup per system) stay on the packed column transforms; their checks below pin that the entry still solves
them.  tests/test_cg48_mixed_operator.py is the numpy statement of the arithmetic.

Shapes: mtot 23 (every group of three rows full), 21 / 13 (the last groups partly / wholly beyond h), 5, 3, 1 (a single mode).
"""
import functools

import pytest
import torch

from test_gpu_cg_hermitian import _herm, _rel, _system

pytestmark = pytest.mark.gpu

SHAPES = [23, 21, 13, 5, 3, 1]
SIG = 0.25


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


@functools.lru_cache(maxsize=None)
def _oracle_solve(mtot, precond, tol):
    from oracle import efgp_oracle as O
    v, T, ws, fy, centre = _case(mtot)
    rhs = ws * fy
    diag = (centre * ws.abs().pow(2).real + SIG) if precond else None
    A = O.make_A_mean(ws, T, SIG)
    xo, ito = O.cg_single(A, rhs, torch.zeros_like(rhs), tol, diag=diag)
    true_o = float(torch.linalg.norm(A(xo) - rhs) / torch.linalg.norm(rhs))
    return xo, ito, true_o


def _hermitian_start(mtot, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * _herm(torch.complex(torch.randn(mtot, mtot, generator=g, dtype=torch.float64),
                                     torch.randn(mtot, mtot, generator=g, dtype=torch.float64))).reshape(-1)


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", SHAPES)
def test_solve_matches_parent_application_and_oracle(mtot, precond, monkeypatch):
    from efgp_hip import ToeplitzOp, cg_solve_mean_async
    from oracle import efgp_oracle as O
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    assert op.cg_shape(hermitian=True) == [48, 48]
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda") if precond else None
    beta, lazy = cg_solve_mean_async(op, ws.cuda(), SIG, dscale, fy.cuda(), tol)
    it_new = int(lazy)
    monkeypatch.setenv("EFGP_CG48_FFT2D", "1")
    beta_p, lazy_p = cg_solve_mean_async(op, ws.cuda(), SIG, dscale, fy.cuda(), tol)
    it_par = int(lazy_p)
    monkeypatch.delenv("EFGP_CG48_FFT2D")
    xo, ito, true_o = _oracle_solve(mtot, precond, tol)
    xtol = (100 if precond else 1e4) * tol
    print(f"\nmtot {mtot} precond {precond}: iterations new {it_new} parent {it_par} oracle {ito}; "
          f"new - parent {_rel(beta, beta_p):.2e}, new - oracle {_rel(beta, xo):.2e}")
    assert abs(it_new - it_par) <= 1 + it_par // (200 if precond else 50), (it_new, it_par)
    assert abs(it_new - ito) <= 1 + ito // (200 if precond else 50), (it_new, ito)
    assert _rel(beta, beta_p) < xtol
    assert _rel(beta, xo) < xtol
    rhs = ws * fy
    A = O.make_A_mean(ws, T, SIG)
    true_h = float(torch.linalg.norm(A(beta.cpu()) - rhs) / torch.linalg.norm(rhs))
    assert true_h < 1.05 * true_o + 0.1 * tol, (true_h, true_o)
    bq = beta.cpu().reshape(mtot, mtot)
    assert torch.equal(torch.flip(bq, dims=(0, 1)).conj()[: mtot // 2], bq[: mtot // 2])


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", SHAPES)
def test_three_forced_iterations_match_parent_application(mtot, precond, monkeypatch):
    """The operator alone: three iterations without the stopping test from a non-zero Hermitian start.  Both applications round
    the same recurrences, as the parent's 48 x 48 and 64 x 64 kernels do: the distance of those two on the same system is the
    yardstick (at most 100 x it)."""
    from efgp_hip import ToeplitzOp, cg_solve
    v, T, ws, b, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    x0 = _hermitian_start(mtot, 5)
    diag = (centre * ws.abs().pow(2).real + SIG).cuda() if precond else None

    def run():
        x, it, _ = cg_solve(op, ws.cuda(), SIG, 0, b.cuda(), x0.cuda(), 1e-8, max_iter=3, early_stop=False, diag=diag,
                            batched=False, hermitian=True)
        assert it == 3
        return x.cpu()
    x_new = run()
    monkeypatch.setenv("EFGP_CG48_FFT2D", "1")
    x_par = run()
    monkeypatch.setenv("EFGP_NO_CG48", "1")
    x_64 = run()
    monkeypatch.delenv("EFGP_NO_CG48")
    monkeypatch.delenv("EFGP_CG48_FFT2D")
    d_new, d_cal = _rel(x_new, x_par), _rel(x_par, x_64)
    print(f"\nmtot {mtot} precond {precond}: new - parent {d_new:.2e}; parent 48 x 48 - 64 x 64 {d_cal:.2e}")
    assert d_new <= 100 * d_cal, (d_new, d_cal)


@pytest.mark.parametrize("variant", [0, 1])
def test_batched_rows_warm_start(variant):
    from efgp_hip import ToeplitzOp, cg_solve
    mtot, B = 23, 9
    v, T, ws, b = _system(mtot, 11, rows=B)
    b = b * torch.logspace(-3, 2, B, dtype=torch.float64)[:, None]
    g = torch.Generator().manual_seed(5)
    x0 = 0.1 * _herm(torch.complex(torch.randn(B, mtot, mtot, generator=g, dtype=torch.float64),
                                   torch.randn(B, mtot, mtot, generator=g, dtype=torch.float64))).reshape(B, -1)
    op = ToeplitzOp(v.cuda())
    args = (op, ws.cuda(), 0.3, variant, b.cuda(), x0.cuda(), 1e-9)
    xh, ith, rows_h = cg_solve(*args, batched=True, hermitian=True)
    xc, itc, rows_c = cg_solve(*args, batched=True)
    assert all(abs(a - c) <= 1 + c // 100 for a, c in zip(rows_h, rows_c)), (rows_h, rows_c)
    assert len(set(rows_h)) >= 2
    for r in range(B):
        assert _rel(xh[r], xc[r]) < 1e-7


def test_refusal_of_non_conforming_input():
    from efgp_hip import ToeplitzOp, cg_solve_async, cg_solve_mean_async
    mtot = 23
    v, T, ws, b, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    g = torch.Generator().manual_seed(1)
    bad = torch.complex(torch.randn(mtot * mtot, generator=g, dtype=torch.float64), torch.randn(mtot * mtot, generator=g, dtype=torch.float64))
    x, lazy = cg_solve_async(op, ws.cuda(), SIG, 0, bad.cuda(), torch.zeros_like(bad).cuda(), 1e-8, batched=False, hermitian=True)
    assert lazy.rows_tensor.tolist() == [-2]
    assert bool(torch.isnan(x.real).all())
    ws_bad = ws.clone()
    ws_bad[5] = ws_bad[5] + 0.1                     # real, not even
    beta, lazy = cg_solve_mean_async(op, ws_bad.cuda(), SIG, None, b.cuda(), 1e-8)
    assert lazy.rows_tensor.tolist() == [-2]
    assert bool(torch.isnan(beta.real).all())


def test_long_run_odd_part_of_row_zero(monkeypatch):
    """row k0 = 0 stores the modes +k1 and -k1 both, and rounding lets a conjugate-odd part grow there.  1000 forced
    iterations on mtot 23: the new application must not make it worse than twice the parent application's value."""
    from efgp_hip import ToeplitzOp, cg_solve
    mtot = 23
    h = (mtot - 1) // 2
    v, T, ws, b, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    diag = (centre * ws.abs().pow(2).real + SIG).cuda()

    def odd_share():
        x, it, _ = cg_solve(op, ws.cuda(), SIG, 0, b.cuda(), None, 1e-8, max_iter=1000, early_stop=False, diag=diag, batched=False,
                            hermitian=True)
        assert it == 1000
        xq = x.cpu().reshape(mtot, mtot)
        row = xq[h]
        odd = 0.5 * (row - torch.flip(row, dims=(0,)).conj())
        return float(torch.linalg.norm(odd) / torch.linalg.norm(xq))
    new = odd_share()
    monkeypatch.setenv("EFGP_CG48_FFT2D", "1")
    par = odd_share()
    monkeypatch.delenv("EFGP_CG48_FFT2D")
    print(f"\nodd part of row k0 = 0 after 1000 iterations, relative to the solution: new {new:.3e}, parent {par:.3e}")
    assert new <= 2.0 * par, f"new {new:.3e}, parent {par:.3e}"
