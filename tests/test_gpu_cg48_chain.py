"""GPU checks of the eight-wave 48 x 48 solve with the x update and the row lanes' loads off the iteration's dependent chain
(cg_herm48_pairs_kernel, csrc/cg_herm.hip; round 10).

The default arm runs x += alpha_k p_k between the barriers of application k + 1, where the row waves wait for the dense waves, and
loads b, the diagonal, x0 and ws at kernel entry.  EFGP_CG48_CHAIN_V1=1 selects the statements of round 9.  Every operation is the
same and in the same order on both arms, so the solution, the iteration count and the residual history are compared BIT FOR BIT
(NaNs included: the comparison is on the 64-bit patterns).  The entries are those of tests/test_gpu_cg48_lag_pairs.py.

Shapes: mtot 23 (every dense group full), 21, 13 (groups beyond h), 5, 3, 1 (a single mode: converges at iteration 1).
max_iter 1 and 2 without the stopping test leave the loop with an x update owed (by the cap; 2 also pays one inside the loop);
max_iter 0 is the entries' "no cap", 2 M forced iterations.  A system that converges at iteration 1 and b = 0 leave through the
"stop" exit behind barrier 1 with the update of iteration 1 owed.
"""
import math

import pytest
import torch

from test_gpu_cg48_freq_dot import _case, _diag, _hermitian_start

pytestmark = pytest.mark.gpu

SHAPES = [1, 3, 5, 13, 21, 23]
SIG = 0.25
SWITCH = "EFGP_CG48_CHAIN_V1"
CAP = 64


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    return t.view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _both_arms(monkeypatch, run):
    new = run()
    monkeypatch.setenv(SWITCH, "1")
    par = run()
    monkeypatch.delenv(SWITCH)
    return new, par


def _assert_equal_arms(what, new, par):
    (x_new, it_new, h_new), (x_par, it_par, h_par) = new, par
    print(f"\n{what}: iterations {it_new} / {it_par}; x bitwise {_same_bits(x_new, x_par)}; history bitwise {_same_bits(h_new, h_par)}")
    assert it_new == it_par, (it_new, it_par)
    assert _same_bits(h_new, h_par)
    assert _same_bits(x_new, x_par)


def _mean_run(op, ws, dscale, fy, tol, **kw):
    """VARIANT 0 through the fit's entry: zero start, right-hand side ws * fy and the Jacobi diagonal formed in the kernel."""
    from efgp_hip import cg_solve_mean_async, cg_residual_history

    def run():
        with cg_residual_history(op.dev, CAP) as rec:
            beta, lazy = cg_solve_mean_async(op, ws, SIG, dscale, fy, tol, **kw)
            it = lazy.rows_tensor.tolist()[0]
        return beta.cpu(), it, rec.values().clone()
    return run


def _solve_run(op, ws, variant, rhs, x0, tol, diag, **kw):
    """Either variant through cg_solve_async: explicit right-hand side, diagonal array and start vector."""
    from efgp_hip import cg_solve_async, cg_residual_history

    def run():
        with cg_residual_history(op.dev, CAP) as rec:
            x, lazy = cg_solve_async(op, ws, SIG, variant, rhs, None if x0 is None else x0.clone(), tol, diag=diag, batched=False,
                                     hermitian=True, **kw)
            it = lazy.rows_tensor.tolist()[0]
        return x.cpu(), it, rec.values().clone()
    return run


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", SHAPES)
def test_cold_start_is_bitwise_the_v1_arm(mtot, variant, precond, monkeypatch):
    from efgp_hip import ToeplitzOp
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    assert op.cg_shape(hermitian=True) == [48, 48]
    if variant == 0:
        dscale = torch.tensor(centre, dtype=torch.float64, device="cuda") if precond else None
        run = _mean_run(op, ws.cuda(), dscale, fy.cuda(), tol)
    else:
        diag = _diag(ws, centre, 1).cuda() if precond else None
        run = _solve_run(op, ws.cuda(), 1, (ws * fy).cuda(), None, tol, diag)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"cold start, mtot {mtot} variant {variant} precond {precond}", new, par)
    assert new[1] > 0 and bool(torch.isfinite(torch.view_as_real(new[0])).all())
    if mtot == 1:
        assert new[1] == 1                    # a single mode: the first step is exact


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", [13, 23])
def test_warm_start_is_bitwise_the_v1_arm(mtot, variant, precond, monkeypatch):
    """The first application forms A x0: x0, ws and the diagonal come from the loads at kernel entry, and nothing is owed to x
    when the loop starts."""
    from efgp_hip import ToeplitzOp
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    diag = _diag(ws, centre, variant).cuda() if precond else None
    run = _solve_run(op, ws.cuda(), variant, (ws * fy).cuda(), _hermitian_start(mtot, 5).cuda(), tol, diag)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"warm start, mtot {mtot} variant {variant} precond {precond}", new, par)
    assert new[1] > 1


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("max_iter", [0, 1, 2])
@pytest.mark.parametrize("mtot", [13, 23])
def test_forced_iterations_pay_the_owed_update(mtot, max_iter, warm, monkeypatch):
    """No stopping test: the loop ends at the cap.  max_iter 0 is "no cap" at the entries (2 M iterations)."""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    if warm:
        run = _solve_run(op, ws.cuda(), 0, (ws * fy).cuda(), _hermitian_start(mtot, 5).cuda(), 1e-300, _diag(ws, centre, 0).cuda(),
                         max_iter=max_iter, early_stop=False)
    else:
        dscale = torch.tensor(centre, dtype=torch.float64, device="cuda")
        run = _mean_run(op, ws.cuda(), dscale, fy.cuda(), 1e-300, max_iter=max_iter, early_stop=False)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"forced, mtot {mtot} max_iter {max_iter} warm {warm}", new, par)
    assert new[1] == (max_iter if max_iter > 0 else 2 * mtot * mtot)
    h = new[2]
    assert bool((h[: min(new[1], CAP)] > 0).all()) and bool((h[min(new[1], CAP):] == 0).all())
    if max_iter > 0:
        # x moved: the update that was owed at the cap has been paid (a cold start's x would still be zero, a warm start's x0)
        x_start = _hermitian_start(mtot, 5) if warm else torch.zeros(mtot * mtot, dtype=torch.complex128)
        assert not _same_bits(new[0], x_start)


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", [13, 23])
def test_convergence_at_iteration_one(mtot, precond, monkeypatch):
    """A Toeplitz vector of 1e-12 v: the operator is sigma^2 I + E with |E| <= 1e-12 max |ws|^2 sum |v|, the first step solves the
    system to the tolerance, and the loop is left through "stop" behind barrier 1 of the second application with the first
    update owed.  (The right-hand side keeps its size: the recurrences' absolute 1e-16 guards do not come into play.)"""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    scale = 1e-12
    op = ToeplitzOp((scale * v).cuda())
    dscale = torch.tensor(scale * centre, dtype=torch.float64, device="cuda") if precond else None
    new, par = _both_arms(monkeypatch, _mean_run(op, ws.cuda(), dscale, fy.cuda(), 1e-8))
    _assert_equal_arms(f"one iteration, mtot {mtot} precond {precond}", new, par)
    assert new[1] == 1
    # beta = ws fy / sigma^2 up to |E| / sigma^2 relative, and the update has been paid (a cold start's x would still be zero)
    want = (ws * fy) / SIG
    bound = 2.0 * scale * float(ws.abs().max()) ** 2 * float(v.abs().sum()) / SIG
    assert bound < 1e-6
    assert float(torch.linalg.norm(new[0] - want)) <= bound * float(torch.linalg.norm(want))


@pytest.mark.parametrize("mtot", [13, 23])
def test_zero_right_hand_side(mtot, monkeypatch):
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda")
    new, par = _both_arms(monkeypatch, _mean_run(op, ws.cuda(), dscale, torch.zeros_like(fy).cuda(), 1e-8))
    _assert_equal_arms(f"b = 0, mtot {mtot}", new, par)
    assert new[1] == 1
    assert bool((new[0] == 0).all())


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("mtot", [3, 23])
def test_refusal_of_weights_that_are_not_real(mtot, switch, monkeypatch):
    from efgp_hip import ToeplitzOp, cg_solve_mean_async
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    ws_bad = ws.clone()
    ws_bad[1] = ws_bad[1] + 1e-3j
    if switch:
        monkeypatch.setenv(SWITCH, "1")
    beta, lazy = cg_solve_mean_async(op, ws_bad.cuda(), SIG, None, fy.cuda(), 1e-8)
    assert lazy.rows_tensor.tolist() == [-2]
    assert bool(torch.isnan(beta.real).all()) and bool(torch.isnan(beta.imag).all())


@pytest.mark.parametrize("switch", [False, True])
@pytest.mark.parametrize("warm", [False, True])
def test_refusal_of_a_right_hand_side_that_is_not_conjugate_even(warm, switch, monkeypatch):
    from efgp_hip import ToeplitzOp, cg_solve_async
    mtot = 23
    v, T, ws, b, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    g = torch.Generator().manual_seed(1)
    bad = torch.complex(torch.randn(mtot * mtot, generator=g, dtype=torch.float64), torch.randn(mtot * mtot, generator=g, dtype=torch.float64))
    x0 = _hermitian_start(mtot, 5) if warm else torch.zeros_like(bad)
    if switch:
        monkeypatch.setenv(SWITCH, "1")
    x, lazy = cg_solve_async(op, ws.cuda(), SIG, 0, bad.cuda(), x0.cuda(), 1e-8, batched=False, hermitian=True)
    assert lazy.rows_tensor.tolist() == [-2]
    assert bool(torch.isnan(x.real).all()) and bool(torch.isnan(x.imag).all())


@pytest.mark.parametrize("mtot", [13, 23])
def test_fused_entry_is_bitwise_the_separate_kernels(mtot, monkeypatch):
    """Default arm: the fused mean solve (loads of b and of the diagonal's scalar at kernel entry, in front of the spectrum's
    prologue) and the separate launches agree bit for bit in ws, iteration count and solution; so does the fused solve of the
    V1 arm."""
    from efgp_hip import ToeplitzOp, cg_solve_mean_async, cg_solve_mean_fused
    from test_gpu_fused_mean_solve import _system as _fsystem, _weights
    v, fy = _fsystem(mtot, 5)
    vd, fyd = v.cuda(), fy.cuda()
    ell, var, h, sig = 0.2, 1.7, 0.37 / mtot, 0.2
    c0 = (2.0 * math.pi * ell ** 2) * var
    centre = vd[tuple((s - 1) // 2 for s in vd.shape)].real
    ws_ref = _weights(0, 0.0, c0, ell, var, h, mtot)
    res = cg_solve_mean_fused(ToeplitzOp(vd, defer_spectra=True), 0, 0.0, c0, ell, h, mtot, sig, centre, fyd, 1e-6)
    assert res is not None, "the fused entry declined a deferred 48 x 48 operator"
    beta_f, ws_f, it_f = res
    beta_e, it_e = cg_solve_mean_async(ToeplitzOp(vd), ws_ref, sig, centre, fyd, 1e-6)
    assert _same_bits(ws_f, ws_ref)
    assert int(it_f) == int(it_e) > 0
    assert _same_bits(beta_f, beta_e)
    monkeypatch.setenv(SWITCH, "1")
    beta_v, ws_v, it_v = cg_solve_mean_fused(ToeplitzOp(vd, defer_spectra=True), 0, 0.0, c0, ell, h, mtot, sig, centre, fyd, 1e-6)
    monkeypatch.delenv(SWITCH)
    assert int(it_v) == int(it_f)
    assert _same_bits(ws_v, ws_f) and _same_bits(beta_v, beta_f)
