"""GPU checks of the eight-wave 48 x 48 solve with <u, A u> and the step length on a dense wave (cg_herm48_pairs_kernel,
csrc/cg_herm.hip; round 12).

The default arm sums the 480 summands of <u, A u> and forms alpha = <r,z> / (<u, A u> + 1e-16) on one wave of the one-row dense role,
between barrier 2 and a new barrier "2b", while the row waves run D's transforms; the row lanes read the quotient behind that
barrier.  EFGP_CG48_ALPHA_ROWS=1 selects the statements of round 11: the row lanes sum and divide inside D.  Both arms run the same
functions on the same summands in the same tree (h48::uAu_summands, uAu_of_lane, quot_half_wave), so the solution, the iteration
count and the residual history are compared BIT FOR BIT, and on every comparison that reaches the kernel the two launches carry
different labels (a comparison of an arm with itself would pass every bitwise check).

What can go wrong and where it would show:
  * the dense wave's <r,z>: 0 in the application in front of the loop (warm starts), the sums in front of the loop in the first
    iteration, the sums behind barrier 3 afterwards -- cold and warm starts with caps 1, 2, 3;
  * the barrier count of the roles on every way through the kernel -- caps 1 to 3 (the cap in either half of the two-iteration
    body; max_iter 0 means the default cap to the library), "stop" after an odd and an even count, b = 0, the refusals; a mismatch
    would not return, so each of these is a case;
  * the VARIANT 1 division of the Toeplitz part by sigma^2 on the dense wave; the instantiation without a preconditioner;
  * blocks whose dead slots and dead rows put zeros among the summands: mtot 1, 3, 5, 13 beside 23.
The non-square block 23 x 5 does not reach the 48 x 48 kernels (they want a square block): its case pins that the switch changes
nothing on that route, label included.
"""
import math

import pytest
import torch

import _dense_toeplitz as D
from test_gpu_cg48_freq_dot import _case, _diag, _hermitian_start
from test_gpu_cg48_row_stream import CAP, _assert_equal_arms, _label, _mean_run, _same_bits, _solve_run

pytestmark = pytest.mark.gpu

SHAPES = [1, 3, 5, 13, 23]
SIG = 0.25
SWITCH = "EFGP_CG48_ALPHA_ROWS"
ROWS_MARK = "step length on the row waves"
OTHER = {"EFGP_CG48_ROW_V1": "row role of round 10", "EFGP_CG48_CHAIN_V1": "round 9"}


def _both_arms(monkeypatch, run, reaches=True):
    new = run()
    label_new = _label()
    monkeypatch.setenv(SWITCH, "1")
    par = run()
    label_par = _label()
    monkeypatch.delenv(SWITCH)
    if reaches:
        assert "eight waves" in label_new and ROWS_MARK not in label_new, label_new
        assert "eight waves" in label_par and ROWS_MARK in label_par, label_par
        assert label_new != label_par
        for mark in OTHER.values():
            assert mark not in label_new and mark not in label_par
    else:
        assert label_new == label_par, (label_new, label_par)
    return new, par


def _precond_run(op, ws, fy, centre, mtot, variant, precond, tol, x0=None, **kw):
    """precond: "scalar" (the mean entry forms the Jacobi diagonal from one number; VARIANT 0, zero start), "modes" (a diagonal
    array through cg_solve_async) or None."""
    if precond == "scalar":
        assert variant == 0 and x0 is None
        return _mean_run(op, ws.cuda(), torch.tensor(centre, dtype=torch.float64, device="cuda"), fy.cuda(), tol, **kw)
    diag = _diag(ws, centre, variant).cuda() if precond == "modes" else None
    return _solve_run(op, ws.cuda(), variant, (ws * fy).cuda(), None if x0 is None else x0.cuda(), tol, diag, **kw)


@pytest.mark.parametrize("precond,variant", [("scalar", 0), ("modes", 0), ("modes", 1), (None, 0), (None, 1)])
@pytest.mark.parametrize("mtot", SHAPES)
def test_cold_start_is_bitwise_the_row_sum_arm(mtot, precond, variant, monkeypatch):
    from efgp_hip import ToeplitzOp
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    assert op.cg_shape(hermitian=True) == [48, 48]
    run = _precond_run(op, ws, fy, centre, mtot, variant, precond, tol)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"cold start, mtot {mtot} variant {variant} precond {precond}", new, par)
    assert new[1] > 0 and bool(torch.isfinite(torch.view_as_real(new[0])).all())
    assert ("no diagonal" in _label()) == (precond is None)
    if mtot == 1:
        assert new[1] == 1                    # a single mode: the first step is exact


@pytest.mark.parametrize("precond", ["modes", None])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", [5, 23])
def test_warm_start_is_bitwise_the_row_sum_arm(mtot, variant, precond, monkeypatch):
    """The application in front of the loop: the dense wave divides 0 and the row lanes drop what they read."""
    from efgp_hip import ToeplitzOp
    tol = 1e-8 if precond else 1e-6
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    run = _precond_run(op, ws, fy, centre, mtot, variant, precond, tol, x0=_hermitian_start(mtot, 5))
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"warm start, mtot {mtot} variant {variant} precond {precond}", new, par)
    assert new[1] > 1


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("ns", [(23, 5)])
def test_a_non_square_block_does_not_see_the_switch(ns, warm, monkeypatch):
    from efgp_hip import ToeplitzOp
    s = D.system(ns, True)
    op = ToeplitzOp(s["v"].cuda())
    assert op.cg_shape(hermitian=True) != [48, 48]
    run = _solve_run(op, s["ws"].cuda(), 0, s["b"][0].cuda(), s["x0"][0].cuda() if warm else None, 1e-8, s["diag"].cuda(),
                     sig=s["sigmasq"])
    new, par = _both_arms(monkeypatch, run, reaches=False)
    _assert_equal_arms(f"block {ns} warm {warm}", new, par)
    assert new[1] > 1 and bool(torch.isfinite(torch.view_as_real(new[0])).all())


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("max_iter", [0, 1, 2, 3])
@pytest.mark.parametrize("mtot", [5, 23])
def test_caps_in_either_half_of_the_loop_body(mtot, max_iter, warm, monkeypatch):
    """No stopping test: the loop ends at the cap, in front of its second half (odd caps) or of its first (even caps).  max_iter 0 is
    the C ABI's "default cap" (toeplitz_cg.hpp: max_iter <= 0 -> 2 M), so a cap of zero iterations cannot be asked of the kernel
    through the library; the case runs the 2 M iterations that 0 stands for."""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    x0 = _hermitian_start(mtot, 5) if warm else None
    run = _precond_run(op, ws, fy, centre, mtot, 0, "modes" if warm else "scalar", 1e-300, x0=x0, max_iter=max_iter, early_stop=False)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"cap, mtot {mtot} max_iter {max_iter} warm {warm}", new, par)
    ran = max_iter if max_iter > 0 else 2 * mtot * mtot
    assert new[1] == ran
    h = new[2]
    assert bool((h[:min(ran, CAP)] >= 0).all()) and bool((h[:min(ran, 3)] > 0).all()) and bool((h[ran:] == 0).all())
    x_start = x0 if warm else torch.zeros(mtot * mtot, dtype=torch.complex128)
    assert not torch.equal(new[0], x_start)                    # the update that was owed at the cap has been paid


@pytest.mark.parametrize("precond", ["scalar", None])
def test_300_forced_iterations(precond, monkeypatch):
    from efgp_hip import ToeplitzOp
    mtot = 23
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    run = _precond_run(op, ws, fy, centre, mtot, 0, precond, 1e-300, max_iter=300, early_stop=False)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"300 forced iterations, precond {precond}", new, par)
    assert new[1] == 300
    assert bool(torch.isfinite(new[2]).all()) and bool(torch.isfinite(torch.view_as_real(new[0])).all())


@pytest.mark.parametrize("precond", ["scalar", None])
@pytest.mark.parametrize("parity", [0, 1])
def test_stop_exit_at_even_and_odd_counts(parity, precond, monkeypatch):
    """The stopping decision is read behind barrier 1 of the next application, in front of barriers 2 and 2b: in the second half of
    the loop body after an odd count, in the first after an even one.  The tolerance is put between two entries of the residual
    history, so that the solve stops at a chosen count of that parity."""
    from efgp_hip import ToeplitzOp
    mtot = 23
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    hist = _precond_run(op, ws, fy, centre, mtot, 0, precond, 1e-300, max_iter=40, early_stop=False)()[2]
    k = next(k for k in range(6, 40) if k % 2 == parity and float(hist[k - 1]) < float(hist[:k - 1].min()))
    tol = 0.5 * (float(hist[k - 1]) + float(hist[:k - 1].min()))
    new, par = _both_arms(monkeypatch, _precond_run(op, ws, fy, centre, mtot, 0, precond, tol))
    _assert_equal_arms(f"stop at {k} (parity {parity}) precond {precond}", new, par)
    assert new[1] == k


@pytest.mark.parametrize("mtot", [5, 23])
def test_zero_right_hand_side(mtot, monkeypatch):
    """<u, A u> = 0: the quotient is 0 / 1e-16 on both arms, and the solve stops behind barrier 1 of the second application."""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    new, par = _both_arms(monkeypatch, _precond_run(op, ws, torch.zeros_like(fy), centre, mtot, 0, "scalar", 1e-8))
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
    assert (ROWS_MARK in _label()) == switch and "eight waves" in _label()


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
    assert (ROWS_MARK in _label()) == switch and "eight waves" in _label()


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("other", sorted(OTHER))
def test_the_other_arms_do_not_see_the_switch(other, warm, monkeypatch):
    """EFGP_CG48_ROW_V1=1 and EFGP_CG48_CHAIN_V1=1 keep their statements and their labels whatever the new switch says; and the
    default arm equals them bit for bit (the summing wave against the row lanes of rounds 9 and 10)."""
    from efgp_hip import ToeplitzOp
    mtot = 23
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    run = _precond_run(op, ws, fy, centre, mtot, 0, "modes", 1e-8, x0=_hermitian_start(mtot, 5) if warm else None)
    default = run()
    assert OTHER[other] not in _label()
    monkeypatch.setenv(other, "1")
    alone = run()
    label_alone = _label()
    monkeypatch.setenv(SWITCH, "1")
    both = run()
    label_both = _label()
    monkeypatch.delenv(SWITCH)
    monkeypatch.delenv(other)
    assert label_alone == label_both and OTHER[other] in label_alone and ROWS_MARK not in label_both, (label_alone, label_both)
    _assert_equal_arms(f"{other} with and without {SWITCH}, warm {warm}", alone, both)
    _assert_equal_arms(f"default against {other}, warm {warm}", default, alone)


@pytest.mark.parametrize("mtot", [5, 23])
def test_fused_entry_is_bitwise_the_separate_kernels(mtot, monkeypatch):
    """On both arms the fused mean solve and the separate launches agree bit for bit in ws, iteration count and solution, and the
    arms agree with each other."""
    from efgp_hip import ToeplitzOp, cg_solve_mean_async, cg_solve_mean_fused
    from test_gpu_fused_mean_solve import _system as _fsystem, _weights
    v, fy = _fsystem(mtot, 5)
    vd, fyd = v.cuda(), fy.cuda()
    ell, var, h, sig = 0.2, 1.7, 0.37 / mtot, 0.2
    c0 = (2.0 * math.pi * ell ** 2) * var
    centre = vd[tuple((s - 1) // 2 for s in vd.shape)].real
    ws_ref = _weights(0, 0.0, c0, ell, var, h, mtot)
    got = {}
    for switch in (False, True):
        if switch:
            monkeypatch.setenv(SWITCH, "1")
        res = cg_solve_mean_fused(ToeplitzOp(vd, defer_spectra=True), 0, 0.0, c0, ell, h, mtot, sig, centre, fyd, 1e-6)
        assert res is not None, "the fused entry declined a deferred 48 x 48 operator"
        beta_f, ws_f, it_f = res
        label_f = _label()
        beta_e, it_e = cg_solve_mean_async(ToeplitzOp(vd), ws_ref, sig, centre, fyd, 1e-6)
        assert _same_bits(ws_f, ws_ref)
        assert int(it_f) == int(it_e) > 0
        assert _same_bits(beta_f, beta_e)
        assert label_f.startswith("fused mean solve") and "eight waves" in label_f and (ROWS_MARK in label_f) == switch, label_f
        assert (ROWS_MARK in _label()) == switch and "eight waves" in _label()
        got[switch] = (beta_f.cpu(), int(it_f))
    monkeypatch.delenv(SWITCH)
    assert got[False][1] == got[True][1]
    assert _same_bits(got[False][0], got[True][0])
