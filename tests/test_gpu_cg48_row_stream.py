"""GPU checks of the eight-wave 48 x 48 solve with the shortened instruction stream of its row waves (cg_herm48_pairs_kernel,
csrc/cg_herm.hip; round 11).

The default arm runs two iterations per pass of the row role's loop with the direction alternating between two arrays (no copy of p
for the deferred x update, none at the back edge), has the preconditioner's choice as a template parameter (no branch and no phi
copies in the loop), interleaves the two wave sums, and leaves out the sixteen selects that zeroed A u in the slots without a mode:
those slots have ws = 0 and u = 0, and the four scratch entries per line that no stage writes are zeroed once, so that what the lanes
j >= 6 read there is finite.  EFGP_CG48_ROW_V1=1 selects the statements of round 10.  Every floating-point operation is the same
and in the same order on both arms, so the solution, the iteration count and the residual history are compared BIT FOR BIT (the
comparison is on the 64-bit patterns).  The entries are those of tests/test_gpu_cg48_chain.py.

Shapes: mtot 23 (every slot of the lanes j < 6 but one holds a mode), 21, 13, 5, 3, 1 (slots, lanes and whole rows without modes:
where a dead slot that did not stay zero would enter <r,r> and <r,z>).  The non-square blocks 23 x 5 and 5 x 23 do not reach the
48 x 48 kernels (they want a square block); the cases pin that the switch changes nothing on their route either.
Forced 1, 2, 3 and 200 iterations leave the two-iteration loop body in its first and in its second half with the x update owed from
either array; a system that converges at iteration 1 and b = 0 leave through the "stop" exit of the first half, and tolerances
chosen from the history leave through the "stop" exit at an even and at an odd count.
The entries take a start vector on the block only, so "garbage outside the block" is not admissible; the nearest case is a warm
start of 1e100 size on small blocks, where the slots without a mode multiply transform values of that size by their ws = 0.
"""
import math

import pytest
import torch

import _dense_toeplitz as D
from test_gpu_cg48_freq_dot import _case, _diag, _hermitian_start

pytestmark = pytest.mark.gpu

SHAPES = [1, 3, 5, 13, 21, 23]
SIG = 0.25
SWITCH = "EFGP_CG48_ROW_V1"
CAP = 256
V1_MARK = "row role of round 10"


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    return t.view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _label():
    from efgp_hip import lib
    return lib().efgp_cg_last_launch().decode()


def _both_arms(monkeypatch, run, reaches=True):
    """Both arms of one solve.  reaches: the solve runs the eight-wave 48 x 48 kernel, and the launch's label shows that the switch
    selected the other instantiation (a comparison of an arm with itself would pass every bitwise check)."""
    new = run()
    label_new = _label()
    monkeypatch.setenv(SWITCH, "1")
    par = run()
    label_par = _label()
    monkeypatch.delenv(SWITCH)
    if reaches:
        assert "eight waves" in label_new and V1_MARK not in label_new, label_new
        assert "eight waves" in label_par and V1_MARK in label_par, label_par
    else:
        assert label_new == label_par, (label_new, label_par)
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


def _solve_run(op, ws, variant, rhs, x0, tol, diag, sig=SIG, **kw):
    """Either variant through cg_solve_async: explicit right-hand side, diagonal array and start vector."""
    from efgp_hip import cg_solve_async, cg_residual_history

    def run():
        with cg_residual_history(op.dev, CAP) as rec:
            x, lazy = cg_solve_async(op, ws, sig, variant, rhs, None if x0 is None else x0.clone(), tol, diag=diag, batched=False,
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


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("ns", [(23, 5), (5, 23)])
def test_non_square_blocks_do_not_see_the_switch(ns, precond, warm, monkeypatch):
    from efgp_hip import ToeplitzOp
    s = D.system(ns, True)
    op = ToeplitzOp(s["v"].cuda())
    assert op.cg_shape(hermitian=True) != [48, 48]
    run = _solve_run(op, s["ws"].cuda(), 0, s["b"][0].cuda(), s["x0"][0].cuda() if warm else None, 1e-8,
                     s["diag"].cuda() if precond else None, sig=s["sigmasq"])
    new, par = _both_arms(monkeypatch, run, reaches=False)
    _assert_equal_arms(f"block {ns} precond {precond} warm {warm}", new, par)
    assert new[1] > 1 and bool(torch.isfinite(torch.view_as_real(new[0])).all())


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", [5, 13, 23])
def test_warm_start_is_bitwise_the_v1_arm(mtot, variant, precond, monkeypatch):
    """The first application forms A x0 in front of the loop; nothing is owed to x when the loop starts."""
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
@pytest.mark.parametrize("max_iter", [1, 2, 3, 200])
@pytest.mark.parametrize("mtot", [5, 23])
def test_forced_iterations_leave_either_half_of_the_loop_body(mtot, max_iter, warm, monkeypatch):
    """No stopping test: the loop ends at the cap, in front of its first half (even counts) or of its second (odd counts), and the x
    update that is owed comes from the array the last iteration ran along."""
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
    assert new[1] == max_iter
    h = new[2]
    assert bool((h[:max_iter] > 0).all()) and bool((h[max_iter:] == 0).all())
    x_start = _hermitian_start(mtot, 5) if warm else torch.zeros(mtot * mtot, dtype=torch.complex128)
    assert not _same_bits(new[0], x_start)                     # the update that was owed at the cap has been paid


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("parity", [0, 1])
def test_stop_exit_at_even_and_odd_counts(parity, precond, monkeypatch):
    """The stopping decision is read behind barrier 1 of the next application: in the second half of the loop body after an odd
    count, in the first after an even one.  The tolerance is put between two entries of the residual history, so that the solve stops
    at a chosen count of that parity."""
    from efgp_hip import ToeplitzOp
    mtot = 23
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda") if precond else None
    hist = _mean_run(op, ws.cuda(), dscale, fy.cuda(), 1e-300, max_iter=40, early_stop=False)()[2]
    # first count k >= 6 of the wanted parity whose residual lies below every earlier one: tol between entries k - 1 and k
    k = next(k for k in range(6, 40) if k % 2 == parity and float(hist[k - 1]) < float(hist[:k - 1].min()))
    tol = 0.5 * (float(hist[k - 1]) + float(hist[:k - 1].min()))
    new, par = _both_arms(monkeypatch, _mean_run(op, ws.cuda(), dscale, fy.cuda(), tol))
    _assert_equal_arms(f"stop at {k} (parity {parity}) precond {precond}", new, par)
    assert new[1] == k


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("mtot", [13, 23])
def test_convergence_at_iteration_one(mtot, precond, monkeypatch):
    """A Toeplitz vector of 1e-12 v: the first step solves the system to the tolerance, and the loop is left through "stop" behind
    barrier 1 of the second application with the first update owed (tests/test_gpu_cg48_chain.py has the bound)."""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    scale = 1e-12
    op = ToeplitzOp((scale * v).cuda())
    dscale = torch.tensor(scale * centre, dtype=torch.float64, device="cuda") if precond else None
    new, par = _both_arms(monkeypatch, _mean_run(op, ws.cuda(), dscale, fy.cuda(), 1e-8))
    _assert_equal_arms(f"one iteration, mtot {mtot} precond {precond}", new, par)
    assert new[1] == 1
    want = (ws * fy) / SIG
    bound = 2.0 * scale * float(ws.abs().max()) ** 2 * float(v.abs().sum()) / SIG
    assert bound < 1e-6
    assert float(torch.linalg.norm(new[0] - want)) <= bound * float(torch.linalg.norm(want))


@pytest.mark.parametrize("mtot", [5, 23])
def test_zero_right_hand_side(mtot, monkeypatch):
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda")
    new, par = _both_arms(monkeypatch, _mean_run(op, ws.cuda(), dscale, torch.zeros_like(fy).cuda(), 1e-8))
    _assert_equal_arms(f"b = 0, mtot {mtot}", new, par)
    assert new[1] == 1
    assert bool((new[0] == 0).all())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mtot", [1, 3, 5, 13])
def test_slots_without_a_mode_stay_zero_under_a_huge_start(mtot, variant, monkeypatch):
    """A start vector of size 1e100: the row transforms carry values of that size to every position of the 48-point lines, also to
    those beyond the block, where the slots without a mode multiply them by ws = 0.  A slot that did not stay zero (or a product
    that was not finite) would enter <r,r> and <r,z> of its wave: the history and x equal the switch arm's, which selects zeros."""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(mtot)
    op = ToeplitzOp(v.cuda())
    x0 = 1e101 * _hermitian_start(mtot, 7)
    run = _solve_run(op, ws.cuda(), variant, (ws * fy).cuda(), x0.cuda(), 1e-300, _diag(ws, centre, variant).cuda(), max_iter=3,
                     early_stop=False)
    new, par = _both_arms(monkeypatch, run)
    _assert_equal_arms(f"huge start, mtot {mtot} variant {variant}", new, par)
    assert new[1] == 3
    assert bool(torch.isfinite(new[2][:3]).all()) and bool(torch.isfinite(torch.view_as_real(new[0])).all())


@pytest.mark.parametrize("precond", [True, False])
def test_the_launch_label_names_the_arm(precond, monkeypatch):
    """The default arm has one instantiation with the Jacobi diagonal and one without; each switch selects its own."""
    from efgp_hip import ToeplitzOp
    v, T, ws, fy, centre = _case(13)
    op = ToeplitzOp(v.cuda())
    dscale = torch.tensor(centre, dtype=torch.float64, device="cuda") if precond else None
    run = _mean_run(op, ws.cuda(), dscale, fy.cuda(), 1e-8)
    labels = {}
    for env in (None, SWITCH, "EFGP_CG48_CHAIN_V1"):
        if env:
            monkeypatch.setenv(env, "1")
        run()
        labels[env] = _label()
        if env:
            monkeypatch.delenv(env)
    print(f"\n{labels}")
    assert len(set(labels.values())) == 3
    assert ("no diagonal" in labels[None]) == (not precond)
    assert V1_MARK in labels[SWITCH] and "round 9" in labels["EFGP_CG48_CHAIN_V1"]


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


@pytest.mark.parametrize("mtot", [5, 13, 23])
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
        beta_e, it_e = cg_solve_mean_async(ToeplitzOp(vd), ws_ref, sig, centre, fyd, 1e-6)
        assert _same_bits(ws_f, ws_ref)
        assert int(it_f) == int(it_e) > 0
        assert _same_bits(beta_f, beta_e)
        assert (V1_MARK in _label()) == switch and "eight waves" in _label()
        got[switch] = (beta_f.cpu(), int(it_f))
    monkeypatch.delenv(SWITCH)
    assert got[False][1] == got[True][1]
    assert _same_bits(got[False][0], got[True][0])
