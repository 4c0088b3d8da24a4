"""GPU: the five entries of csrc/pg_ops.hip against the references of tests/_pg_edges.py at the sizes where their grids end or wrap
(E-step, gradient, M-step: 1024 workgroups of 256, first wrap at 262145; weight rows: 512, first wrap at 131073), with the points
at which the per-point formulas change arm planted at fixed indices, and with non-finite inputs: a NaN stays a NaN, as in the
torch expressions of the reference.

Tolerances: per point 1e-14 relative to the restatement (zeros exact), the residual 4 eps, counts / bit patterns / refusals
exact, sums within their summation depth times 2^-53 times the sum of the magnitudes.  Every case prints what it measured.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _helper_seams as H
import _pg_edges as E
from _pgnb import gauss_hermite

pytestmark = pytest.mark.gpu

_F = torch.float64
EPS = float(np.finfo(np.float64).eps)
SEED = 24680
RHOS = (0.0, 0.7, 1.0)


def _dev():
    return torch.device("cuda", 0)


def _run_estep(case, rho, r=None, *, hash_seed=None):
    """One call of the entry on a case -> (mean, sigma_diag, delta, residual, metric) on the host."""
    from efgp_hip.ops import pg_estep_update, pg_nb_estep_update
    dev = _dev()
    S, y, delta = case["S"].to(dev), case["y"].to(dev), case["delta0"].to(dev)
    probes = None if hash_seed is not None else case["probes"].to(dev)
    seed = hash_seed or 0
    if r is None:
        pg_b = case["pg_b"].to(dev) if case["pg_b"] is not None else None
        mean, sd, resid, correct = pg_estep_update(S, delta, y, rho, probes=probes, seed=seed, pg_b=pg_b)
        return mean.cpu(), sd.cpu(), delta.cpu(), float(resid), int(correct)
    mean, sd, sc = pg_nb_estep_update(S, delta, y, r, rho, probes=probes, seed=seed)
    resid, abs_err = sc.tolist()
    return mean.cpu(), sd.cpu(), delta.cpu(), resid, abs_err


def _rel_per_point(got, ref):
    """max over the points of |got - ref| / |ref|; a zero of the reference must be a zero, a NaN a NaN, an inf the same inf."""
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)])
    zero = fin & (ref == 0)
    assert bool((got[zero] == 0).all())
    nz = fin & ~zero
    return float(((got[nz] - ref[nz]).abs() / ref[nz].abs()).max()) if bool(nz.any()) else 0.0


def _same_scalar(got, ref, tol):
    if math.isnan(ref) or math.isinf(ref):
        return (math.isnan(got) and math.isnan(ref)) or got == ref
    return abs(got - ref) <= tol * abs(ref)


def _check_estep(tag, case, rho, r, got, *, overflow=False):
    (m_ref, sd_ref, d_ref, r_ref, met_ref), terms = E.estep_reference(case, rho, r)
    mean, sd, delta, resid, metric = got
    N, J = case["S"].shape[1], case["probes"].shape[0]
    assert torch.equal(H.bits(mean), H.bits(case["S"][0]))
    e_sd, e_d = _rel_per_point(sd, sd_ref), _rel_per_point(delta, d_ref)
    line = f"\n{tag} N={N} J={J} rho={rho}: sigma_diag {e_sd:.1e} delta {e_d:.1e} residual {resid:.17g} vs {r_ref:.17g}"
    if r is None:
        print(line + f" count {metric} vs {met_ref}")
    else:
        exact, mag = E.fsum_terms(terms)
        bound = E.sum_depth(N) * E.U53 * mag
        err = abs(metric - exact) if math.isfinite(exact) else 0.0
        print(line + f" sum {metric:.17g} vs {exact:.17g}: |err| {err:.3e} bound {bound:.3e} ({err / bound if bound else 0:.3f})")
    assert e_sd <= 1e-14 and e_d <= 1e-14
    assert _same_scalar(resid, r_ref, 4 * EPS), (resid, r_ref)
    if rho == 0.0:
        keep = case["delta0"] >= 0
        assert torch.equal(H.bits(delta[keep]), H.bits(case["delta0"][keep]))
    if rho == 1.0 and math.isfinite(r_ref):
        assert resid == 0.0 and r_ref == 0.0
    if J == 0:
        assert bool((sd == 0).all()) and not bool(torch.signbit(sd).any())
    if r is None:
        assert metric == met_ref
    elif overflow:
        assert exact == math.inf and metric == math.inf
    elif math.isfinite(exact):
        assert math.isfinite(metric) and err <= bound, (metric, exact, bound)
    else:
        assert _same_scalar(metric, exact, 0.0), (metric, exact)
    return e_sd, e_d


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the E-step pass of both likelihoods
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.ESTEP_SIZES)
def test_bernoulli_estep_at_edge_sizes(N):
    for J in (0, 1, 2):
        kinds = E.estep_kinds("bernoulli", J)
        for rho in RHOS:
            for start in (range(0, len(kinds), N) if N < len(kinds) else [0]):   # a size below the table: every kind in its turn
                case = E.estep_case(N, J, "bernoulli", start=start)
                assert len(case["kinds"]) == min(N, len(kinds))
                _check_estep("bernoulli", case, rho, None, _run_estep(case, rho))


@pytest.mark.parametrize("r", E.NB_TOTAL_COUNTS)
@pytest.mark.parametrize("N", E.ESTEP_SIZES)
def test_negative_binomial_estep_at_edge_sizes(N, r):
    for J in (0, 1, 2):
        kinds = E.estep_kinds("negative_binomial", J)
        for rho in RHOS:
            for start in (range(0, len(kinds), N) if N < len(kinds) else [0]):
                case = E.estep_case(N, J, "negative_binomial", start=start)
                assert len(case["kinds"]) == min(N, len(kinds))
                _check_estep(f"negative binomial r={r}", case, rho, r, _run_estep(case, rho, r))


@pytest.mark.parametrize("N", [65, E.WRAP + 257])
def test_negative_binomial_mean_count_overflow_gives_inf(N):
    case = E.estep_case(N, 2, "negative_binomial", overflow=True)
    assert "m_710_mean_count_inf" in case["kinds"]
    _check_estep("negative binomial m=710", case, 0.7, 1.0, _run_estep(case, 0.7, 1.0), overflow=True)


@pytest.mark.parametrize("position", E.MAX_POSITIONS)
@pytest.mark.parametrize("likelihood", ["bernoulli", "negative_binomial"])
def test_residual_with_the_maximum_planted(likelihood, position):
    """The only large |delta - Lambda| at index 0, in the last lane of wave 3 of workgroup 0, in the last thread of the last
    workgroup, and in the wrapped tail."""
    N = E.WRAP + 257
    r = None if likelihood == "bernoulli" else 37.5
    case = E.estep_case(N, 2, likelihood, max_at=position)
    assert case["max_index"] == E.max_index(position, N)
    for rho in RHOS:
        got = _run_estep(case, rho, r)
        _check_estep(f"{likelihood} max at {position} ({case['max_index']})", case, rho, r, got)
        if rho < 1.0:
            assert got[3] > 1e11                                      # the planted point, not the runner-up


@pytest.mark.parametrize("hits", [True, False], ids=["all_hits", "no_hits"])
def test_hit_count_of_every_point_and_of_none(hits):
    N = E.WRAP + 257
    case = E.estep_case(N, 2, "bernoulli", all_hits=hits)
    got = _run_estep(case, 0.7)
    _check_estep("all hits" if hits else "no hits", case, 0.7, None, got)
    assert got[4] == (N if hits else 0)


@pytest.mark.parametrize("likelihood", ["bernoulli", "negative_binomial"])
def test_hash_probes_equal_pointer_probes_bit_for_bit(likelihood):
    """At a size that wraps: the hash index of the last points exceeds 2^18."""
    from efgp_hip.ops import rademacher_fill
    N, J = E.WRAP + 257, 2
    r = None if likelihood == "bernoulli" else 1.0
    probes = rademacher_fill(_dev(), SEED, J, N).cpu()
    assert [float(probes[j, n]) for j in (0, 1) for n in (0, N - 1)] == [H.rademacher(SEED, j, n) for j in (0, 1) for n in (0, N - 1)]
    case = E.estep_case(N, J, likelihood, probes=probes, with_b=False)
    ptr = _run_estep(case, 0.7, r)
    hsh = _run_estep(case, 0.7, r, hash_seed=SEED)
    _check_estep(f"{likelihood} hash probes", case, 0.7, r, hsh)
    for a, b in zip(ptr[:3], hsh[:3]):
        assert torch.equal(H.bits(a), H.bits(b))
    assert ptr[3] == hsh[3] and ptr[4] == hsh[4]


@pytest.mark.parametrize("likelihood", ["bernoulli", "negative_binomial"])
def test_small_call_after_a_large_one_reads_no_stale_partials(likelihood):
    """The finish kernel reads `blocks` partials of a reused scratch slot: 1 after 1024."""
    r = None if likelihood == "bernoulli" else 1.0
    small, large = E.estep_case(65, 2, likelihood), E.estep_case(E.WRAP + 257, 2, likelihood, max_at="wrapped_tail")
    large["delta0"][large["max_index"]] = 10.0 * E.MAX_DELTA0          # a stale maximum would win (workgroup 1 of the large call)
    first = _run_estep(small, 0.7, r)
    assert _run_estep(large, 0.7, r)[3] > 2.0 * first[3]
    again = _run_estep(small, 0.7, r)
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(H.bits(a), H.bits(b))
    assert first[3] == again[3] and first[4] == again[4]
    print(f"\n{likelihood}: residual {again[3]:.17g} metric {again[4]} after a 1024-workgroup call, as before it")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. non-finite inputs: a NaN stays a NaN
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("likelihood,what", [("bernoulli", w) for w in E.ESTEP_NONFINITE] +
                         [("negative_binomial", w) for w in E.NB_NONFINITE])
def test_estep_keeps_nonfinite_values_as_the_reference_does(likelihood, what):
    r = None if likelihood == "bernoulli" else 37.5
    base = E.nonfinite_base(likelihood)
    case, at = E.plant_nonfinite(base, what)
    clean = _run_estep(base, 0.7, r)
    _check_estep(f"{likelihood} clean", base, 0.7, r, clean)
    got = _run_estep(case, 0.7, r)
    _check_estep(f"{likelihood} {what}", case, 0.7, r, got)
    others = torch.ones(E.NONFINITE_N, dtype=torch.bool)
    others[at] = False
    for a, b in zip(clean[:3], got[:3]):                              # every other point keeps its bits
        assert torch.equal(H.bits(a[others]), H.bits(b[others]))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the total-count gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _grad(y, mean, sd, r, x, w):
    from efgp_hip.ops import pg_nb_total_count_grad
    dev = _dev()
    return pg_nb_total_count_grad(y.to(dev), mean.to(dev), sd.to(dev), r, x.to(dev), w.to(dev))


@pytest.mark.parametrize("Q", [1, 2, 128])
@pytest.mark.parametrize("N", [1, 257, E.WRAP + 1])
def test_total_count_grad_against_the_exact_sum(N, Q):
    x, w = gauss_hermite(Q)
    y, mean, sd, kinds = E.grad_case(N)
    assert N == 1 or (len(kinds) == 5 and bool((sd < 0).any()))
    for r in E.NB_TOTAL_COUNTS:
        exact, mag = E.grad_reference(y, mean, sd, r, x, w)
        got = _grad(y, mean, sd, r, x, w)
        bound = E.grad_depth(N, Q) * E.U53 * mag
        err = abs(float(got) - exact)
        print(f"\ntotal-count gradient N={N} Q={Q} r={r}: {float(got):.17g} vs {exact:.17g}, |err| {err:.3e} bound {bound:.3e} "
              f"({err / bound:.3f})")
        assert err <= bound
        assert torch.equal(H.bits(got), H.bits(_grad(y, mean, sd, r, x, w)))


@pytest.mark.parametrize("what", E.GRAD_NONFINITE)
def test_total_count_grad_keeps_nan(what):
    x, w = gauss_hermite(2)
    y, mean, sd, _ = E.grad_case(E.NONFINITE_N)
    nan = float("nan")
    if what in ("nan_sigma_diag", "all"):
        sd[E.NONFINITE_AT - (2 if what == "all" else 0)] = nan
    if what in ("nan_mean", "all"):
        mean[E.NONFINITE_AT - (1 if what == "all" else 0)] = nan
    if what in ("nan_y", "all"):
        y[E.NONFINITE_AT] = nan
    exact, _ = E.grad_reference(y, mean, sd, 1.0, x, w)
    got = float(_grad(y, mean, sd, 1.0, x, w))
    print(f"\ntotal-count gradient {what}: {got} vs {exact}")
    assert math.isnan(exact) and math.isnan(got)


def test_device_digamma_answers_nan_outside_its_domain():
    """psi is evaluated for x > 0 only: y + r = -3.5 and y = NaN give NaN (the estimators refuse such targets)."""
    x, w = gauss_hermite(1)
    one = torch.ones(1, dtype=_F)
    for yv in (-4.5, float("nan")):
        got = float(_grad(one * yv, one * -800.0, one * 0.0, 1.0, x, w))
        print(f"\ndigamma(y + r) for y = {yv}, r = 1: gradient {got}")
        assert math.isnan(got)
    assert math.isfinite(float(_grad(one * 3.0, one * -800.0, one * 0.0, 1.0, x, w)))


def _refused(entry, call, out):
    from efgp_hip.lib import EFGP_EINVAL, lib
    rc = call(lib())
    msg = lib().efgp_last_error().decode()
    assert rc == EFGP_EINVAL and rc != 0
    assert entry in msg, msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    return msg


@pytest.mark.parametrize("nnodes,total_count,word", [(129, 1.0, "nodes"), (2, 0.0, "total_count"), (2, -1.0, "total_count"),
                                                     (2, float("nan"), "total_count")])
def test_total_count_grad_refuses_what_it_cannot_hold(nnodes, total_count, word):
    """Refused on the host side of the entry point (nothing is launched): a non-zero code and a message naming the argument."""
    dev = _dev()
    buf = torch.zeros(256, dtype=_F, device=dev)
    out = torch.full((4,), -7.0, dtype=_F, device=dev)
    p = C.c_void_p(buf.data_ptr())
    msg = _refused("efgp_pg_nb_total_count_grad", lambda L: L.efgp_pg_nb_total_count_grad(dev.index, 4, p, p, p, total_count, nnodes, p, p,
                                                                                          C.c_void_p(out.data_ptr()), None), out)
    assert word in msg, msg


# ------------------------------------------------------------------------------------------------------------------------------
# 4. weight rows
# ------------------------------------------------------------------------------------------------------------------------------
def _weight_rows(omega, nrows, *, probes=None, seed=0):
    """efgp_pg_weight_rows into a buffer filled with -7 beforehand (a fresh torch.empty may be handed the block that held the
    expected product a moment ago, and an entry the kernel never wrote would then compare equal)."""
    from efgp_hip.lib import check, lib
    out = torch.full((nrows, omega.numel()), -7.0, dtype=_F, device=omega.device)
    check(lib().efgp_pg_weight_rows(omega.device.index, omega.numel(), nrows, C.c_void_p(probes.data_ptr()) if probes is not None else None,
                                    seed, C.c_void_p(omega.data_ptr()), C.c_void_p(out.data_ptr()), None), "efgp_pg_weight_rows")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nrows", [1, 3])
@pytest.mark.parametrize("N", [1, 257, 131072, 131073, 131072 + 257])
def test_weight_rows_at_edge_sizes(N, nrows):
    from efgp_hip.ops import rademacher_fill
    dev = _dev()
    assert E.WEIGHT_ROWS_BLOCKS * E.THREADS == 131072
    g = torch.Generator().manual_seed(4000 + N)
    omega = H.signed_wide(N, g, False)
    for k, v in enumerate((-0.0, float("inf"), float("nan"), 0.0, -float("inf"))[:N]):
        omega[N - 1 - k] = v                                           # in the wrapped tail when there is one
    omega = omega.to(dev)
    z = rademacher_fill(dev, SEED, nrows, N)
    want = H.bits(omega * z)
    assert torch.equal(H.bits(_weight_rows(omega, nrows, seed=SEED)), want)
    assert torch.equal(H.bits(_weight_rows(omega, nrows, probes=z)), want)
    host = torch.tensor([[H.rademacher(SEED, j, n) for n in (0, N - 1)] for j in range(nrows)], dtype=_F)
    assert torch.equal(z[:, [0, N - 1]].cpu(), host)
    print(f"\nweight rows N={N} rows={nrows}: bit-equal to omega * z, hash and pointer form")


def test_weight_rows_at_65535_rows_and_refused_beyond():
    from efgp_hip.ops import rademacher_fill
    dev = _dev()
    omega = torch.tensor([-0.0, 2.5, float("nan")], dtype=_F, device=dev)
    z = rademacher_fill(dev, SEED, H.GRID_ROWS, 3)
    assert torch.equal(H.bits(_weight_rows(omega, H.GRID_ROWS, seed=SEED)), H.bits(omega * z))
    assert float(z[H.GRID_ROWS - 1, 2]) == H.rademacher(SEED, H.GRID_ROWS - 1, 2)
    out = torch.full((4,), -7.0, dtype=_F, device=dev)
    _refused("efgp_pg_weight_rows", lambda L: L.efgp_pg_weight_rows(dev.index, 3, H.GRID_ROWS + 1, None, SEED, C.c_void_p(omega.data_ptr()),
                                                                    C.c_void_p(out.data_ptr()), None), out)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. M-step terms
# ------------------------------------------------------------------------------------------------------------------------------
_MSTEP = {}


def _mstep(M, J):
    """The case and its exact sums at P = 4, computed once; fewer hypers read the first columns."""
    if (M, J) not in _MSTEP:
        case = E.mstep_case(M, J)
        _MSTEP[(M, J)] = (case, E.mstep_reference(*case))
    return _MSTEP[(M, J)]


@pytest.mark.parametrize("J", [0, 1, 3])
@pytest.mark.parametrize("M", [1, 255, 257, E.WRAP + 5])
def test_mstep_terms_against_the_exact_sums(M, J):
    from efgp_hip.ops import pg_mstep_terms
    dev = _dev()
    (bx, bj, R, dp4), (t1, t2, grad, mag1, mag2) = _mstep(M, J)
    d1, d2 = E.mstep_depth(M, J)
    bxd = bx.to(dev)
    bjd, Rd = (bj.to(dev), R.to(dev)) if J else (None, None)
    for P in (1, 2, 3, 4):
        dp = dp4[:, :P].contiguous()
        out = pg_mstep_terms(bxd, bjd, Rd, dp.to(dev))
        dpc = torch.complex(dp, torch.full_like(dp, float("nan"))).contiguous()
        outc = pg_mstep_terms(bxd, bjd, Rd, dpc.to(dev))
        assert bool(torch.isfinite(out).all()) and torch.equal(H.bits(out), H.bits(outc))          # the imaginary parts are not read
        assert torch.equal(H.bits(out), H.bits(pg_mstep_terms(bxd, bjd, Rd, dp.to(dev))))
        o = out.tolist()
        worst = 0.0
        for p in range(P):
            b1, b2 = d1 * E.U53 * mag1[p], d2 * E.U53 * mag2[p]
            bg = 0.5 * (b1 + b2) + E.U53 * 0.5 * (mag1[p] + mag2[p])
            e1, e2, eg = abs(o[p] - t1[p]), abs(o[P + p] - t2[p]), abs(o[2 * P + p] - grad[p])
            worst = max(worst, e1 / b1, e2 / b2 if b2 else 0.0, eg / bg)
            assert e1 <= b1 and e2 <= b2 and eg <= bg, (p, o, t1, t2)
            if J == 0:
                assert o[P + p] == 0.0 and o[2 * P + p] == 0.5 * o[p]
        print(f"\nM-step terms M={M} J={J} P={P}: worst |err| / bound {worst:.3f} (depths {d1}, {d2})")


def test_mstep_terms_refuses_five_hypers():
    dev = _dev()
    buf = torch.zeros(256, dtype=_F, device=dev)
    out = torch.full((16,), -7.0, dtype=_F, device=dev)
    p = C.c_void_p(buf.data_ptr())
    _refused("efgp_pg_mstep_terms", lambda L: L.efgp_pg_mstep_terms(dev.index, 4, 1, 5, p, p, p, p, 0, C.c_void_p(out.data_ptr()), None), out)
