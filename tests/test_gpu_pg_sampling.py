"""GPU checks of posterior function draws on the Polya-Gamma estimators: the type-1 transform of per-point scaled normals generated
inside the spreaders (efgp_nufft_type1_normal_scaled against efgp_normal_fill rows scaled in memory and against the exact sums),
and `sample_latent` / `sample_proba` / `sample_mean_count` against the dense restatement of tests/_pg_sampling.py.

Tolerances are those of tests/test_gpu_sampling.py.  All seeds are fixed; statistical bounds are five standard errors of the
estimator, derived from its sample count, so the outcome is deterministic."""
import math
import warnings

import numpy as np
import pytest
import torch

import _pg_sampling as P

pytestmark = pytest.mark.gpu

CG_TOL, NUFFT_EPS, NS = 1e-8, 1e-7, 5


def _rel(a, b):
    a = a.detach().cpu()
    b = b.detach().cpu()
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


def _points(N, d, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, d, generator=g, dtype=torch.float64) * (hi - lo) + lo


# ------------------------------------------------------------------------------------------------------------------------------
# fused scaled transform
# ------------------------------------------------------------------------------------------------------------------------------
def _check_scaled_transform(plan, plain, x, h, shape, T, tol, seed, off, s, tag, pairs_bitwise):
    """type1_normal_scaled against scaled materialised rows through `plain` (4 tol), the exact sums (2 tol), itself (bits), and
    with the row count T + 1 (row r does not depend on the row count)."""
    from efgp_hip import normal_fill
    from oracle import efgp_oracle as O
    N = x.shape[0]
    sd = s.cuda()
    FZ = plan.type1_normal_scaled(seed, T, shape, sd, index_offset=off)
    assert FZ.shape == (T,) + tuple(shape) and FZ.dtype == torch.complex128
    Z = normal_fill(sd.device, seed, T, N, index_offset=off)
    r_mem = _rel(FZ, plain.type1(sd * Z, shape).reshape(FZ.shape))
    exact = O.nudft_type1(x, h, (sd * Z).cpu(), shape).reshape(FZ.shape)
    r_exact = max(_rel(FZ[b], exact[b]) for b in range(T))
    print(f"{tag}: against memory rows {r_mem:.2e}, against exact sums {r_exact:.2e} (tol {tol:g})")
    assert r_mem < 4 * tol
    assert r_exact < 2 * tol
    assert torch.equal(FZ, plan.type1_normal_scaled(seed, T, shape, sd, index_offset=off))
    F0 = plan.type1_normal_scaled(seed, T, shape, sd)                            # offset 0: other draws
    assert _rel(F0, plain.type1(sd * normal_fill(sd.device, seed, T, N), shape).reshape(FZ.shape)) < 4 * tol
    assert _rel(F0, FZ) > 0.1
    F1 = plan.type1_normal_scaled(seed, T + 1, shape, sd, index_offset=off)
    for b in range(T):
        assert _rel(F1[b], FZ[b]) < 4 * tol
    if pairs_bitwise and T >= 2:                 # 2-D: every row of both calls rides in a pair grid (an odd count pads its last pair)
        assert torch.equal(F1[:T], FZ)
    return FZ


@pytest.mark.parametrize("tol", [1e-5, 1e-7])
@pytest.mark.parametrize("layout", [True, False])
@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_type1_normal_scaled_2d(T, layout, tol):
    """The configurations of test_type1_normal_2d (MFMA spreader of a layout plan, LDS spreader of a plain plan) with both scale
    vectors; with a scale of ones the entry agrees with type1_normal within 4 tol."""
    from efgp_hip import NufftPlan, PointSet
    N, h, nm = 50000, 0.31, 23
    x = _points(N, 2, 31 + T)
    xd = x.cuda()
    plan = NufftPlan(xd, h, tol, points=PointSet(xd)) if layout else NufftPlan(xd, h, tol)
    plain = NufftPlan(xd, h, tol)
    seed, off = 990 + T, 7
    for name, make in P.SCALES.items():
        _check_scaled_transform(plan, plain, x, h, (nm, nm), T, tol, seed, off, make(N, 5 + T), f"2-D T={T} layout={layout} {name}", True)
    ones = torch.ones(N, dtype=torch.float64, device="cuda")
    r_one = _rel(plan.type1_normal_scaled(seed, T, (nm, nm), ones, index_offset=off), plan.type1_normal(seed, T, (nm, nm), index_offset=off))
    print(f"2-D T={T} layout={layout}: scale of ones against type1_normal {r_one:.2e}")
    assert r_one < 4 * tol


@pytest.mark.parametrize("d,N,h,nm,T,tol", [
    (1, 30000, 0.2, 41, 3, 1e-7),                # 1-D, LDS spreader: one pair pass and a single-row pass
    (3, 20000, 0.3, 9, 3, 1e-5),                 # 3-D, fine grid in LDS
    (3, 40000, 0.12, 21, 4, 1e-5),               # 3-D, fine grid beyond LDS: tile-sorted spreader
    (3, 6000, 0.12, 21, 3, 1e-5),                # 3-D, beyond LDS with few points: global fixed-point atomics
    (2, 50000, 0.12, 71, 5, 1e-7),               # 2-D plain plan, fine grid beyond LDS
])
def test_type1_normal_scaled_other_spread_paths(d, N, h, nm, T, tol):
    """The configurations of test_type1_normal_other_spread_paths with both scale vectors and with a scale of ones."""
    from efgp_hip import NufftPlan
    x = _points(N, d, 5 + d)
    xd = x.cuda()
    plan = NufftPlan(xd, h, tol)
    shape = (nm,) * d
    seed, off = 31337, 11
    for name, make in P.SCALES.items():
        _check_scaled_transform(plan, plan, x, h, shape, T, tol, seed, off, make(N, 9 + d), f"{d}-D N={N} nm={nm} {name}", False)
    ones = torch.ones(N, dtype=torch.float64, device="cuda")
    assert _rel(plan.type1_normal_scaled(seed, T, shape, ones, index_offset=off), plan.type1_normal(seed, T, shape, index_offset=off)) < 4 * tol


def test_type1_normal_scaled_rows_numbered_across_calls_zero_scale_and_empty_plan():
    """normal_row_offset continues the row numbering in a second call; an all-zero scale and a plan without points return zeros;
    bad counts and a scale of the wrong length raise."""
    from efgp_hip import NufftPlan, PointSet, normal_row_offset
    N, h, nm, tol = 40000, 0.31, 23, 1e-7
    xd = _points(N, 2, 77).cuda()
    s = P.pg_like_scale(N, 3).cuda()
    for plan in (NufftPlan(xd, h, tol, points=PointSet(xd)), NufftPlan(xd, h, tol)):
        full = plan.type1_normal_scaled(5, 6, (nm, nm), s)
        tail = plan.type1_normal_scaled(5, 2, (nm, nm), s, index_offset=normal_row_offset(4))
        assert torch.equal(tail, full[4:6])
        zero = plan.type1_normal_scaled(5, 3, (nm, nm), torch.zeros_like(s))
        assert zero.shape == (3, nm, nm) and float(zero.abs().max()) == 0.0
        after = plan.type1_normal_scaled(5, 6, (nm, nm), s)                      # the zero scale left no state behind
        assert torch.equal(after, full)
    empty = NufftPlan(torch.zeros(0, 2, dtype=torch.float64, device="cuda"), h, tol)
    out = empty.type1_normal_scaled(5, 3, (nm, nm), torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert out.shape == (3, nm, nm) and float(out.abs().max()) == 0.0
    with pytest.raises(ValueError):
        plan.type1_normal_scaled(5, 0, (nm, nm), s)
    with pytest.raises(ValueError, match="scale"):
        plan.type1_normal_scaled(5, 2, (nm, nm), s[:-1])


def test_null_point_scale_is_refused_by_name():
    from efgp_hip import NufftPlan
    from efgp_hip.lib import lib
    from efgp_hip.ops import _i64, _ptr
    xd = _points(1000, 2, 1).cuda()
    plan = NufftPlan(xd, 0.31, 1e-7)
    out = torch.empty((2, 9, 9), dtype=torch.complex128, device="cuda")
    rc = lib().efgp_nufft_type1_normal_scaled(plan._h, 1, 0, 2, None, _i64((9, 9)), 0, _ptr(out), None)
    assert rc != 0
    assert b"point_scale" in lib().efgp_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# estimators, small and exact
# ------------------------------------------------------------------------------------------------------------------------------
def _estimator(case):
    if case == "clf1d":
        return P.small_classifier(1)
    if case == "clf2d":
        return P.small_classifier(2)
    return P.small_nb_regressor()


_FITTED = ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_")


def _snapshot(est):
    return ({a: getattr(est, a).copy() for a in _FITTED}, est._delta.clone(), est._beta_mean.clone(), est._spec, est._op_pred,
            {"solves": [dict(s) for s in est.last_fit_stats["solves"]]}, est.lengthscale_, est.variance_)


def _unchanged(est, snap):
    arrays, delta, beta, spec, op, stats, ell, var = snap
    return (all(np.array_equal(getattr(est, a), v) for a, v in arrays.items()) and torch.equal(est._delta, delta)
            and torch.equal(est._beta_mean, beta) and est._spec is spec and est._op_pred is op and est.last_fit_stats == stats
            and est.lengthscale_ == ell and est.variance_ == var)


@pytest.mark.parametrize("case", ["clf1d", "clf2d", "nb2d"])
def test_sample_latent_state_is_exact(case):
    from efgp_hip import normal_fill
    from efgpnd import _derive_seed
    est, X = _estimator(case)
    snap = _snapshot(est)
    d = X.shape[1]
    xn = _points(40, d, 9).numpy()
    seed = 20240607
    paths, state = est.sample_latent(xn, NS, seed=seed, cg_tolerance=CG_TOL, return_state=True)
    assert _unchanged(est, snap)                                                 # no refit, nothing fitted moved
    spec, dev = est._spec, est._dev
    N, M, ws = X.shape[0], spec.M, spec.ws.reshape(-1)
    assert isinstance(paths, np.ndarray) and paths.shape == (NS, 40) and paths.dtype == np.float64 and np.isfinite(paths).all()
    assert state["seed"] == seed and state["weights"].shape == (NS, M) and len(state["cg_iters"]) == NS
    # rhs = D F*(sqrt(delta) e1) + e2 from the materialised noise and the explicit feature matrix
    xd = torch.as_tensor(X).to(dev)
    F = P.feature_matrix(xd, spec.h, spec.mtot)
    e1 = normal_fill(dev, _derive_seed(seed, 1), NS, N)
    e2 = P.hermitian_rows(normal_fill(dev, _derive_seed(seed, 2), 2 * NS, M))
    rhs = P.sampler_rhs(F, ws, est._delta, e1, e2)
    Fn = P.feature_matrix(torch.as_tensor(xn).to(dev), spec.h, spec.mtot)
    exact = P.paths_from_weights(Fn, ws, state["weights"])
    res = P.apply_A(est, state["delta"])
    pt = torch.as_tensor(paths)
    for s in range(NS):
        r_rhs = _rel(state["rhs"][s], rhs[s])
        r_res = _rel(res[s], state["rhs"][s])
        r_path = _rel(pt[s], exact[s])
        print(f"{case} row {s}: rhs {r_rhs:.2e} residual {r_res:.2e} paths {r_path:.2e} iters {state['cg_iters'][s]}")
        assert r_rhs < 2 * NUFFT_EPS
        assert r_res <= 1.05 * CG_TOL
        assert r_path < 2 * NUFFT_EPS
        assert 0 < state["cg_iters"][s] < 2000
    assert torch.equal(state["weights"], ws.reshape(1, M) * est._beta_mean.reshape(1, M) + state["delta"])
    assert torch.equal(state["delta"].flip(1).conj(), state["delta"])            # conjugate-even bit for bit
    assert est.last_sample_stats["seed"] == seed and est.last_sample_stats["cg_iters"] == state["cg_iters"]
    assert state["cg_capped"] == [] and state["cg_max_iterations"] == 2000
    # against the dense solve of the same system: a relative error of the right-hand side (2 nufft_eps) and of the residual
    # (1.05 cg_tolerance) moves the solution by at most cond(A) times their sum
    A = P.operator_A(F, ws, est._delta)
    cond = float(torch.linalg.cond(A))
    u = torch.linalg.solve(A, rhs.T).T
    for s in range(NS):
        assert _rel(state["delta"][s], u[s]) < cond * (2 * NUFFT_EPS + 1.05 * CG_TOL)


@pytest.mark.parametrize("case", ["clf1d", "clf2d", "nb2d"])
def test_sample_latent_seeding(case, monkeypatch):
    import efgpnd
    est, X = _estimator(case)
    d = X.shape[1]
    xn = _points(40, d, 9).numpy()
    a = est.sample_latent(xn, NS, seed=11, cg_tolerance=CG_TOL)
    snap = _snapshot(est)
    assert np.array_equal(a, est.sample_latent(xn, NS, seed=11, cg_tolerance=CG_TOL))
    assert _unchanged(est, snap)
    assert not np.array_equal(a, est.sample_latent(xn, NS, seed=12, cg_tolerance=CG_TOL))
    torch.manual_seed(7)
    b = est.sample_latent(xn, NS, cg_tolerance=CG_TOL)
    seed_b = est.last_sample_stats["seed"]
    torch.manual_seed(7)
    assert np.array_equal(b, est.sample_latent(xn, NS, cg_tolerance=CG_TOL))
    assert est.last_sample_stats["seed"] == seed_b and 0 <= seed_b < 2 ** 63
    assert not np.array_equal(b, est.sample_latent(xn, NS, cg_tolerance=CG_TOL))     # the default generator moved on
    # rows are numbered across blocks: with blocks of 4 rows the first 3 rows of an 11-row call are the 3-row call
    big, sbig = est.sample_latent(xn, 11, seed=11, cg_tolerance=CG_TOL, return_state=True)
    monkeypatch.setitem(efgpnd._SAMPLE_BLOCK, d, 4)
    cut, scut = est.sample_latent(xn, 11, seed=11, cg_tolerance=CG_TOL, return_state=True)
    assert est.last_sample_stats["blocks"] == 3
    a3 = est.sample_latent(xn, 3, seed=11, cg_tolerance=CG_TOL)
    for s in range(11):
        assert _rel(scut["rhs"][s], sbig["rhs"][s]) < 4 * NUFFT_EPS
        assert _rel(torch.as_tensor(cut[s]), torch.as_tensor(big[s])) < 4 * NUFFT_EPS + 2 * CG_TOL
    for s in range(3):
        assert _rel(torch.as_tensor(a3[s]), torch.as_tensor(big[s])) < 4 * NUFFT_EPS + 2 * CG_TOL
    for s in range(NS):
        assert _rel(torch.as_tensor(a[s]), torch.as_tensor(big[s])) < 4 * NUFFT_EPS + 2 * CG_TOL


def test_sample_latent_refusals_on_a_fitted_estimator():
    est, X = P.small_classifier(2)
    with pytest.raises(ValueError, match="n_samples"):
        est.sample_latent(X[:5], 0)
    with pytest.raises(ValueError, match="shape"):
        est.sample_latent(X[:5, :1], 2)
    with pytest.raises(ValueError, match="shape"):
        est.sample_proba(X[:5, :1], 2)


# ------------------------------------------------------------------------------------------------------------------------------
# estimators, statistical
# ------------------------------------------------------------------------------------------------------------------------------
def test_latent_draws_have_the_posterior_moments():
    est, X = P.small_classifier(2, cg_tol=1e-6)
    ns = 2048
    xn = P.moment_points()
    xn_np = xn.numpy()
    dev, spec = est._dev, est._spec
    mean = torch.as_tensor(est.decision_function(xn_np))
    v = torch.as_tensor(est.predictive_variance(xn_np))
    paths = torch.as_tensor(est.sample_latent(xn_np, ns, seed=1))
    assert est.last_sample_stats["blocks"] == ns // 64 and est.last_sample_stats["cg_capped"] == []
    ws = spec.ws.reshape(-1)
    F = P.feature_matrix(torch.as_tensor(X).to(dev), spec.h, spec.mtot)
    C = P.latent_cov(F, P.feature_matrix(xn.to(dev), spec.h, spec.mtot), ws, torch.as_tensor(est.delta_).to(dev)).cpu()
    print("dense diagonal against predictive_variance:", float((C.diagonal() - v).abs().max()), "of", float(v.max()))
    assert float((C.diagonal() - v).abs().max()) < 1e-3 * float(v.max())         # the exact variance is this diagonal
    sm, sv = paths.mean(0), paths.var(0, unbiased=True)
    dm = (sm - mean).abs()
    print("posterior mean deviation / s.e.:", [round(float(t), 2) for t in dm / (v / ns).sqrt()])
    print("posterior variance deviation / s.e.:", [round(float(t), 2) for t in (sv / v - 1) / math.sqrt(2 / (ns - 1))])
    assert bool((dm <= 5 * (v / ns).sqrt() + 2 * NUFFT_EPS * mean.abs().max()).all())
    assert bool(((sv / v - 1).abs() <= 5 * math.sqrt(2 / (ns - 1))).all())
    d = paths - sm
    for i, j in ((0, 1), (2, 3)):
        assert float((xn[i] - xn[j]).norm()) < min(0.3, est.lengthscale_)
        c = float(C[i, j])
        sc = float((d[:, i] * d[:, j]).sum() / (ns - 1))
        se = math.sqrt((c * c + float(v[i] * v[j])) / ns)
        print(f"pair ({i},{j}): correlation {c / math.sqrt(float(v[i] * v[j])):.3f} deviation {abs(sc - c) / se:.2f} s.e.")
        assert abs(sc - c) <= 5 * se
    assert bool(((xn.abs() > 1.0).any(1)).any())                                 # some points lie outside the data's box


def test_response_draws_are_pointwise_maps_of_the_latent_draws():
    clf, X = P.small_classifier(2)
    xn = P.moment_points().numpy()
    f = clf.sample_latent(xn, 7, seed=5)
    p = clf.sample_proba(xn, 7, seed=5)
    assert p.shape == (7, 16) and p.dtype == np.float64
    assert np.array_equal(p, torch.sigmoid(torch.as_tensor(f)).numpy())
    assert ((p > 0) & (p < 1)).all()
    reg, Xr = P.small_nb_regressor()
    fr = reg.sample_latent(xn, 7, seed=5)
    mc = reg.sample_mean_count(xn, 7, seed=5)
    assert mc.shape == (7, 16) and mc.dtype == np.float64
    assert np.array_equal(mc, (reg.total_count_ * torch.exp(torch.as_tensor(fr))).numpy())
    assert reg.total_count_ == 3.0 and (mc > 0).all()


def test_capped_latent_solves_are_reported():
    """Rows that reach max_cg_iterations are listed in last_sample_stats and in the state, and return_state=True warns."""
    est, X = P.small_classifier(2)
    xn = P.moment_points().numpy()
    _, ok = est.sample_latent(xn, NS, seed=20240607, cg_tolerance=CG_TOL, return_state=True)
    need = min(ok["cg_iters"])
    assert ok["cg_capped"] == [] and need > 12, ok["cg_iters"]
    cap = 3                                                                      # far below what every row needs
    est.sample_latent(xn, NS, seed=20240607, cg_tolerance=CG_TOL, max_cg_iterations=cap)
    stats = est.last_sample_stats
    assert stats["cg_max_iterations"] == cap and stats["cg_capped"] == list(range(NS)) and all(v >= cap for v in stats["cg_iters"])
    with pytest.warns(RuntimeWarning, match="max_cg_iterations"):
        _, state = est.sample_latent(xn, NS, seed=20240607, cg_tolerance=CG_TOL, max_cg_iterations=cap, return_state=True)
    assert state["cg_capped"] == list(range(NS)) and state["cg_max_iterations"] == cap
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        est.sample_latent(xn, NS, seed=20240607, cg_tolerance=CG_TOL, return_state=True)     # default cap: no warning


# ------------------------------------------------------------------------------------------------------------------------------
# full size
# ------------------------------------------------------------------------------------------------------------------------------
def test_sample_latent_at_full_size():
    """N = 1e6, 2-D classifier, device probes (random_state=None), two outer iterations, then 8 draws at 128 points.  The noise
    right-hand sides excite every mode, so their solves are bounded by CG's worst case sqrt(cond) ln(2 / tol) / 2 with
    cond <= 1 + max(ws^2) sum(delta); the counts are printed next to that bound."""
    from polyagamma_classification import PolyagammaGPClassifier
    gen = torch.Generator().manual_seed(4)
    N = 10 ** 6
    x = torch.rand(N, 2, dtype=torch.float64, generator=gen) * 2 - 1
    f = 2.0 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.5 * x[:, 1]) + 0.8 * x[:, 1]
    y = (torch.rand(N, dtype=torch.float64, generator=gen) < torch.sigmoid(2.0 * f)).to(torch.int64).numpy()
    torch.manual_seed(0)
    clf = PolyagammaGPClassifier(max_iter=2, device="cuda").fit(x.numpy(), y)
    idx = torch.randint(0, N, (128,), generator=torch.Generator().manual_seed(5))
    xn = x[idx].numpy()
    cap = 2000
    paths, state = clf.sample_latent(xn, 8, seed=99, return_state=True)
    assert paths.shape == (8, 128) and np.isfinite(paths).all()
    ws2 = float((clf._spec.ws.abs() ** 2).max())
    cond = 1.0 + ws2 * float(clf._delta.sum())
    bound = P.cg_iteration_bound(cond, clf.cg_tol)
    print(f"full size: mtot {clf._spec.mtot} cond <= {cond:.4g} bound {bound:.0f} cg_iters {state['cg_iters']}")
    assert all(0 < it < cap for it in state["cg_iters"])
    assert state["cg_capped"] == [] and state["cg_max_iterations"] == cap
    assert torch.equal(state["delta"].flip(1).conj(), state["delta"])
    res = P.apply_A(clf, state["delta"])
    for s in range(8):
        assert _rel(res[s], state["rhs"][s]) <= 1.05 * clf.cg_tol
