"""Approximate predictive variances of the PG estimators on the MI355X: the interpolation kernel efgp_cheb_interp against the
dense barycentric formula, the stochastic route against its dense restatement, the Chebyshev route against its own node values
and the exact variance, both against the reference's recorded values (tests/golden/variance_pg_*.npz), and what must not have
moved.  Helpers and formulas: tests/_pg_variance.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _pg_sampling as P
import _pg_variance as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
NUFFT_EPS = 1e-7          # of the small estimators of _pg_sampling
CG_TOL = 1e-8

# ---- the kernel alone --------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [((2,), 1), ((64,), 257), ((7, 7), 257), ((3, 64), 1000), ((3, 5, 4), 257), ((16, 16, 16), 300)]
BOXES = [(-0.7, 1.9), (0.3, 2.1), (-2.5, -0.5)]
_KERNEL = {}


def kernel_case(shape, npts):
    """(axes, values (both signs), targets (npts, d), dense interpolant, Lebesgue sums), computed once per case."""
    key = (shape, npts)
    if key not in _KERNEL:
        d = len(shape)
        axes = [V.cheb_axis(lo, hi, n) for (lo, hi), n in zip(BOXES[:d], shape)]
        rng = np.random.default_rng(100 + sum(shape))
        values = rng.normal(size=shape) * 3.0
        if npts == 1:
            x = np.array([[0.123456789]])                              # one interior point of the 2-node axis
        else:
            x, n_fixed = V.kernel_points([a[0] for a in axes], 200 + sum(shape), npts)
            assert n_fixed <= npts
            x = x[-npts:]                                              # every special point, the rest uniform
        mats = [V.bary_matrix(ax[0], ax[1], x[:, a]) for a, ax in enumerate(axes)]
        _KERNEL[key] = (axes, values, x, V.interp_dense(values, mats), V.lebesgue(mats))
    return _KERNEL[key]


@pytest.mark.parametrize("shape,npts", KERNEL_CASES, ids=[f"{'x'.join(map(str, s))}-{n}" for s, n in KERNEL_CASES])
def test_cheb_interp_matches_the_dense_formula(shape, npts):
    from efgp_hip.ops import cheb_interp
    axes, values, x, dense, leb = kernel_case(shape, npts)
    assert x.shape == (npts, len(shape))
    if npts > 1:
        assert (dense < 0).any() and (dense > 0).any()              # the clamp has something to do
    nodes, weights = [a[0] for a in axes], [a[1] for a in axes]
    xd = torch.as_tensor(x).to(DEV)
    vd = torch.as_tensor(values).to(DEV)
    raw = cheb_interp(nodes, weights, vd, xd, clamp=False)
    clamped = cheb_interp(nodes, weights, vd, xd, clamp=True)
    assert raw.shape == (npts,) and raw.dtype == torch.float64 and raw.device.type == "cuda"
    tol = 1e-13 * np.abs(values).max()
    err = float(np.abs(raw.cpu().numpy() - dense).max())
    print(f"\n{shape} npts {npts}: max error {err:.2e} (tolerance {tol:.2e}), largest Lebesgue sum {leb.max():.2f}")
    assert err <= tol
    assert float(np.abs(clamped.cpu().numpy() - np.maximum(dense, 0.0)).max()) <= tol
    assert torch.equal(clamped, raw.clamp_min(0.0))
    # one thread per output, a fixed order of operations: a second call gives the same bits
    assert torch.equal(cheb_interp(nodes, weights, vd, xd, clamp=False), raw)


def test_cheb_interp_of_no_points_is_empty():
    from efgp_hip.ops import cheb_interp
    axes, values, _, _, _ = kernel_case((7, 7), 257)
    out = cheb_interp([a[0] for a in axes], [a[1] for a in axes], torch.as_tensor(values).to(DEV),
                      torch.empty((0, 2), dtype=torch.float64, device=DEV))
    assert out.shape == (0,) and out.dtype == torch.float64


@pytest.mark.parametrize("counts,dim,word", [((1,), 1, "n_nodes[0]"), ((65,), 1, "n_nodes[0]"), ((17, 17, 17), 3, "product of n_nodes"),
                                             ((2, 2, 2, 2), 4, "dim")], ids=["n1", "n65", "box17", "dim4"])
def test_cheb_interp_refuses_sizes_it_cannot_hold(counts, dim, word):
    """Refused on the host side of the entry point (nothing is launched): a non-zero code and a message naming the argument."""
    from efgp_hip.lib import EFGP_EINVAL, lib
    dev = torch.device(DEV, torch.cuda.current_device())
    buf = torch.zeros(8192, dtype=torch.float64, device=dev)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    p = C.c_void_p(buf.data_ptr())
    rc = lib().efgp_cheb_interp(dev.index, dim, (C.c_int64 * len(counts))(*counts), p, p, p, p, 4, 1, C.c_void_p(out.data_ptr()), None)
    msg = lib().efgp_last_error().decode()
    assert rc == EFGP_EINVAL and rc != 0
    assert "efgp_cheb_interp" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- stochastic route against the dense restatement -----------------------------------------------------------------------------------
_EST = {}


def estimator(case):
    if case not in _EST:
        _EST[case] = {"clf1d": lambda: P.small_classifier(1), "clf2d": lambda: P.small_classifier(2), "nb2d": P.small_nb_regressor}[case]()
    return _EST[case]


def query_points(d):
    if d == 2:
        return P.moment_points().numpy()
    g = torch.Generator().manual_seed(102)
    return (torch.rand(16, d, generator=g, dtype=torch.float64) * 2.4 - 1.2).numpy()


@pytest.mark.parametrize("case", ["clf1d", "clf2d", "nb2d"])
def test_stochastic_variance_matches_the_dense_restatement(case):
    est, X = estimator(case)
    xn = query_points(X.shape[1])
    est.set_params(predictive_variance_probes=16)
    est._variance_sums_cache = None                       # whatever an earlier test of this process left
    solves = len(est.last_fit_stats["solves"])
    got = est.predictive_variance(xn, method="stochastic")
    st = est.last_variance_stats
    assert st["method"] == "stochastic" and st["n_probes"] == 16 and st["seed"] == est.random_state + 2_000_000
    assert st["cached"] is False and 0 < st["cg_iters"] < 2000 and len(st["rows"]) == 16
    assert len(est.last_fit_stats["solves"]) == solves    # the fit's record is the fit's
    spec, dev = est._spec, est._dev
    xd = torch.as_tensor(X).to(dev)
    ws = spec.ws.reshape(-1).real
    A, cond = V.stochastic_operator(xd, est._delta, ws, spec.h, spec.mtot)
    eta = V.reference_probes(16, spec.M, est.random_state).to(dev)
    dense = V.stochastic_dense(xd, est._delta, ws, spec.h, spec.mtot, eta, torch.as_tensor(xn).to(dev), A=A).cpu().numpy()
    # a relative error of the operator / transforms (2 nufft_eps) and of the residual (1.05 cg_tol) moves the solution by at most
    # cond(A) times their sum (tests/test_gpu_pg_sampling.py); the evaluating type 2 adds its own 2 nufft_eps
    bound = cond * (2 * NUFFT_EPS + 1.05 * CG_TOL) + 2 * NUFFT_EPS
    err = float(np.abs(got - dense).max() / np.abs(dense).max())
    print(f"\n{case}: cond(A) {cond:.2e} error {err:.2e} bound {bound:.2e} cg_iters {st['cg_iters']}")
    assert got.shape == (16,) and got.dtype == np.float64 and (got >= 0).all()
    assert err <= bound
    # the alias, and the cache: no new solve, the same array
    again = est.predictive_variance(xn, method="stochastic_diag_sums")
    st2 = est.last_variance_stats
    assert st2["cached"] is True and st2["method"] == "stochastic" and st2["cg_iters"] == st["cg_iters"] and st2["rows"] == st["rows"]
    assert np.array_equal(again, got)
    # the response means go through the same variance
    mean = torch.as_tensor(est.decision_function(xn))
    want = est._response_mean(mean, torch.as_tensor(got)).numpy()
    assert np.allclose(est.predict_response_mean(xn, variance_method="stochastic"), want, rtol=1e-12, atol=0)
    # another probe count: a new solve and another estimate
    est.set_params(predictive_variance_probes=8)
    other = est.predictive_variance(xn, method="stochastic")
    st3 = est.last_variance_stats
    assert st3["cached"] is False and st3["n_probes"] == 8 and len(st3["rows"]) == 8
    assert not np.array_equal(other, got)
    est.set_params(predictive_variance_probes=0)
    with pytest.raises(ValueError, match="predictive_variance_probes"):
        est.predictive_variance(xn, method="stochastic")
    est.set_params(predictive_variance_probes=16)
    with pytest.raises(ValueError, match="bogus"):
        est.predictive_variance(xn, method="bogus")
    with pytest.raises(ValueError, match="bogus"):
        est.predict_response_mean(xn, variance_method="bogus")
    # empty and training inputs
    assert est.predictive_variance(np.empty((0, X.shape[1])), method="stochastic").shape == (0,)
    assert np.array_equal(est.predictive_variance(X, method="stochastic"), est.posterior_var_diag_)
    assert np.array_equal(est.predictive_variance(X, method="chebyshev"), est.posterior_var_diag_)


def test_refit_clears_the_cache_and_unseeded_probes_stay_until_then():
    est, X = P.small_classifier(1, random_state=None, max_iter=2)
    y = (np.sin(3.0 * X[:, 0]) > 0).astype(int)
    xn = query_points(1)
    torch.manual_seed(5)
    a = est.predictive_variance(xn, method="stochastic")
    first = est.last_variance_stats
    b = est.predictive_variance(xn, method="stochastic")
    assert first["cached"] is False and est.last_variance_stats["cached"] is True and est.last_variance_stats["seed"] == first["seed"]
    assert np.array_equal(a, b)
    est.fit(X, y)
    assert est._variance_sums_cache is None and est.last_variance_stats == {}
    c = est.predictive_variance(xn, method="stochastic")
    assert est.last_variance_stats["cached"] is False and est.last_variance_stats["seed"] != first["seed"]
    assert not np.array_equal(a, c)
    # a seeded estimator's cache goes with a refit too
    clf, Xs = estimator("clf1d")
    clf.predictive_variance(xn, method="stochastic")
    assert clf._variance_sums_cache is not None
    _EST.pop("clf1d")
    clf.fit(Xs, y)
    assert clf._variance_sums_cache is None
    clf.predictive_variance(xn, method="stochastic")
    assert clf.last_variance_stats["cached"] is False


# ---- Chebyshev route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["clf1d", "clf2d", "nb2d"])
def test_chebyshev_variance_is_the_interpolant_of_its_node_values(case):
    est, X = estimator(case)
    d = X.shape[1]
    xn = query_points(d)
    est.set_params(predictive_variance_chebyshev_nodes=7)
    got = est.predictive_variance(xn, method="chebyshev")
    st = est.last_variance_stats
    assert st["method"] == "chebyshev" and st["n_nodes_total"] == 7 ** d and len(st["nodes"]) == d
    assert st["node_values"].shape == (7,) * d
    for a in range(d):
        lo, hi = xn[:, a].min(), xn[:, a].max()
        want_nodes, _ = V.cheb_axis(lo, hi, 7)
        assert np.array_equal(st["nodes"][a], want_nodes)
    mats = [V.bary_matrix(st["nodes"][a], V.cheb_axis(0.0, 1.0, 7)[1], xn[:, a]) for a in range(d)]
    dense = np.maximum(V.interp_dense(st["node_values"], mats), 0.0)
    err = float(np.abs(got - dense).max())
    print(f"\n{case}: interpolation error {err:.2e} of max {np.abs(st['node_values']).max():.2e}")
    assert err <= 1e-13 * np.abs(st["node_values"]).max()
    # the node values are the exact variance at the node points, to twice the solves' own accuracy
    mesh = np.stack([g.reshape(-1) for g in np.meshgrid(*st["nodes"], indexing="ij")], axis=1)
    exact = est.predictive_variance(mesh)
    xd = torch.as_tensor(X).to(est._dev)
    _, cond = V.stochastic_operator(xd, est._delta, est._spec.ws.reshape(-1).real, est._spec.h, est._spec.mtot)
    nerr = V.rel(st["node_values"].reshape(-1), exact)
    print(f"{case}: node values against the exact variance {nerr:.2e} (bound {2 * cond * 1.05 * CG_TOL:.2e})")
    assert nerr <= 2 * cond * 1.05 * CG_TOL
    want = est._response_mean(torch.as_tensor(est.decision_function(xn)), torch.as_tensor(got)).numpy()
    assert np.allclose(est.predict_response_mean(xn, variance_method="chebyshev"), want, rtol=1e-12, atol=0)
    # a constant coordinate: the padded interval
    flat = xn.copy()
    flat[:, -1] = 0.25
    out = est.predictive_variance(flat, method="chebyshev")
    nd = est.last_variance_stats["nodes"][-1]
    assert np.isfinite(out).all() and (out >= 0).all()
    assert abs(nd[0] - (0.25 - 1e-6)) < 1e-15 and abs(nd[-1] - (0.25 + 1e-6)) < 1e-15
    for n in (1, 65):
        est.set_params(predictive_variance_chebyshev_nodes=n)
        with pytest.raises(ValueError, match="predictive_variance_chebyshev_nodes"):
            est.predictive_variance(xn, method="chebyshev")
    est.set_params(predictive_variance_chebyshev_nodes=7)
    assert est.predictive_variance(np.empty((0, d)), method="chebyshev").shape == (0,)


# ---- against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.CASES)
def test_approximate_variances_match_the_reference(case):
    """rel (2-norm) of both variances against the reference's at most 1e-5, the probabilities within 1e-6: the project's bounds
    for the exact variance against the same reference (tests/test_gpu_pg_classifier.py)."""
    g, v, clf = V.fit_golden(case)
    Xt = g["X_test"]
    clf.set_params(predictive_variance_probes=int(v["n_probes"]), predictive_variance_chebyshev_nodes=int(v["chebyshev_nodes"]))
    sto = clf.predictive_variance(Xt, method="stochastic")
    p_sto = clf.predict_proba(Xt, variance_method="stochastic")
    che = clf.predictive_variance(Xt, method="chebyshev")
    p_che = clf.predict_proba(Xt, variance_method="chebyshev")
    r_sto, r_che = V.rel(sto, v["variance_stochastic"]), V.rel(che, v["variance_chebyshev"])
    d_sto, d_che = float(np.abs(p_sto - v["proba_stochastic"]).max()), float(np.abs(p_che - v["proba_chebyshev"]).max())
    print(f"\n{case}: stochastic variance rel {r_sto:.2e} proba {d_sto:.2e}; chebyshev variance rel {r_che:.2e} proba {d_che:.2e}")
    assert r_sto <= 1e-5 and r_che <= 1e-5
    assert d_sto <= 1e-6 and d_che <= 1e-6


# ---- unchanged behaviour -------------------------------------------------------------------------------------------------------------------
def test_exact_keyword_and_default_are_todays_code():
    g, v, clf = V.fit_golden("se2d_n1000")
    Xt = g["X_test"]
    a = clf.predictive_variance(Xt)
    assert clf.last_variance_stats == {"method": "exact"}
    assert np.array_equal(a, clf.predictive_variance(Xt, method="exact"))
    assert np.array_equal(a, clf.predictive_variance(Xt, method=None))
    assert V.rel(a, g["predictive_variance"]) <= 1e-5
    proba = clf.predict_proba(Xt)
    assert np.array_equal(proba, clf.predict_proba(Xt, variance_method="exact"))
    assert float(np.abs(proba - g["predict_proba"]).max()) <= 1e-6


def test_constructor_option_is_still_refused_on_the_gpu():
    from polyagamma_classification import PolyagammaGPClassifier
    X = np.linspace(-1, 1, 40).reshape(-1, 1)
    with pytest.raises(NotImplementedError, match="predictive_variance_method"):
        PolyagammaGPClassifier(predictive_variance_method="stochastic", device="cuda").fit(X, np.arange(40) % 2)
