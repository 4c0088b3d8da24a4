"""Host side of the PG estimators' approximate predictive variances: the restated formulas of tests/_pg_variance.py against
themselves and against the reference's recorded values (tests/golden/variance_pg_*.npz, tools/gen_golden_pg_variance.py), the
goldens' shape, and the new symbol and keywords.  No GPU."""
import fnmatch
import inspect
import json
import os

import numpy as np
import pytest
import torch

import _pg_variance as V


# ---- barycentric weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 7, 16, 64])
def test_bary_matrix_is_one_hot_at_and_next_to_every_node(n):
    nodes, weights = V.cheb_axis(-0.7, 1.9, n)
    assert np.all(np.diff(nodes) > 0) and abs(nodes[0] + 0.7) < 1e-15 and abs(nodes[-1] - 1.9) < 1e-15
    eye = np.eye(n)
    for off in (0.0, 3e-15, -3e-15):
        assert np.array_equal(V.bary_matrix(nodes, weights, nodes + off), eye), off


@pytest.mark.parametrize("n", [2, 7, 64])
def test_bary_matrix_divides_just_outside_the_hit_radius(n):
    nodes, weights = V.cheb_axis(-0.7, 1.9, n)
    mat = V.bary_matrix(nodes, weights, nodes + 5e-14)
    assert not np.array_equal(mat, np.eye(n))
    assert np.all(np.abs(mat - np.eye(n)).max(axis=1) > 0)            # every row went through the division
    assert np.abs(mat - np.eye(n)).max() < 1e-9                       # and is the node's row to O(5e-14 / spacing)
    assert np.allclose(mat.sum(axis=1), 1.0, rtol=0, atol=1e-15 * n)


@pytest.mark.parametrize("shape", [(2,), (64,), (7, 7), (3, 64), (3, 5, 4), (16, 16, 16)])
def test_bary_matrix_reproduces_tensor_polynomials(shape):
    """A polynomial of degree n_a - 1 per axis is its own interpolant: 1e-13 of its maximum (float64 against extended precision
    differs by at most 4e-15 for d <= 3, n <= 64)."""
    rng = np.random.default_rng(5)
    d = len(shape)
    boxes = [(-1.0, 1.0), (0.3, 2.1), (-2.5, -0.5)][:d]
    axes = [V.cheb_axis(lo, hi, n) for (lo, hi), n in zip(boxes, shape)]
    # Chebyshev coefficients on the box's own coordinates keep the polynomial O(1) on the box
    coef = [rng.normal(size=n) for n in shape]

    def poly(points):
        out = np.ones(points.shape[0])
        for a, ((lo, hi), c) in enumerate(zip(boxes, coef)):
            out = out * np.polynomial.chebyshev.chebval((2.0 * points[:, a] - (lo + hi)) / (hi - lo), c)
        return out

    mesh = np.stack([g.reshape(-1) for g in np.meshgrid(*[a[0] for a in axes], indexing="ij")], axis=1)
    values = poly(mesh).reshape(shape)
    targets = np.stack([rng.uniform(lo, hi, 300) for lo, hi in boxes], axis=1)
    mats = [V.bary_matrix(ax[0], ax[1], targets[:, a]) for a, ax in enumerate(axes)]
    err = np.abs(V.interp_dense(values, mats) - poly(targets)).max()
    print(f"{shape}: max error {err:.2e} of max |p| {np.abs(values).max():.2e}")
    assert err <= 1e-13 * np.abs(values).max()


# ---- the dense stochastic variance against the reference's ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.CASES)
def test_stochastic_dense_matches_the_reference(case):
    """The restatement, fed the reference's fit (delta_, h, mtot, hyper-parameters) and its seeded probes, against the reference's
    `variance_stochastic`.  The reference's own solve stops at a relative residual cg_tol, which moves its solution by at most
    cond(A) cg_tol: bound cond(A) * 1.05 * cg_tol, relative to the largest value."""
    g, v = V.load_case(case)
    params = json.loads(str(g["params"]))
    cg_tol = params.get("cg_tol", 1e-6)
    X = torch.as_tensor(g["X"])
    d, mtot, h = X.shape[1], int(g["mtot"]), float(g["h"])
    ws = V.se_weights(float(g["lengthscale_"]), float(g["variance_"]), h, mtot, d)
    delta = torch.as_tensor(g["delta_"])
    A, cond = V.stochastic_operator(X, delta, ws, h, mtot)
    eta = V.reference_probes(int(v["n_probes"]), mtot ** d, int(v["random_state"]))
    dense = V.stochastic_dense(X, delta, ws, h, mtot, eta, torch.as_tensor(g["X_test"]), A=A).numpy()
    want = v["variance_stochastic"]
    err = float(np.abs(dense - want).max() / np.abs(want).max())
    print(f"{case}: M {mtot ** d} cond(A) {cond:.3e} max error {err:.2e} (bound {cond * 1.05 * cg_tol:.2e})")
    assert err <= cond * 1.05 * cg_tol


# ---- goldens, symbol, signatures -----------------------------------------------------------------------------------------------------
def test_variance_goldens_are_small_and_outside_the_fit_globs():
    names = sorted(f for f in os.listdir(V.GOLD) if f.startswith("variance_pg_"))
    assert names == sorted(f"variance_pg_{c}.npz" for c in V.CASES)
    for name in names:
        assert os.path.getsize(os.path.join(V.GOLD, name)) < 64 * 1024
        assert not fnmatch.fnmatch(name, "pg_*.npz") and not fnmatch.fnmatch(name, "pgnb_*.npz")
        z = np.load(os.path.join(V.GOLD, name))
        assert not {"X", "y"} & set(z.files)
        n = int(z["n_test"])
        assert z["variance_stochastic"].shape == z["variance_chebyshev"].shape == (n,)
        assert z["proba_stochastic"].shape == z["proba_chebyshev"].shape == (n, 2)
        assert float(z["delta_rel_to_fit_golden"]) <= 1e-12


def test_cheb_interp_is_declared_and_bound():
    from efgp_hip import declared_symbols
    from efgp_hip.lib import _SIGNATURES
    assert "efgp_cheb_interp" in declared_symbols()
    assert "efgp_cheb_interp" in _SIGNATURES


def test_prediction_methods_carry_the_variance_keyword():
    from polyagamma_classification import PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor
    for cls in (PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor):
        p = inspect.signature(cls.predictive_variance).parameters["method"]
        assert p.kind is p.KEYWORD_ONLY and p.default is None
        p = inspect.signature(cls.predict_response_mean).parameters["variance_method"]
        assert p.kind is p.KEYWORD_ONLY and p.default is None
        assert "last_variance_stats" in dir(cls)
    p = inspect.signature(PolyagammaGPClassifier.predict_proba).parameters["variance_method"]
    assert p.kind is p.KEYWORD_ONLY and p.default is None
    p = inspect.signature(PolyagammaGPNegativeBinomialRegressor.predict_mean_count).parameters["variance_method"]
    assert p.kind is p.KEYWORD_ONLY and p.default is None


def test_variance_keyword_is_checked_before_anything_else():
    from polyagamma_classification import PolyagammaGPClassifier
    with pytest.raises(ValueError, match="bogus.*'exact', 'stochastic', 'stochastic_diag_sums', 'chebyshev'"):
        PolyagammaGPClassifier().predictive_variance(np.zeros((2, 1)), method="bogus")


@pytest.mark.parametrize("method", ["stochastic", "stochastic_diag_sums", "chebyshev"])
def test_constructor_option_is_still_refused(method):
    from polyagamma_classification import PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor
    X = np.linspace(-1, 1, 20).reshape(-1, 1)
    with pytest.raises(NotImplementedError, match="predictive_variance_method"):
        PolyagammaGPClassifier(predictive_variance_method=method).fit(X, np.arange(20) % 2)
    with pytest.raises(NotImplementedError, match="predictive_variance_method"):
        PolyagammaGPNegativeBinomialRegressor(predictive_variance_method=method).fit(X, np.arange(20) % 3)
