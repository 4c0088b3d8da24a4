"""Polya-Gamma negative-binomial regressor, host side (no GPU): import surface without scikit-learn, constructor defaults against
the reference's, refusals before any device work, the helpers and the torch restatements of the r gradient against the
reference's recorded values, the new C-ABI entries, and the goldens themselves."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _pgnb import expected_log_sigmoid_negative_gaussian, gauss_hermite, total_count_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gp-quadrature_amd")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pgnb_*.npz")))
HISTORY_KEYS = ["iter", "lengthscale", "variance", "grad_lengthscale", "grad_variance", "e_residual", "e_cg_iters", "m_cg_iters",
                "total_count", "grad_total_count", "total_count_updated", "mean_count_mae"]


def _xy(n=40, d=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, d))
    y = rng.integers(0, 20, n)
    return X, y


def test_regressor_imports_without_sklearn():
    """Both import forms work in a process where scikit-learn cannot be imported at all."""
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name == 'sklearn' or name.startswith('sklearn.'):\n"
            "            raise ImportError('sklearn blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            f"sys.path.insert(0, {PKG!r})\n"
            "from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor, negative_binomial_gaussian_mean\n"
            f"sys.path.insert(0, {os.path.join(PKG, 'polyagamma_classification')!r})\n"
            "from pg_classifier import PolyagammaGPNegativeBinomialRegressor as R2, negative_binomial_gaussian_mean as m2\n"
            "assert 'sklearn' not in sys.modules\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def test_constructor_defaults_match_the_reference():
    from polyagamma_classification import PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor
    ref = json.loads(str(np.load(GOLDEN[0])["default_params"]))
    reg = PolyagammaGPNegativeBinomialRegressor()
    assert reg.get_params() == ref
    # every classifier keyword, with the classifier's default
    clf = PolyagammaGPClassifier().get_params()
    assert {k: v for k, v in reg.get_params().items() if k in clf} == clf
    assert reg.set_params(total_count=2.5, learn_total_count=True).get_params()["total_count"] == 2.5
    assert reg.learn_total_count is True
    with pytest.raises(ValueError):
        reg.set_params(no_such_option=1)
    with pytest.raises(TypeError):
        PolyagammaGPNegativeBinomialRegressor(2.0)                              # keyword-only


@pytest.mark.parametrize("y_fn,kwargs,exc,match", [
    (lambda y: y - 30, {}, ValueError, "Negative binomial targets must be nonnegative."),
    (lambda y: y + 0.5, {}, ValueError, "Negative binomial targets must be integer-valued."),
    (lambda y: y.astype(float) * np.nan, {}, ValueError, "integer-valued"),
    (None, {"total_count": 0.0}, ValueError, "total_count must be positive."),
    (None, {"total_count": -1.0}, ValueError, "total_count must be positive."),
    (None, {"total_count_update_frequency": 0}, ValueError, "total_count_update_frequency must be positive."),
    (None, {"total_count_quadrature_nodes": 0}, ValueError, "total_count_quadrature_nodes must be positive."),
    (None, {"total_count_quadrature_nodes": 129, "learn_total_count": True}, ValueError, "at most 128"),
    (None, {"kernel": "matern"}, ValueError, "kernel"),
    (None, {"dtype": "float32"}, ValueError, "float32"),
    (None, {"dtype": torch.float32}, ValueError, "float32"),
    (None, {"predictive_variance_method": "chebyshev"}, NotImplementedError, "chebyshev"),
    (None, {"predictive_variance_method": "stochastic"}, NotImplementedError, "stochastic"),
    (None, {"device": "cpu"}, ValueError, "cpu"),
])
def test_refusals_come_before_any_device_work(y_fn, kwargs, exc, match):
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    X, y = _xy()
    if y_fn is not None:
        y = y_fn(y)
    with pytest.raises(exc, match=match):
        PolyagammaGPNegativeBinomialRegressor(max_iter=1, **kwargs).fit(X, y)


def test_unfitted_prediction_is_an_error():
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    with pytest.raises(RuntimeError, match="not fitted"):
        PolyagammaGPNegativeBinomialRegressor().predict(np.zeros((2, 2)))


def test_score_is_r2():
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    reg = PolyagammaGPNegativeBinomialRegressor()
    y = np.array([0.0, 3.0, 1.0, 7.0, 2.0])
    pred = np.array([0.5, 2.0, 1.5, 6.0, 2.5])
    reg.predict = lambda X: pred
    expected = 1.0 - np.sum((y - pred) ** 2) / np.sum((y - y.mean()) ** 2)
    assert reg.score(None, y) == pytest.approx(expected, rel=1e-15)
    reg.predict = lambda X: np.full(3, 2.0)
    assert reg.score(None, np.full(3, 2.0)) == 1.0 and reg.score(None, np.full(3, 1.0)) == 0.0


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_helpers_match_the_reference(path):
    from polyagamma_classification import _gauss_hermite_normal_rule, negative_binomial_gaussian_mean
    g = np.load(path)
    m, v = torch.from_numpy(g["helper_nb_mean_in"]), torch.from_numpy(g["helper_nb_var_in"])
    got = negative_binomial_gaussian_mean(m, v, total_count=float(g["helper_nb_total_count"])).numpy()
    np.testing.assert_allclose(got, g["helper_nb_mean"], rtol=1e-15, atol=0)
    for q in (12, 16, 64):
        x, w = _gauss_hermite_normal_rule(q)
        assert np.array_equal(x, g[f"helper_gh{q}_nodes"]) and np.array_equal(w, g[f"helper_gh{q}_weights"]), q
    with pytest.raises(ValueError, match="positive"):
        _gauss_hermite_normal_rule(0)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_restatements_match_the_reference(path):
    """The torch restatements the GPU tests use as their oracle reproduce the reference's expectation and r gradient."""
    g = np.load(path)
    m, v = torch.from_numpy(g["helper_els_mean"]), torch.from_numpy(g["helper_els_var"])
    for q in (12, 64):
        x, w = gauss_hermite(q)
        np.testing.assert_allclose(expected_log_sigmoid_negative_gaussian(m, v, x, w).numpy(), g[f"helper_els_q{q}"],
                                   rtol=1e-14, atol=0)
    y, m, v = (torch.from_numpy(g[k]) for k in ("helper_tcg_y", "helper_tcg_mean", "helper_tcg_var"))
    assert float(y.max()) == 1e4 and float(y.min()) == 0.0 and float(v.min()) < 0.0
    for q in (12, 16):
        x, w = gauss_hermite(q)
        got = [float(total_count_grad(y, m, v, float(r), x, w)) for r in g["helper_tcg_r"]]
        np.testing.assert_allclose(got, g[f"helper_tcg_q{q}"], rtol=1e-14, atol=0)


def test_goldens_are_present_small_and_carry_the_history_keys():
    assert [os.path.basename(p) for p in GOLDEN] == ["pgnb_se1d_learn_n500.npz", "pgnb_se2d_fixed_n1000.npz",
                                                      "pgnb_se3d_learn_n500.npz"]
    for p in GOLDEN:
        assert os.path.getsize(p) < (1 << 20)
        g = np.load(p)
        assert list(g["history_keys"]) == HISTORY_KEYS
        upd = g["history_total_count_updated"]
        assert upd[-1] == 0.0 and g["history_grad_total_count"][-1] == 0.0
        if "fixed" in p:
            assert not upd.any() and not g["history_grad_total_count"].any()
    # the learnt 1-D case steps r every second iteration: updated and skipped records both appear
    g = np.load(GOLDEN[0])
    assert list(g["history_total_count_updated"][:-1]) == [0.0, 1.0] * 4


def test_nb_entries_are_declared_with_signatures():
    import efgp_hip
    from efgp_hip.lib import _SIGNATURES
    names = efgp_hip.declared_symbols()
    for n in ("efgp_pg_nb_estep_update", "efgp_pg_nb_total_count_grad"):
        assert n in names and n in _SIGNATURES
    assert len(_SIGNATURES["efgp_pg_nb_estep_update"][1]) == 15 and len(_SIGNATURES["efgp_pg_nb_total_count_grad"][1]) == 11
