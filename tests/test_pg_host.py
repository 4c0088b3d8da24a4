"""Polya-Gamma classifier, host side (no GPU): import surface without scikit-learn, option refusals, the closed-form helpers
against the reference's recorded values, and the new C-ABI entries declared in include/efgp_hip.h."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gp-quadrature_amd")
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pg_*.npz")))


def _xy(n=40, d=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, d))
    y = (X[:, 0] > 0).astype(int)
    return X, y


def test_package_imports_without_sklearn():
    """Both import forms work in a process where scikit-learn cannot be imported at all."""
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name == 'sklearn' or name.startswith('sklearn.'):\n"
            "            raise ImportError('sklearn blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            f"sys.path.insert(0, {PKG!r})\n"
            "from polyagamma_classification import PolyagammaGPClassifier, approximate_logistic_gaussian_prob, _pg_omega_expectation\n"
            f"sys.path.insert(0, {os.path.join(PKG, 'polyagamma_classification')!r})\n"
            "from pg_classifier import PolyagammaGPClassifier as P2\n"
            "assert 'sklearn' not in sys.modules\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr


def test_constructor_keeps_reference_defaults():
    from polyagamma_classification import PolyagammaGPClassifier
    clf = PolyagammaGPClassifier()
    p = clf.get_params()
    assert p["kernel"] == "squared_exponential" and p["lengthscale_init"] == 0.3 and p["variance_init"] == 1.0
    assert p["max_iter"] == 50 and p["e_step_iters"] == 1 and p["n_e_probes"] == 10 and p["n_m_probes"] == 10
    assert p["cg_tol"] == 1e-6 and p["nufft_eps"] == 1e-7 and p["spectral_eps"] == 1e-4 and p["trunc_eps"] == 1e-4
    assert p["use_exact_weighted_toeplitz_operator"] is True and p["prediction_batch_size"] == 64
    assert p["predictive_variance_method"] == "exact" and p["random_state"] is None and p["dtype"] == "float64"
    assert clf.set_params(max_iter=3).max_iter == 3
    with pytest.raises(ValueError):
        clf.set_params(no_such_option=1)


def test_non_binary_targets_are_refused():
    from polyagamma_classification import PolyagammaGPClassifier
    X, _ = _xy()
    with pytest.raises(ValueError, match="binary"):
        PolyagammaGPClassifier(max_iter=1).fit(X, np.arange(X.shape[0]) % 3)
    with pytest.raises(ValueError, match="binary"):
        PolyagammaGPClassifier(max_iter=1).fit(X, np.zeros(X.shape[0]))


@pytest.mark.parametrize("kwargs,exc,word", [
    ({"kernel": "matern"}, ValueError, "kernel"),
    ({"dtype": "float32"}, ValueError, "float32"),
    ({"dtype": torch.float32}, ValueError, "float32"),
    ({"predictive_variance_method": "chebyshev"}, NotImplementedError, "chebyshev"),
    ({"predictive_variance_method": "stochastic"}, NotImplementedError, "stochastic"),
    ({"predictive_variance_method": "bogus"}, ValueError, "bogus"),
    ({"device": "cpu"}, ValueError, "cpu"),
])
def test_unsupported_options_are_refused_by_name(kwargs, exc, word):
    from polyagamma_classification import PolyagammaGPClassifier
    X, y = _xy()
    with pytest.raises(exc, match=word):
        PolyagammaGPClassifier(max_iter=1, **kwargs).fit(X, y)


def test_unfitted_prediction_is_an_error():
    from polyagamma_classification import PolyagammaGPClassifier
    with pytest.raises(RuntimeError, match="not fitted"):
        PolyagammaGPClassifier().predict(np.zeros((2, 2)))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_helpers_match_the_reference(path):
    from polyagamma_classification import _pg_omega_expectation, approximate_logistic_gaussian_prob
    g = np.load(path)
    mean, var = torch.from_numpy(g["helper_mean"]), torch.from_numpy(g["helper_var"])
    np.testing.assert_allclose(approximate_logistic_gaussian_prob(mean, var).numpy(), g["helper_prob"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(approximate_logistic_gaussian_prob(mean).numpy(), g["helper_prob_novar"], rtol=1e-15, atol=0)
    c, b = torch.from_numpy(g["helper_c"]), torch.from_numpy(g["helper_b"])
    np.testing.assert_allclose(_pg_omega_expectation(c, b).numpy(), g["helper_omega"], rtol=1e-15, atol=0)


def test_goldens_are_present_and_small():
    assert len(GOLDEN) == 3
    for p in GOLDEN:
        assert os.path.getsize(p) < (1 << 20)
        g = np.load(p)
        assert set(g["history_keys"]) == {"iter", "lengthscale", "variance", "grad_lengthscale", "grad_variance", "e_residual",
                                          "e_cg_iters", "m_cg_iters", "approx_accuracy"}


def test_pg_entries_are_declared_with_signatures():
    import efgp_hip
    from efgp_hip.lib import _SIGNATURES
    names = efgp_hip.declared_symbols()
    for n in ("efgp_pg_estep_update", "efgp_pg_mstep_terms", "efgp_pg_weight_rows"):
        assert n in names and n in _SIGNATURES
