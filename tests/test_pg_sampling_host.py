"""Posterior function draws on the Polya-Gamma estimators, host side (no GPU): the new C-ABI entry is declared, the estimators
carry the sampling methods, the refusals hold before any device work, and the six-decade scale vector of the GPU tests is within
reach of a fixed-point spreader sized from the largest strength."""
import numpy as np
import pytest
import torch

import _pg_sampling as P


def test_scaled_normal_entry_is_declared_with_a_signature():
    import efgp_hip
    from efgp_hip.lib import _SIGNATURES
    assert "efgp_nufft_type1_normal_scaled" in efgp_hip.declared_symbols()
    assert "efgp_nufft_type1_normal_scaled" in _SIGNATURES
    assert len(_SIGNATURES["efgp_nufft_type1_normal_scaled"][1]) == 9
    assert hasattr(efgp_hip.NufftPlan, "type1_normal_scaled")


def test_estimators_have_the_sampling_methods():
    from polyagamma_classification import PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor
    for cls in (PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor):
        assert callable(getattr(cls, "sample_latent"))
        assert isinstance(getattr(cls, "last_sample_stats"), property)
    assert callable(getattr(PolyagammaGPClassifier, "sample_proba"))
    assert callable(getattr(PolyagammaGPNegativeBinomialRegressor, "sample_mean_count"))
    assert PolyagammaGPClassifier().last_sample_stats == {}


@pytest.mark.parametrize("method", ["sample_latent", "sample_proba"])
def test_unfitted_classifier_is_refused_before_any_device_work(method):
    from polyagamma_classification import PolyagammaGPClassifier
    with pytest.raises(RuntimeError, match="not fitted"):
        getattr(PolyagammaGPClassifier(), method)(np.zeros((2, 2)), 3)


@pytest.mark.parametrize("method", ["sample_latent", "sample_mean_count"])
def test_unfitted_regressor_is_refused_before_any_device_work(method):
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    with pytest.raises(RuntimeError, match="not fitted"):
        getattr(PolyagammaGPNegativeBinomialRegressor(), method)(np.zeros((2, 2)), 3)


def _as_if_fitted(cls):
    """An estimator that passes `_check_fitted` with two features and nothing else: every refusal below must come before the first
    use of a device (there is none here)."""
    est = cls()
    est._beta_mean = torch.zeros(1, dtype=torch.complex128)
    est.n_features_in_ = 2
    return est


def test_bad_sample_count_and_column_count_are_refused_by_name():
    from polyagamma_classification import PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor
    for cls in (PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor):
        est = _as_if_fitted(cls)
        for bad in (0, -2):
            with pytest.raises(ValueError, match="n_samples"):
                est.sample_latent(np.zeros((3, 2)), bad)
        with pytest.raises(ValueError, match=r"\(n_samples, 2\)"):
            est.sample_latent(np.zeros((3, 3)), 2)
        with pytest.raises(ValueError, match="max_cg_iterations"):
            est.sample_latent(np.zeros((3, 2)), 2, max_cg_iterations=0)
    with pytest.raises(ValueError, match="n_samples"):
        PolyagammaGPClassifier().sample_latent(np.zeros((3, 2)), 0)             # a bad count is refused fitted or not
    with pytest.raises(ValueError, match=r"\(n_samples, 2\)"):
        _as_if_fitted(PolyagammaGPClassifier).sample_proba(np.zeros((3, 1)), 2)
    with pytest.raises(ValueError, match=r"\(n_samples, 2\)"):
        _as_if_fitted(PolyagammaGPNegativeBinomialRegressor).sample_mean_count(np.zeros((3, 1)), 2)


def test_scale_vectors_are_what_the_gpu_tests_say():
    s = P.pg_like_scale(50000, 1)
    assert float(s.min()) > 0 and 100.0 < float(s.max()) <= 250.0 and torch.isfinite(s).all()
    z = P.six_decade_scale(50000, 1)
    nz = z[z > 0]
    assert float(z.max()) == 1.0 and int((z == 0).sum()) >= 50000 // 7 and 1e-6 <= float(nz.min()) < 2e-6


@pytest.mark.parametrize("d,nm,h", [(1, 41, 0.2), (2, 23, 0.31)])
def test_six_decade_scale_is_within_reach_of_max_scaled_fixed_point(d, nm, h):
    """The fixed-point spreaders size ONE scale from the largest strength, bound * max(scale), as the memory rows do from max|c|.
    With N = 5e4 points the accumulators hold at least 2^61 / N > 2^45 steps per unit of that maximum (csrc/nufft.hip,
    fixed_scale_for), every one of the W^d <= 8^3 contributions of a point is rounded to a step, and a row's own norm is set by
    its large entries: a strength vector rounded that coarsely must stay orders of magnitude inside the 2 tol = 2e-7 the GPU tests
    ask against the exact sums, or the six-decade range would have to be narrowed there.  Checked here in double precision with
    the oracle's exact sums, every strength moved by a full W^d = 512 steps of 2^-45 max|c| in the worst direction."""
    from oracle import efgp_oracle as O
    N, bound = 4000, 8.5717
    g = torch.Generator().manual_seed(3)
    x = torch.rand(N, d, generator=g, dtype=torch.float64) * 2 - 1
    s = P.six_decade_scale(N, 11)
    zn = torch.randn(2, N, generator=g, dtype=torch.float64).clamp(-bound, bound)
    c = s * zn
    step = bound * float(s.max()) * 2.0 ** -45
    moved = c + 512 * step * torch.sign(torch.randn(2, N, generator=g, dtype=torch.float64))
    shape = (nm,) * d
    exact = O.nudft_type1(x, h, c, shape)
    coarse = O.nudft_type1(x, h, moved, shape)
    for b in range(2):
        err = float(torch.linalg.norm((coarse[b] - exact[b]).reshape(-1)) / torch.linalg.norm(exact[b].reshape(-1)))
        print(f"{d}-D six decades, row {b}: fixed-point model error {err:.2e} of the row's norm")
        assert err < 1e-2 * 2e-7
