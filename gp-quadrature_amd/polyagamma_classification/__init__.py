"""GP classification and count regression by Polya-Gamma augmentation on the HIP EFGP operators
(reference: polyagamma_classification/pg_classifier.py): PolyagammaGPClassifier (binary labels) and
PolyagammaGPNegativeBinomialRegressor (negative-binomial counts).

The directory mirrors the reference's: with it on sys.path, ``from pg_classifier import PolyagammaGPClassifier`` works as
there; from the package root, ``from polyagamma_classification import PolyagammaGPClassifier``."""
import os as _os
import sys as _sys

_PKG = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
if _PKG not in _sys.path:
    _sys.path.insert(0, _PKG)

from .pg_classifier import (PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor,  # noqa: E402
                            _gauss_hermite_normal_rule, _pg_omega_expectation, approximate_logistic_gaussian_prob,
                            negative_binomial_gaussian_mean)

__all__ = ["PolyagammaGPClassifier", "PolyagammaGPNegativeBinomialRegressor", "approximate_logistic_gaussian_prob",
           "negative_binomial_gaussian_mean", "_gauss_hermite_normal_rule", "_pg_omega_expectation"]
