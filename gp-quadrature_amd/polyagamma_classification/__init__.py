"""Binary GP classification by Polya-Gamma augmentation on the HIP EFGP operators
(reference: polyagamma_classification/pg_classifier.py).

The directory mirrors the reference's: with it on sys.path, ``from pg_classifier import PolyagammaGPClassifier`` works as
there; from the package root, ``from polyagamma_classification import PolyagammaGPClassifier``."""
import os as _os
import sys as _sys

_PKG = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
if _PKG not in _sys.path:
    _sys.path.insert(0, _PKG)

from .pg_classifier import (PolyagammaGPClassifier, _pg_omega_expectation,  # noqa: E402
                            approximate_logistic_gaussian_prob)

__all__ = ["PolyagammaGPClassifier", "approximate_logistic_gaussian_prob", "_pg_omega_expectation"]
