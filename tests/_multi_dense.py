"""Dense restatement of the multi-output model (efgpnd_multi.EFGPNDMulti) for tests/test_multi_output_host.py and
tests/test_gpu_multi_output.py, in numpy on the host, built on tests/_ard_dense.py.

B outputs at the same points with one kernel and one noise level are B independent feature-space models that share the operator
A = D F^H F D + sigma^2 I: the coefficients are B columns of one direct solve, and the gradient of the joint negative log marginal
is the sum of the per-output estimators with the SAME probes Z (T, N), V (T, M).  Its trace part (term1) does not depend on the
data, so it is B times one output's; its data part (term2) is the sum of the outputs'.
"""
import numpy as np

import _ard_dense as D


def fit(F, Y, ws, sigmasq):
    """beta (B, M): row b = A^-1 D F^H y_b, all columns in one direct solve."""
    Y = D._np(Y).astype(np.float64)
    A = D.operator_mean(F, ws, sigmasq)
    return np.linalg.solve(A, ws[:, None] * (F.conj().T @ Y)).T


def scale_exponents(Y):
    """e_b = frexp exponent of max|y_b| (0 for an all-zero column): column b is stored as y_b / 2^e_b."""
    Y = D._np(Y).astype(np.float64)
    return np.frexp(np.abs(Y).max(axis=0))[1]


def fit_scaled(F, Y, ws, sigmasq):
    """`fit` the way the model does it: columns divided by 2^e_b, solved, coefficients multiplied back."""
    Y = D._np(Y).astype(np.float64)
    s = np.ldexp(1.0, scale_exponents(Y))
    return fit(F, Y / s[None, :], ws, sigmasq) * s[:, None]


def joint_gradient(F, Y, ws, dprime, sigmasq, Z, V, variance):
    """(grad, term1, term2) of the joint objective: the data part summed over the columns, the trace part computed ONCE (from
    column 0's estimator, where it does not depend on the column) and counted B times."""
    Y = D._np(Y).astype(np.float64)
    B = Y.shape[1]
    _, term1_one, _ = D.gradient_estimator(F, Y[:, 0], ws, dprime, sigmasq, Z, V, variance)
    term2 = np.zeros_like(term1_one)
    for b in range(B):
        term2 += D.gradient_estimator(F, Y[:, b], ws, dprime, sigmasq, Z, V, variance)[2]
    term1 = B * term1_one
    return 0.5 * (term1 - term2), term1, term2


def draw_columns(x, ells, variance, sigmasq, seed, B):
    """(N, B): B independent draws of y = f + noise from ONE squared-exponential (ARD) prior at x (`_ard_dense.draw_se_ard`)."""
    return np.stack([D.draw_se_ard(x, ells, variance, sigmasq, seed + 1000 * b) for b in range(B)], axis=1)
