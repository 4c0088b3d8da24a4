"""Host checks of the dense restatement of the multi-output model (tests/_multi_dense.py): what tests/test_gpu_multi_output.py
compares EFGPNDMulti with.  No GPU."""
import numpy as np

import _ard_dense as D
import _multi_dense as MD
from kernels import SquaredExponential

N, B, T = 60, 3, 4
HS, SHAPE = (0.35, 0.35), (7, 7)
SIG = 0.3


def _problem():
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.0, 1.0, (N, 2))
    Y = np.stack([np.sin(3 * x[:, 0] + b) * np.cos(2 * x[:, 1]) + 0.1 * rng.standard_normal(N) for b in range(B)], axis=1)
    kern = SquaredExponential(dimension=2, init_lengthscale=0.4, init_variance=1.3)
    F = D.features(x, HS, SHAPE)
    ws, dprime = D.weights(kern, HS, SHAPE)
    Z = rng.integers(0, 2, (T, N)) * 2.0 - 1.0
    V = rng.integers(0, 2, (T, ws.size)) * 2.0 - 1.0
    return F, Y, ws, dprime, Z, V, float(kern.get_hyper("variance"))


def test_joint_gradient_is_the_sum_over_columns():
    F, Y, ws, dprime, Z, V, variance = _problem()
    grad, term1, term2 = MD.joint_gradient(F, Y, ws, dprime, SIG, Z, V, variance)
    per = [D.gradient_estimator(F, Y[:, b], ws, dprime, SIG, Z, V, variance) for b in range(B)]
    want = sum(p[0] for p in per)
    # rounding: every entry is a sum of O(B N M) products whose absolute values are bounded by the terms' own magnitudes
    scale = sum(np.abs(p[1]) + np.abs(p[2]) for p in per)
    assert np.all(np.abs(grad - want) <= 1e-12 * scale), (grad, want)
    assert np.all(np.abs(term2 - sum(p[2] for p in per)) <= 1e-12 * scale)
    assert np.all(np.abs(term1 - sum(p[1] for p in per)) <= 1e-12 * scale)


def test_trace_part_is_B_times_one_column():
    F, Y, ws, dprime, Z, V, variance = _problem()
    _, term1, _ = MD.joint_gradient(F, Y, ws, dprime, SIG, Z, V, variance)
    for b in range(B):          # term1 does not depend on the data: any column's will do
        one = D.gradient_estimator(F, Y[:, b], ws, dprime, SIG, Z, V, variance)[1]
        assert np.all(np.abs(term1 - B * one) <= 1e-12 * B * np.abs(one)), (b, term1, one)


def test_power_of_two_scaling_is_exact():
    F, Y, ws, _, _, _, _ = _problem()
    Y = Y * np.array([1.0, 1e-6, 1e6])[None, :]
    e = MD.scale_exponents(Y)
    assert np.all(np.abs(Y / np.ldexp(1.0, e)[None, :]).max(axis=0) < 1.0) and np.all(np.abs(Y / np.ldexp(1.0, e)[None, :]).max(axis=0) >= 0.5)
    # the same columns scaled by further powers of two: the solve sees the same numbers, the result is scaled exactly
    k = np.array([3, -17, 40])
    scaled = MD.fit_scaled(F, Y * np.ldexp(1.0, k)[None, :], ws, SIG)
    plain = MD.fit_scaled(F, Y, ws, SIG)
    assert np.array_equal(scaled, plain * np.ldexp(1.0, k)[:, None])
    # an all-zero column has exponent 0 and zero coefficients, without NaN
    Y0 = np.concatenate([Y, np.zeros((N, 1))], axis=1)
    assert MD.scale_exponents(Y0)[-1] == 0
    b0 = MD.fit_scaled(F, Y0, ws, SIG)
    assert np.all(b0[-1] == 0) and np.all(np.isfinite(b0))


def test_scaled_fit_matches_the_plain_fit():
    F, Y, ws, _, _, _, _ = _problem()
    plain, scaled = MD.fit(F, Y, ws, SIG), MD.fit_scaled(F, Y, ws, SIG)
    assert np.abs(plain - scaled).max() <= 1e-12 * np.abs(plain).max()
