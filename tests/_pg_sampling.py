"""Helpers of the PG sampler's tests: the scale vectors of the scaled-noise transform, small seeded estimators, and the dense
restatement of `sample_latent` (torch on the host or the device; feature matrices as in tests/_sampling.py).

Weight-space model of the fitted variational posterior: weights ~ N(m, A^-1), A = I + D F^H diag(delta) F D with D = diag(ws), F
the (N, M) matrix of phi_j(x_n) and delta the fitted PG expectation; a draw is

    u = A^-1 (D F^H (sqrt(delta) .* e1) + e2),   f(x*) = Re Phi_new (ws .* (ws .* m + u)),

and the bracket has covariance D F^H diag(delta) F D + I = A."""
import math

import numpy as np
import torch

import _sampling as S


def pg_like_scale(N, seed):
    """0.25 b tanh(c / 2) / (c / 2): PG expectations with the shape b log-uniform on [1, 1e3] (the negative-binomial range) and
    the tilt c uniform on [0, 12]."""
    g = torch.Generator().manual_seed(seed)
    b = 10.0 ** (3.0 * torch.rand(N, generator=g, dtype=torch.float64))
    c = 12.0 * torch.rand(N, generator=g, dtype=torch.float64)
    half = (0.5 * c).clamp_min(1e-12)
    return 0.25 * b * torch.tanh(half) / half


def six_decade_scale(N, seed):
    """Log-uniform on [1e-6, 1] with the maximum 1 present and every seventh entry an exact zero."""
    g = torch.Generator().manual_seed(seed)
    s = 10.0 ** (-6.0 * torch.rand(N, generator=g, dtype=torch.float64))
    s[0::7] = 0.0
    s[1] = 1.0
    return s


SCALES = {"pg": pg_like_scale, "six_decades": six_decade_scale}


def small_classifier(d, **over):
    """A seeded PolyagammaGPClassifier on 1000 points of [-1, 1]^d (five outer iterations) and its training inputs."""
    from polyagamma_classification import PolyagammaGPClassifier
    rng = np.random.default_rng(40 + d)
    X = rng.uniform(-1, 1, (1000, d))
    f = 2.0 * np.sin(3.0 * X[:, 0]) * (np.cos(2.5 * X[:, -1]) if d > 1 else 1.0) + 0.5 * X[:, -1]
    y = (rng.uniform(size=X.shape[0]) < 1.0 / (1.0 + np.exp(-2.0 * f))).astype(int)
    params = dict(max_iter=5, random_state=3, cg_tol=1e-8, nufft_eps=1e-7, lengthscale_init=0.3 if d > 1 else 0.2, device="cuda")
    params.update(over)
    return PolyagammaGPClassifier(**params).fit(X, y), X


def small_nb_regressor(**over):
    """A seeded PolyagammaGPNegativeBinomialRegressor (r = 3) on 800 points of [-1, 1]^2 and its training inputs."""
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    rng = np.random.default_rng(77)
    X = rng.uniform(-1, 1, (800, 2))
    f = np.sin(2.5 * X[:, 0]) + 0.7 * X[:, 1]
    p = 1.0 / (1.0 + np.exp(-f))
    y = rng.negative_binomial(3.0, 1.0 - p).astype(np.float64)          # mean r p / (1 - p) = r exp(f)
    params = dict(total_count=3.0, max_iter=5, random_state=5, cg_tol=1e-8, nufft_eps=1e-7, device="cuda")
    params.update(over)
    return PolyagammaGPNegativeBinomialRegressor(**params).fit(X, y), X


def sampler_rhs(F, ws, delta, e1, e2):
    """D F^H (sqrt(delta) .* e1) + e2 for rows e1 (S, N) real and e2 (S, M) complex -> (S, M)."""
    return ws.reshape(1, -1) * ((e1 * torch.sqrt(delta).reshape(1, -1)).to(F.dtype) @ F.conj()) + e2


def operator_A(F, ws, delta):
    """A = I + D F^H diag(delta) F D as a dense (M, M) complex matrix."""
    M = F.shape[1]
    G = F.conj().T @ (delta.reshape(-1, 1).to(F.dtype) * F)
    return ws.reshape(M, 1) * G * ws.reshape(1, M) + torch.eye(M, dtype=F.dtype, device=F.device)


def latent_cov(F, F_new, ws, delta):
    """Covariance of the draws at the rows of F_new: Phi_new D A^-1 D Phi_new^H (real for conjugate-even weights)."""
    PD = F_new * ws.reshape(1, -1)
    return (PD @ torch.linalg.solve(operator_A(F, ws, delta), PD.conj().T)).real


def apply_A(est, v):
    """A v = v + ws .* T_w(ws .* v) through the estimator's fitted Toeplitz operator, row by row, independently of the solver."""
    spec = est._spec
    ws = spec.ws.reshape(-1)
    rows = v.reshape(-1, spec.M)
    return (rows + ws * est._op_pred.apply(ws * rows).reshape(rows.shape)).reshape(v.shape)


def moment_points(seed=101):
    """16 test points in [-1.2, 1.2]^2 (some outside the data's box), two pairs closer than a lengthscale (0.3)."""
    g = torch.Generator().manual_seed(seed)
    xn = torch.rand(16, 2, generator=g, dtype=torch.float64) * 2.4 - 1.2
    xn[1] = xn[0] + torch.tensor([0.12, -0.05], dtype=torch.float64)
    xn[3] = xn[2] + torch.tensor([-0.08, 0.1], dtype=torch.float64)
    return xn


def cg_iteration_bound(cond, tol):
    """CG's worst case for a relative residual tol: sqrt(cond) ln(2 / tol) / 2."""
    return 0.5 * math.sqrt(cond) * math.log(2.0 / tol)


feature_matrix = S.feature_matrix
hermitian_rows = S.hermitian_rows
paths_from_weights = S.paths_from_weights
