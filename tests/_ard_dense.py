"""Dense restatements for the ARD tests (tests/test_ard_host.py, tests/test_gpu_ard.py), in numpy on the host.

Two references, both O(N^3) / O(M^3) and for small problems only:

* the exact GP with a kernel's `kernel_matrix`: posterior mean, latent variance, log marginal likelihood, and (for the squared
  exponential ARD kernel) an Adam loop on the exact negative log marginal likelihood;
* the feature-space model of EFGPND on a per-axis grid, with everything explicit: F[n, k] = exp(2 pi i sum_a k_a h_a x_na) on the
  box k_a = -(n_a - 1)/2 .. (n_a - 1)/2 (row-major, last axis fastest), ws = sqrt(S(omega_k) prod h_a), Dprime = prod h_a *
  spectral_grad, solves by numpy.linalg.solve, and the gradient estimator of efgp_gradient_assemble (include/efgp_hip.h)
  evaluated for GIVEN probes Z (T, N) and V (T, M).

An isotropic kernel is the case hs = (h,) * d, shape = (mtot,) * d.
"""
import math

import numpy as np
import torch


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


# ---- exact GP -----------------------------------------------------------------------------------------------------------------
def exact_gp(kernel, x, y, sigmasq, x_new):
    """(mean (B,), latent variance (B,), log marginal likelihood) of the exact GP with kernel.kernel_matrix."""
    x, x_new = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(x_new, dtype=torch.float64)
    K = _np(kernel.kernel_matrix(x, x)) + float(sigmasq) * np.eye(x.shape[0])
    Kn = _np(kernel.kernel_matrix(x_new, x))
    Knn = np.diag(_np(kernel.kernel_matrix(x_new, x_new)))
    yv = _np(y).astype(np.float64)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, yv))
    W = np.linalg.solve(L, Kn.T)
    lm = -0.5 * yv @ alpha - np.log(np.diag(L)).sum() - 0.5 * len(yv) * math.log(2 * math.pi)
    return Kn @ alpha, Knn - (W * W).sum(0), float(lm)


def draw_se_ard(x, ells, variance, sigmasq, seed):
    """y = f + noise with f from the exact squared-exponential ARD prior at x (numpy generator `seed`)."""
    x = _np(x).astype(np.float64)
    u = x / np.asarray(ells, dtype=np.float64)[None, :]
    d2 = ((u[:, None, :] - u[None, :, :]) ** 2).sum(-1)
    K = variance * np.exp(-0.5 * d2) + 1e-10 * np.eye(x.shape[0])
    rng = np.random.default_rng(seed)
    return np.linalg.cholesky(K) @ rng.standard_normal(x.shape[0]) + math.sqrt(sigmasq) * rng.standard_normal(x.shape[0])


def dense_adam_se_ard(x, y, ells0, variance0, sigmasq0, steps, lr):
    """Adam (torch defaults, step `lr`) on log(l_0 .. l_{d-1}, variance, sigma^2) with the EXACT gradient of the negative log
    marginal likelihood of the squared-exponential ARD GP: what EFGPND.optimize_hyperparameters approximates.  Returns the final
    (lengthscales, variance, sigma^2)."""
    xt, yt = torch.as_tensor(_np(x), dtype=torch.float64), torch.as_tensor(_np(y), dtype=torch.float64)
    d = xt.shape[1]
    raw = torch.log(torch.tensor(list(ells0) + [variance0, sigmasq0], dtype=torch.float64)).requires_grad_(True)
    opt = torch.optim.Adam([raw], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        p = raw.exp()
        u = xt / p[:d]
        K = p[d] * torch.exp(-0.5 * torch.cdist(u, u) ** 2) + p[d + 1] * torch.eye(xt.shape[0], dtype=torch.float64)
        L = torch.linalg.cholesky(K)
        nll = 0.5 * yt @ torch.cholesky_solve(yt[:, None], L)[:, 0] + torch.log(torch.diagonal(L)).sum()
        nll.backward()
        opt.step()
    p = raw.detach().exp().tolist()
    return p[:d], p[d], p[d + 1]


# ---- feature-space model --------------------------------------------------------------------------------------------------------
def mode_numbers(shape):
    """(M, d) integer mode numbers of the box, row-major, last axis fastest."""
    axes = [np.arange(-(n // 2), n // 2 + 1, dtype=np.float64) for n in shape]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(shape))


def frequencies(hs, shape):
    return mode_numbers(shape) * np.asarray(hs, dtype=np.float64)[None, :]


def features(x, hs, shape):
    """(N, M) complex: exp(2 pi i sum_a k_a h_a x_na)."""
    x = _np(x).astype(np.float64).reshape(len(x), -1)
    return np.exp(2j * math.pi * (x @ frequencies(hs, shape).T))


def weights(kernel, hs, shape):
    """(ws (M,), dprime (M, H)) from the kernel class's own spectral_density / spectral_grad."""
    om = torch.as_tensor(frequencies(hs, shape))
    hp = float(np.prod(hs))
    return np.sqrt(_np(kernel.spectral_density(om)) * hp), hp * _np(kernel.spectral_grad(om))


def operator_mean(F, ws, sigmasq):
    """A = D F^H F D + sigma^2 I."""
    return ws[:, None] * (F.conj().T @ F) * ws[None, :] + sigmasq * np.eye(len(ws))


def fit(F, y, ws, sigmasq):
    """beta = A^-1 D F^H y."""
    return np.linalg.solve(operator_mean(F, ws, sigmasq), ws * (F.conj().T @ _np(y)))


def mean(Fn, ws, beta):
    return (Fn @ (ws * beta)).real


def _solve_var(F, ws, sigmasq, rhs):
    """(D F^H F D / sigma^2 + I)^-1 rhs, rhs (M, R)."""
    return np.linalg.solve(operator_mean(F, ws, sigmasq) / sigmasq, rhs)


def variance_regular(F, Fn, ws, sigmasq):
    """s^2(x*) = max(0, Re sum_k f_k ws_k gamma_k), gamma = A_var^-1 (ws conj(f))   (efgp_variance_rhs / _contract)."""
    gamma = _solve_var(F, ws, sigmasq, (ws[None, :] * Fn.conj()).T)
    return np.maximum(0.0, ((Fn * ws[None, :]) * gamma.T).sum(1).real)


def variance_lag_sums(F, Fn, ws, sigmasq, eta, complex_sums=False):
    """The stochastic estimator with GIVEN probes eta (J, M): s^2(x*) = Re sum_r c[r] exp(2 pi i sum_a r_a h_a x*_a) with the lag sums
    c[r] = mean_j sum_{k-l=r} (ws u_j)[k] eta_j[l], u_j = A_var^-1 (ws eta_j) -- summed here as mean_j (f . ws u_j)(conj f . eta_j).
    complex_sums=True returns the complex sums the estimator is the real part of (the scale a real-only transform is judged on)."""
    eta = _np(eta).astype(np.float64)
    u = _solve_var(F, ws, sigmasq, (ws[None, :] * eta).T)               # (M, J)
    sums = ((Fn @ (ws[:, None] * u)) * (Fn.conj() @ eta.T)).mean(1)
    return sums if complex_sums else sums.real


def gradient_estimator(F, y, ws, dprime, sigmasq, Z, V, variance):
    """d(negative log marginal)/d(kernel hypers.., sigma^2) as efgp_gradient_assemble forms it (adjoint estimator) with probes
    Z (T, N) and V (T, M): the last kernel hyper is the variance, every other one is traced.  -> (grad, term1, term2)."""
    y, Z, V = _np(y).astype(np.float64), _np(Z).astype(np.float64), _np(V).astype(np.float64)
    N, M = F.shape
    H = dprime.shape[1]
    T = Z.shape[0]
    Tm = F.conj().T @ F
    A = operator_mean(F, ws, sigmasq)
    fy = F.conj().T @ y
    beta = np.linalg.solve(A, ws * fy)
    g = ws * beta
    tg = Tm @ g
    fa = (fy - tg) / sigmasq
    yy = float(y @ y)
    y_z, z_z = np.vdot(fy, g).real, np.vdot(g, tg).real
    a_norm = (yy - 2.0 * y_z + z_z) / sigmasq ** 2
    y_alpha = (yy - y_z) / sigmasq
    term1, term2 = np.zeros(H + 1), np.zeros(H + 1)
    for i in range(H):
        term2[i] = np.vdot(fa, dprime[:, i] * fa).real
    term2[H] = a_norm
    fz = (F.conj().T @ Z.T).T                                            # (T, M)
    for i in range(H - 1):
        rhs = ws[:, None] * (Tm @ (dprime[:, i, None] * fz.T))
        bk = np.linalg.solve(A, rhs).T                                   # (T, M)
        term1[i] = sum(np.vdot(fz[t], dprime[:, i] * fz[t] - ws * bk[t]).real for t in range(T)) / sigmasq / T
    bn = np.linalg.solve(A, ws[:, None] * (Tm @ (ws[:, None] * V.T))).T
    t1_noise = N / sigmasq - np.mean([np.vdot(V[t], bn[t]).real for t in range(T)]) / sigmasq
    term1[H] = t1_noise
    term2[H - 1] = (y_alpha - sigmasq * a_norm) / variance
    term1[H - 1] = (N - sigmasq * t1_noise) / variance
    return 0.5 * (term1 - term2), term1, term2


def kernel_error(kernel, x, hs, shape):
    """max |k(x_i, x_j) - feature-space kernel| over the points x: what the quadrature tolerance eps bounds."""
    F = features(x, hs, shape)
    ws, _ = weights(kernel, hs, shape)
    x = torch.as_tensor(_np(x), dtype=torch.float64)
    return float(np.abs(((F * ws[None, :] ** 2) @ F.conj().T).real - _np(kernel.kernel_matrix(x, x))).max())
