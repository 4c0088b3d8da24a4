"""Dense restatement of the posterior gradient (EFGPND.predict_gradient) for tests/test_predict_gradient_host.py and
tests/test_gpu_predict_gradient.py, in float64 torch on the CPU (torch, so that autograd can check the derivative rows).

Everything explicit on a per-axis grid (an isotropic grid is hs = (h,) * d, shape = (mtot,) * d):

    Phi[n, k]    = exp(2 pi i sum_a xi_ka x_na),   xi_ka = h_a k_a,  k_a = -(n_a // 2) .. (n_a - 1) // 2, row-major
    Phi'_a[n, k] = 2 pi i xi_ka Phi[n, k]                                     the derivative of feature k along axis a
    A = D Phi^H Phi D + sigma^2 I,  beta = A^-1 D Phi^H y                     the normal equations of the fit
    mean = Re Phi* D beta,          d_a mean = Re Phi*'_a D beta
    C = D (A / sigma^2)^-1 D                                                  the noise scaling of tests/_ard_dense.variance_regular
    Var f = diag(Phi* C Phi*^H),    Var d_a f = diag(Phi*'_a C Phi*'_a^H)
    the same with GIVEN probes eta (J, M): mean_j (Phi* D u_j)(conj Phi* eta_j), u_j = (A / sigma^2)^-1 D eta_j
"""
import math

import torch

from _nudft import mode_numbers

_RD, _CD = torch.float64, torch.complex128


def frequencies(hs, shape):
    """(M, d): xi_ka of every mode, row-major, last axis fastest."""
    axes = [mode_numbers(n, 0) * float(h) for n, h in zip(shape, hs)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(shape))


def features(x, hs, shape):
    """(N, M) complex128; differentiable in x."""
    x = torch.as_tensor(x, dtype=_RD).reshape(len(x), -1)
    ang = (2.0 * math.pi) * (x @ frequencies(hs, shape).T)
    return torch.complex(torch.cos(ang), torch.sin(ang))


def feature_derivatives(Phi, hs, shape):
    """List over the axes of (N, M): 2 pi i xi_a Phi."""
    xi = frequencies(hs, shape)
    return [Phi * torch.complex(torch.zeros(len(xi), dtype=_RD), 2.0 * math.pi * xi[:, a])[None, :] for a in range(len(shape))]


def exact_type2(x, hs, shape, f):
    """Re sum_k f_k exp(2 pi i sum_a h_a k_a x_a) at the points x, one phase table per axis as tests/_nudft._tables builds them (but
    with the spacing of each axis) -> (N,) float64."""
    x = torch.as_tensor(x, dtype=_RD).reshape(len(x), -1)
    tabs = []
    for a, n in enumerate(shape):
        ang = (2.0 * math.pi * float(hs[a])) * x[:, a, None] * mode_numbers(n, 0)[None, :]
        tabs.append(torch.complex(torch.cos(ang), torch.sin(ang)))
    ff = torch.as_tensor(f).to(_CD).reshape(tuple(shape))
    spec = {1: "k,nk->n", 2: "kl,nk,nl->n", 3: "klm,nk,nl,nm->n"}[len(shape)]
    return torch.einsum(spec, ff, *tabs).real


def operator_mean(F, ws, sigmasq):
    ws = torch.as_tensor(ws).to(_CD)
    return ws[:, None] * (F.conj().T @ F) * ws[None, :] + float(sigmasq) * torch.eye(len(ws), dtype=_CD)


def fit(F, y, ws, sigmasq):
    ws = torch.as_tensor(ws).to(_CD)
    return torch.linalg.solve(operator_mean(F, ws, sigmasq), ws * (F.conj().T @ torch.as_tensor(y).to(_CD)))


def mean(Fn, ws, beta):
    return (Fn @ (torch.as_tensor(ws).to(_CD) * beta)).real


def mean_gradient(dFn, ws, beta):
    """(N*, d) from the derivative rows dFn = feature_derivatives(Fn, ..)."""
    g = torch.as_tensor(ws).to(_CD) * beta
    return torch.stack([(Fa @ g).real for Fa in dFn], dim=1)


def covariance(F, ws, sigmasq):
    """C = D (A / sigma^2)^-1 D, (M, M)."""
    ws = torch.as_tensor(ws).to(_CD)
    return ws[:, None] * torch.linalg.inv(operator_mean(F, ws, sigmasq) / float(sigmasq)) * ws[None, :]


def variance(Fn, C):
    return ((Fn @ C) * Fn.conj()).sum(dim=1).real


def gradient_variance(dFn, C):
    return torch.stack([variance(Fa, C) for Fa in dFn], dim=1)


def _probe_solves(F, ws, sigmasq, eta):
    ws = torch.as_tensor(ws).to(_CD)
    eta = torch.as_tensor(eta).to(_CD)
    u = torch.linalg.solve(operator_mean(F, ws, sigmasq) / float(sigmasq), (ws[None, :] * eta).T)          # (M, J)
    return ws[:, None] * u, eta


def variance_probes(F, Fn, ws, sigmasq, eta):
    """The stochastic estimator of Var f with GIVEN probes eta (J, M) applied to the dense C."""
    g, eta = _probe_solves(F, ws, sigmasq, eta)
    return ((Fn @ g) * (Fn.conj() @ eta.T)).mean(dim=1).real


def gradient_variance_probes(F, dFn, ws, sigmasq, eta):
    g, eta = _probe_solves(F, ws, sigmasq, eta)
    return torch.stack([((Fa @ g) * (Fa.conj() @ eta.T)).mean(dim=1).real for Fa in dFn], dim=1)
