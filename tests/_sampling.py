"""Dense restatement of the weight-space sampler of EFGPND.sample_paths, for the tests (torch on the host or the device).

Feature model on the equispaced mode grid {-m..m}^d (row-major flat index j, spacing h): f(x) = Re sum_j phi_j(x) ws_j w_j with
phi_j(x) = exp(2 pi i h k_j . x) and w ~ N(0, I) (conjugate-even complex normal, so f is real).  With D = diag(ws), F the (N, M)
matrix of phi_j(x_n) and A = D F^H F D + sigma^2 I, the posterior of the weights given y = f(x) + noise is N(beta, sigma^2 A^-1),
beta = A^-1 D F^H y, and

    w = beta + A^-1 (sigma D F^H e1 + sigma^2 e2),   e1 ~ N(0, I_N) real,  e2 conjugate-even standard complex normal,

has that law: the bracket has covariance sigma^2 D F^H F D + sigma^4 I = sigma^2 A.
"""
import math

import torch


def mode_grid(mtot, d):
    """(M, d) float64 integer frequencies k_j of the box {-m..m}^d, last dimension fastest."""
    m = (int(mtot) - 1) // 2
    k1 = torch.arange(-m, m + 1, dtype=torch.float64)
    if d == 1:
        return k1.reshape(-1, 1)
    return torch.cartesian_prod(*([k1] * d)).reshape(-1, d)


def conj_index(M):
    """Flat index of the negated frequency of every mode: j -> M - 1 - j (the box is symmetric and row-major)."""
    return torch.arange(int(M) - 1, -1, -1)


def feature_matrix(x, h, mtot):
    """(N, M) complex128 matrix of phi_j(x_n) = exp(2 pi i h k_j . x_n) on x's device."""
    x = x.reshape(x.shape[0], -1).to(torch.float64)
    k = mode_grid(mtot, x.shape[1]).to(x.device)
    ph = 2.0 * math.pi * float(h) * (x @ k.T)
    return torch.complex(torch.cos(ph), torch.sin(ph))


def hermitian_rows(fill, a=0.0, ws=None, fz=None, b=1.0):
    """What efgp_hermitian_normal_rows computes, from fill = normal_fill(seed, 2 S rows, M): rows p = fill[2s], q = fill[2s + 1];
    e[s, j] = (p[j] + i q[j]) / sqrt 2 below the centre, p[centre] at the centre, conj of the mirror above; a ws fz + b e, the
    first term (like the kernel) from the lower half of fz mirrored."""
    p, q = fill[0::2], fill[1::2]
    S, M = p.shape
    c = (M - 1) // 2
    low = torch.complex(p[:, :c], q[:, :c]) / math.sqrt(2.0) * b
    mid = torch.complex(p[:, c:c + 1] * b, torch.zeros_like(p[:, c:c + 1]))
    if ws is not None:
        prod = a * ws.reshape(1, M) * fz.reshape(S, M)
        low = low + prod[:, :c]
        mid = mid + torch.complex(prod[:, c:c + 1].real, torch.zeros_like(p[:, c:c + 1]))
    return torch.cat([low, mid, low.flip(1).conj()], dim=1)


def conj_even_normal(S, M, generator):
    """Host draw of S conjugate-even standard complex normal rows (E e e^H = I) from a torch generator."""
    fill = torch.randn(2 * S, M, dtype=torch.float64, generator=generator)
    return hermitian_rows(fill)


def operator_A(F, ws, sigmasq):
    """A = D F^H F D + sigma^2 I as a dense (M, M) complex matrix."""
    M = F.shape[1]
    G = F.conj().T @ F
    return ws.reshape(M, 1) * G * ws.reshape(1, M) + float(sigmasq) * torch.eye(M, dtype=F.dtype, device=F.device)


def posterior_weights(F, y, ws, sigmasq):
    A = operator_A(F, ws, sigmasq)
    return torch.linalg.solve(A, ws * (F.conj().T @ y.to(F.dtype)))


def sampler_rhs(F, ws, sigmasq, e1, e2):
    """sigma D F^H e1 + sigma^2 e2 for rows e1 (S, N) real and e2 (S, M) complex -> (S, M)."""
    sig = float(sigmasq)
    return math.sqrt(sig) * ws.reshape(1, -1) * (e1.to(F.dtype) @ F.conj()) + sig * e2


def dense_paths(F, F_new, ws, sigmasq, beta, e1, e2):
    """(S, B) posterior draws at the rows of F_new and the (S, M) weights, with torch.linalg.solve."""
    A = operator_A(F, ws, sigmasq)
    delta = torch.linalg.solve(A, sampler_rhs(F, ws, sigmasq, e1, e2).T).T
    w = beta.reshape(1, -1) + delta
    return paths_from_weights(F_new, ws, w), w


def paths_from_weights(F_new, ws, w):
    """f[s, b] = Re sum_j phi_j(x_b) ws_j w[s, j]."""
    return ((ws.reshape(1, -1) * w) @ F_new.T).real


def weight_space_cov(F, F_new, ws, sigmasq):
    """Covariance of the draws at the rows of F_new: sigma^2 Phi D A^-1 D Phi^H (real for conjugate-even weights)."""
    A = operator_A(F, ws, sigmasq)
    PD = F_new * ws.reshape(1, -1)
    return (float(sigmasq) * PD @ torch.linalg.solve(A, PD.conj().T)).real


def function_space_cov(F, F_new, ws, sigmasq):
    """Exact posterior covariance of the feature model's GP, kernel K = F D^2 F^H: K_nn - K_no (K_oo + sigma^2 I)^-1 K_on."""
    D2 = (ws * ws.conj()).real.to(F.dtype).reshape(1, -1)
    K_oo = ((F * D2) @ F.conj().T).real
    K_no = ((F_new * D2) @ F.conj().T).real
    K_nn = ((F_new * D2) @ F_new.conj().T).real
    N = F.shape[0]
    return K_nn - K_no @ torch.linalg.solve(K_oo + float(sigmasq) * torch.eye(N, dtype=K_oo.dtype, device=K_oo.device), K_no.T)


def prior_cov(F_new, ws):
    """Kernel of the feature model at the rows of F_new: sum_j |ws_j|^2 cos(2 pi xi_j . (x - x'))."""
    D2 = (ws * ws.conj()).real.to(F_new.dtype).reshape(1, -1)
    return ((F_new * D2) @ F_new.conj().T).real
