"""Helpers of the tests of the PG estimators' approximate predictive variances, written from the formulas (numpy / torch on the
host, no product code):

Chebyshev route.  Per axis: nodes mid + half cos(pi k / (n - 1)) sorted ascending, barycentric weights (-1)^k halved at both
ends in the same order.  For a target x: if |x - x_k| <= 1e-14 for some k the weight row is one-hot at the first such k, else
w_k = (c_k / (x - x_k)) / sum_l (c_l / (x - x_l)).  The interpolant is sum over the node box of prod_a w_a[i_a] V[i_0, ..].

Stochastic route.  A = I + Ds G Ds with G = F^H diag(delta) F and Ds = sqrt(max(ws^2, floor)), floor = max(mean(ws^2) 1e-14,
1e-14); y = A^-1 Ds eta for +-1 probes eta on the mode grid, gamma = ws^2 / Ds y; c[r] = mean_j sum_{k - l = r} gamma_j[k] eta_j[l]
on the (2 mtot - 1)^d lag box; variance(x) = max(0, Re sum_r c[r] exp(2 pi i h r . x)).
"""
import json
import math
import os

import numpy as np
import torch

import _sampling as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("se2d_n1000", "se1d_n500", "se3d_n500")
HIT = 1e-14


def cheb_axis(lo, hi, n):
    """(nodes ascending, weights in the same order) of the n Chebyshev-Lobatto points of [lo, hi]."""
    k = np.arange(n, dtype=np.float64)
    nodes = 0.5 * (lo + hi) + 0.5 * (hi - lo) * np.cos(np.pi * k / (n - 1))
    weights = (-1.0) ** k
    weights[0] *= 0.5
    weights[-1] *= 0.5
    order = np.argsort(nodes)
    return nodes[order], weights[order]


def bary_matrix(nodes, weights, targets):
    """(len(targets), len(nodes)) rows of interpolation weights."""
    nodes, weights, targets = (np.asarray(v, dtype=np.float64) for v in (nodes, weights, targets))
    mat = np.zeros((targets.size, nodes.size))
    for i, x in enumerate(targets):
        diff = x - nodes
        hits = np.nonzero(np.abs(diff) <= HIT)[0]
        if hits.size:
            mat[i, hits[0]] = 1.0
        else:
            raw = weights / diff
            mat[i] = raw / raw.sum()
    return mat


def interp_dense(values, mats):
    """sum over the node box of prod_a mats[a][p, i_a] values[i_0, ..] -> (npts,)."""
    out = np.asarray(values, dtype=np.float64)
    # contract the last axis first: out[..., i_a] mats[a][p, i_a], keeping the point index in front
    d = len(mats)
    if d == 1:
        return np.einsum("na,a->n", mats[0], out)
    if d == 2:
        return np.einsum("na,nb,ab->n", mats[0], mats[1], out)
    return np.einsum("na,nb,nc,abc->n", mats[0], mats[1], mats[2], out)


def lebesgue(mats):
    """prod_a sum_k |w_a[k]| per point: how far the interpolant's rounding error is amplified over that of the node values."""
    out = np.ones(mats[0].shape[0])
    for m in mats:
        out = out * np.abs(m).sum(axis=1)
    return out


def outside_fraction(n):
    """How far outside the box (as a fraction of the box's width, 10 % at the most) the tests place points on an axis of n
    nodes.  The interpolant there is the degree n - 1 extrapolant, whose weights grow like T_{n-1}(1 + 2 f) ~
    cosh((n - 1) sqrt(4 f)): with (n - 1) sqrt(4 f) <= 1.5 the axis's Lebesgue sum stays below cosh(1.5) = 2.4 < the interior
    bound 1 + (2 / pi) ln n of n = 64, so a rounding-level tolerance relative to max |V| means outside what it means inside."""
    return min(0.1, (1.5 / (n - 1)) ** 2 / 4.0)


def kernel_points(axes, seed, n_uniform):
    """Targets of one kernel case: uniform in the box, every node of axis 0 (other coordinates uniform), all 2^d corners, node
    +- 3e-15 (one-hot branch), node + 5e-14 (division branch, raw weights ~ 1e13) and points outside the box by
    `outside_fraction` of its width -> (npts, d) with n_uniform + fixed rows; the caller trims or pads with uniform points."""
    rng = np.random.default_rng(seed)
    d = len(axes)
    lo = np.array([a[0] for a in axes])
    hi = np.array([a[-1] for a in axes])
    uni = lambda m: lo + (hi - lo) * rng.uniform(size=(m, d))          # noqa: E731
    rows = []
    p = uni(len(axes[0]))
    p[:, 0] = axes[0]
    rows.append(p)
    corners = np.array(np.meshgrid(*[[l, h] for l, h in zip(lo, hi)], indexing="ij")).reshape(d, -1).T
    rows.append(corners)
    for off in (3e-15, -3e-15, 5e-14):
        p = uni(4)
        for a in range(d):
            p[:, a] = rng.choice(axes[a], size=4) + off
        rows.append(p)
        q = uni(2 * d)                                                # one coordinate near a node, the others free
        for a in range(d):
            q[2 * a:2 * a + 2, a] = rng.choice(axes[a], size=2) + off
        rows.append(q)
    frac = np.array([outside_fraction(len(a)) for a in axes])
    out = uni(6)
    out[:3] = hi + (hi - lo) * frac * rng.uniform(0.2, 1.0, size=(3, d))
    out[3:5] = lo - (hi - lo) * frac * rng.uniform(0.2, 1.0, size=(2, d))
    out[5, 0] = hi[0] + (hi[0] - lo[0]) * frac[0]
    rows.append(out)
    fixed = np.concatenate(rows)
    return np.concatenate([uni(n_uniform), fixed]), fixed.shape[0]


# ---- stochastic route ----------------------------------------------------------------------------------------------------------
def se_weights(lengthscale, variance, h, mtot, d):
    """ws^2 = S(xi) h^d of the squared exponential kernel on the grid xi = h k: S = var (2 pi l^2)^(d/2) exp(-2 pi^2 l^2 |xi|^2)."""
    k = S.mode_grid(mtot, d)
    q = (float(h) * k).pow(2).sum(dim=1)
    dens = float(variance) * (2.0 * math.pi * float(lengthscale) ** 2) ** (d / 2.0) * torch.exp(-2.0 * math.pi ** 2 * float(lengthscale) ** 2 * q)
    return torch.sqrt(dens * float(h) ** d)


def reference_probes(n_probes, M, random_state):
    """The reference's seeded +-1 stream of the predictive variance: seed random_state + 2_000_000, float64 uniforms."""
    gen = torch.Generator(device="cpu").manual_seed(int(random_state) + 2_000_000)
    u = torch.rand((n_probes, M), generator=gen, dtype=torch.float64)
    return torch.floor(2.0 * u) * 2.0 - 1.0


def clamped_scale(ws):
    d2 = (ws * ws).real if ws.is_complex() else ws * ws
    floor = max(float(d2.mean()) * 1e-14, 1e-14)
    return torch.sqrt(torch.clamp(d2, min=floor)), d2


def stochastic_operator(X, delta, ws, h, mtot):
    """Dense A = I + Ds F^H diag(delta) F Ds (complex128, on X's device) and its 2-norm condition number from eigvalsh."""
    F = S.feature_matrix(X, h, mtot)
    ds, _ = clamped_scale(ws)
    M = F.shape[1]
    G = F.conj().T @ (delta.reshape(-1, 1).to(F.dtype) * F)
    A = ds.reshape(M, 1) * G * ds.reshape(1, M) + torch.eye(M, dtype=F.dtype, device=F.device)
    ev = torch.linalg.eigvalsh(A)
    return A, float(ev[-1] / ev[0])


def stochastic_dense(X, delta, ws, h, mtot, eta, X_new, A=None):
    """The stochastic variance at the rows of X_new from the probes eta (J, M), everything dense (torch, on X's device)."""
    d = X.shape[1]
    if A is None:
        A, _ = stochastic_operator(X, delta, ws, h, mtot)
    ds, d2 = clamped_scale(ws)
    y = torch.linalg.solve(A, (ds.reshape(1, -1) * eta).to(A.dtype).T).T
    gamma = (d2 / ds).reshape(1, -1) * y
    J = eta.shape[0]
    box, corr = (int(mtot),) * d, (2 * int(mtot) - 1,) * d
    dims = tuple(range(1, d + 1))
    # the correlation on the host: an odd transform length new to the process costs the GPU's FFT library a runtime compilation
    gf = torch.fft.fftn(gamma.cpu().reshape((J,) + box), s=corr, dim=dims)
    ef = torch.fft.fftn(eta.cpu().to(A.dtype).reshape((J,) + box), s=corr, dim=dims)
    sums = torch.fft.ifftn(gf * ef.conj(), s=corr, dim=dims).mean(dim=0).to(X.device)   # (2 mtot - 1)^d, lags in FFT order
    m = int(mtot)
    lag1 = torch.cat([torch.arange(0, m), torch.arange(-(m - 1), 0)]).to(torch.float64)
    lags = (lag1.reshape(-1, 1) if d == 1 else torch.cartesian_prod(*([lag1] * d))).to(X.device)
    ph = 2.0 * math.pi * float(h) * (X_new.to(torch.float64) @ lags.T)
    var = (torch.cos(ph) @ sums.reshape(-1).real - torch.sin(ph) @ sums.reshape(-1).imag)
    return var.clamp_min(0.0)


# ---- goldens -------------------------------------------------------------------------------------------------------------------
def load_case(case):
    """(fit golden pg_<case>.npz, variance golden variance_pg_<case>.npz)."""
    return np.load(os.path.join(GOLD, f"pg_{case}.npz")), np.load(os.path.join(GOLD, f"variance_pg_{case}.npz"))


_DTYPES = {"torch.float32": torch.float32, "torch.float64": torch.float64}
_FITS = {}


def fit_golden(case):
    """The classifier fitted on the GPU from pg_<case>.npz's inputs and settings, once per process."""
    if case not in _FITS:
        from polyagamma_classification import PolyagammaGPClassifier
        g, v = load_case(case)
        params = json.loads(str(g["params"]))
        params.update(device="cuda", store_history=True)
        prev = torch.get_default_dtype()
        torch.set_default_dtype(_DTYPES[str(g["torch_default_dtype"])])      # the dtype the reference's hyper-parameters lived in
        try:
            _FITS[case] = (g, v, PolyagammaGPClassifier(**params).fit(g["X"], g["y"]))
        finally:
            torch.set_default_dtype(prev)
    return _FITS[case]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(np.ravel(b)), 1e-300))
