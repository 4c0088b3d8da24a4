"""The Lanczos mode of the single-launch CG kernels (EFGP_LANCZOS_BRANCH in csrc/cg_persistent.hip, reached through efgp_lanczos and
efgp_hip.ops.lanczos) written down from the definition, and the cases of tests/test_lanczos_host.py and tests/test_gpu_lanczos.py.

The recurrence (`recurrence`): q = z / |z|; per step v = A q - beta_prev q_prev, alpha = Re <q, v>, v -= alpha q, beta = |v|; the
step is recorded and the loop then stops if beta < 1e-12 (the reference project's rule, an absolute threshold), else
q_prev, q = q, v / beta.  It runs on three operators that are equal in exact arithmetic:

    dense f64     the dense matrix of tests/_dense_toeplitz.py, complex128 (`lanczos_dense(A, z, steps, numpy.complex128)`)
    dense 80-bit  the same matrix entries, every operation in numpy.clongdouble (`lanczos_dense(..., numpy.clongdouble)`)
    FFT f64       the oracle's circulant product (oracle.efgp_oracle.Toeplitz with make_A_mean / make_A_var) (`lanczos_fft`)

`distances` is the references' own disagreement per step, d_k; `prefix` the leading run of steps with d_k <= 1e-10: what a fourth
implementation can be held to.  `quadrature` is the Gauss-Lanczos value |z|^2 e_1^T log(T_K) e_1 of the recorded steps and
`exact_quadratic_form` the number it estimates, z^H log(A) z from the eigen-decomposition of the dense matrix.

A Krylov recurrence amplifies rounding once its space is nearly exhausted, so in f64 the break at beta < 1e-12 is only taken where
it comes within about three steps (BREAKDOWN below); later breaks are missed by every f64 implementation, the kernel included,
because the kernel copies the rule.  tests/test_lanczos_host.py measures which cases qualify.
"""
import functools
import math

import numpy as np
import torch

import _cg_routes as R
import _dense_toeplitz as D

BREAK = 1e-12                 # the reference project's absolute threshold on beta
PREFIX_TOL = 1e-10            # a step belongs to the compared prefix while the references agree to this (relative to |alpha_k|)
STEPS = 12                    # step-by-step comparisons: K = min(STEPS, M)
QUAD_STEPS = 25               # quadrature comparisons (the default of the log marginal likelihood)
EIGH_MAX = 1100               # the largest block whose dense eigen-decomposition a test pays for


def recurrence(apply, z, steps):
    """The three-term recurrence from the row z (numpy, complex128 or clongdouble) with `apply`: u -> A u in z's precision.
    -> (alpha (taken,), beta (taken,), |z|^2, taken) in the real type of z."""
    rt = z.real.dtype
    norm2 = (z.real * z.real + z.imag * z.imag).sum()
    q = z / np.sqrt(norm2)
    q_prev = np.zeros_like(q)
    beta_prev = rt.type(0)
    alpha, beta = [], []
    for _ in range(int(steps)):
        v = apply(q) - beta_prev * q_prev
        a = (q.conj() * v).sum().real
        v = v - a * q
        b = np.sqrt((v.real * v.real + v.imag * v.imag).sum())
        alpha.append(a)
        beta.append(b)
        if b < BREAK:
            break
        q_prev, beta_prev, q = q, b, v / b
    return np.array(alpha, dtype=rt), np.array(beta, dtype=rt), norm2, len(alpha)


def _np(t, dtype):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype)


def lanczos_dense(A, z, steps, dtype=np.complex128):
    """`steps` Lanczos steps on the dense matrix A from the row z, every operation in `dtype` (complex128 or clongdouble)."""
    a = _np(A, dtype)
    return recurrence(lambda u: a @ u, _np(z, dtype).reshape(-1), steps)


def lanczos_fft(s, variant, z, steps, ws=None):
    """The same loop on the oracle's FFT Toeplitz product of the system s (f64); ws: in place of the system's own."""
    from oracle import efgp_oracle as O
    w = s["ws"] if ws is None else ws
    Af = (O.make_A_mean if variant == 0 else O.make_A_var)(w, O.Toeplitz(s["v"]), s["sigmasq"])
    return recurrence(lambda u: Af(torch.from_numpy(u)).numpy(), _np(z, np.complex128).reshape(-1), steps)


def distances(ref, other):
    """d_k = max(|alpha_k - alpha'_k|, |beta_k - beta'_k|) / |alpha_k| on the steps both took; float64 (k,)."""
    k = min(ref[3], other[3])
    a, b = ref[0][:k].astype(np.longdouble), ref[1][:k].astype(np.longdouble)
    d = np.maximum(np.abs(a - other[0][:k]), np.abs(b - other[1][:k])) / np.abs(a)
    return d.astype(np.float64)


def prefix(d):
    """Length of the leading run of steps with d_k <= PREFIX_TOL."""
    bad = np.nonzero(~(d <= PREFIX_TOL))[0]
    return int(bad[0]) if bad.size else len(d)


def references(A, s, variant, z, steps, ws=None):
    """The three references of one probe -> dict(f64, fft, ld: the (alpha, beta, norm2, taken) of each; d (k,): the larger of the two
    distances from dense f64 per step; prefix: the compared steps)."""
    f64 = lanczos_dense(A, z, steps, np.complex128)
    fft = lanczos_fft(s, variant, z, steps, ws)
    ld = lanczos_dense(A, z, steps, np.clongdouble)
    k = min(f64[3], fft[3], ld[3])
    d = np.maximum(distances(f64, fft)[:k], distances(f64, ld)[:k])
    return dict(f64=f64, fft=fft, ld=ld, d=d, prefix=prefix(d))


def quadrature(alpha, beta, norm2):
    """norm2 * e_1^T log(T_K) e_1, T_K the tridiagonal matrix of the recorded steps (beta_i couples steps i and i + 1; the last
    recorded beta is not part of it)."""
    a = np.asarray(alpha, dtype=np.float64)
    b = np.asarray(beta, dtype=np.float64)
    k = len(a)
    T = np.diag(a) + np.diag(b[:k - 1], 1) + np.diag(b[:k - 1], -1)
    lam, U = np.linalg.eigh(T)
    return float(norm2) * float((U[0, :] ** 2 * np.log(lam)).sum())


@functools.lru_cache(maxsize=2)
def _eigh(ns, variant, ws_key):
    A = matrix(ns, variant, ws_key)
    a = A.numpy()
    return np.linalg.eigh(0.5 * (a + a.conj().T))


def exact_quadratic_form(A, z):
    """z^H log(A) z = sum_i |u_i^H z|^2 log lambda_i from eigh of the dense Hermitian A (a tensor, or the (lambda, U) of one)."""
    if isinstance(A, tuple):
        lam, U = A
    else:
        a = _np(A, np.complex128)
        lam, U = np.linalg.eigh(0.5 * (a + a.conj().T))
    c = U.conj().T @ _np(z, np.complex128).reshape(-1)
    return float(((c.real ** 2 + c.imag ** 2) * np.log(lam)).sum())


# ---- operators ------------------------------------------------------------------------------------------------------------------
def low_rank_ws(ns, rank, seed=3):
    """ws that is non-zero (the system's own values) at `rank` random modes of the block: A_var = I + a matrix of that rank, so a
    Krylov space of dimension rank + 1 at the most."""
    M = math.prod(ns)
    g = torch.Generator().manual_seed(seed)
    keep = torch.randperm(M, generator=g)[:rank]
    w = torch.zeros(M, dtype=torch.complex128)
    w[keep] = D.system(ns)["ws"][keep]
    return w


def weights(ns, ws_key):
    """ws_key: "own" (the system's), "zero", "rank1", "rank3", ..."""
    if ws_key == "own":
        return D.system(ns)["ws"]
    if ws_key == "zero":
        return torch.zeros(math.prod(ns), dtype=torch.complex128)
    assert ws_key.startswith("rank")
    return low_rank_ws(ns, int(ws_key[4:]))


@functools.lru_cache(maxsize=2)
def _other_matrix(ns, variant, ws_key):
    s = D.system(ns)
    return D.dense_A(s["v"], weights(ns, ws_key), s["sigmasq"], variant)


def matrix(ns, variant, ws_key="own"):
    """The dense A of the block, cached for the case at hand (its two variants): system_A for the system's own ws."""
    return D.system_A(ns, False, variant) if ws_key == "own" else _other_matrix(ns, variant, ws_key)


def eigen(ns, variant, ws_key="own"):
    """(lambda, U) of matrix(...), cached the same way."""
    return _eigh(ns, variant, ws_key)


# ---- probes ---------------------------------------------------------------------------------------------------------------------
def probes(ns, nreal=2, ncomplex=2, seed=11):
    """(nreal + ncomplex, M) complex128: rows of +-1 first, then complex normal rows; a function of the block alone."""
    M = math.prod(ns)
    g = torch.Generator().manual_seed(7919 * seed + 31 * len(ns) + sum((a + 1) * n for a, n in enumerate(ns)))
    real = torch.randint(0, 2, (nreal, M), generator=g).to(torch.float64) * 2 - 1
    cplx = torch.complex(torch.randn(ncomplex, M, generator=g, dtype=torch.float64), torch.randn(ncomplex, M, generator=g, dtype=torch.float64))
    return torch.cat([real.to(torch.complex128), cplx], 0)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# the distinct blocks of the dense CG cases the Lanczos mode takes, with the kernel it runs on: Lanczos bars line1d, herm64 and
# herm48 and ignores the Hermitian promise, so the _herm duplicates collapse and 1-D blocks and odd squares run the general kernels
def _cases():
    out = {}
    for name, (ns, _, _) in R.DENSE.items():
        kernel = R.route(ns, lanczos=True)[0]
        if kernel in ("generic", "2d64") and ns not in [c[0] for c in out.values()]:
            out[name[:-5] if name.endswith("_herm") else name] = (ns, kernel)
    return out


CASES = _cases()
# what the list must be, written out (tests/test_lanczos_host.py::test_lanczos_routes holds both to route(ns, lanczos=True))
ROUTES = {
    "1d_2": "generic", "1d_3": "generic", "1d_4": "generic", "1d_255": "generic", "1d_256": "generic", "1d_700": "generic",
    "1d_2048": "generic",
    "2d_2x3": "generic", "2d_8x64": "generic", "2d_64x16": "generic", "2d_4x256": "generic", "2d_16x17": "generic",
    "2d_20x30": "generic", "2d_1x37": "generic", "2d_37x1": "generic",
    "sq_2": "2d64", "sq_8": "2d64", "sq_16": "2d64", "sq_24": "2d64", "sq_32": "2d64", "sq_23": "2d64", "sq_25": "2d64", "sq_31": "2d64",
    "3d_2x3x5": "generic", "3d_4x8x16": "generic", "3d_16x4x8": "generic", "3d_8x16x4": "generic", "3d_8x8x8": "generic",
    "3d_3x7x9": "generic", "3d_1x7x7": "generic", "3d_7x1x7": "generic", "3d_1x20x20": "generic", "3d_1x1x9": "generic",
}
# blocks efgp_lanczos refuses (ops.lanczos returns None): no single-launch kernel takes them
REFUSED = {name: R.CASES[name][0] for name in ("1d_1", "2d_30x50", "3d_5x7x12", *R.ORACLE)}

# Breakdown: (block, ws, steps taken) of the cases in which all three references break at the same step with the last beta below
# 1e-13, ten times under the threshold (variant 1: the threshold is absolute, and at sigma^2 = 150 variant 0 does not reach it
# reliably).  Asserted on the CPU by tests/test_lanczos_host.py::test_breakdown_cases_qualify.
BREAKDOWN = {
    "zero_ws_8x8": ((8, 8), "zero", 1),
    "rank1_8x8": ((8, 8), "rank1", 2),
    "rank1_20x30": ((20, 30), "rank1", 2),
    "own_2": ((2,), "own", 2),
    "own_3": ((3,), "own", 3),
    "own_1x1x3": ((1, 1, 3), "own", 3),
}
# ... and not (2, 2), (2, 3), weights(ns, "rank3") on (2, 3, 5) or weights(ns, "rank4") on (700,): four and more steps in, the f64
# references sit within a factor of ten of the threshold or miss the break (figures in tests/test_lanczos_host.py)
