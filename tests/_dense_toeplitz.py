"""The CG systems of csrc/cg_persistent.hip, csrc/cg_herm.hip, csrc/cg_coop2d.hip and csrc/cg_multi.hip (operator: csrc/toeplitz_cg.hip) written down from the definition: the block Toeplitz matrix as a
dense M x M array, A = D T D + sigma^2 I (variant 0) or D T D / sigma^2 + I (variant 1), a direct solve, and the oracle's CG loops
(oracle/efgp_oracle.py: cg_single, cg_batched) driven by the dense matrix product -- no FFT, no circulant embedding anywhere.

Every kernel and the oracle's own Toeplitz apply the operator through a circulant embedding; this file is the second construction.
tests/test_dense_toeplitz_host.py ties it to the oracle and to the point sums on a machine without a GPU.

The systems (`system`): the Toeplitz vector of 400 random points by the definition (T positive semi-definite, as a model's),
ws = exp(-2.5 U), sigma^2 = 150 and the Jacobi diagonal 400 |ws|^2 + sigma^2: condition numbers of about 10, up to 34 iterations at
tol = 1e-8 up to M = 2048.

Why sigma^2 = 150 and not 4.  A test that compares iteration counts needs a system whose stopping index is a property of the
system, not of the rounding of one implementation.  At sigma^2 = 4 (condition numbers 1e2..3e2, 40..280 iterations, more than M of
them on the small blocks) it is not: this file's CG on the dense matrix and the oracle's CG on its FFT product -- equal in exact
arithmetic, 1e-15 apart per product -- disagree on the count in 4 of 11 cases looked at, by up to 2, and their residual histories
differ by up to 30 % (CG past the loss of orthogonality amplifies the rounding of a product by 1e14).  The same holds at 30 or 60 points.
At sigma^2 = 40 the counts agree but the histories still differ by 40 %; at 150 they agree to 3e-5 and every count is equal.
tests/test_dense_toeplitz_host.py::test_stopping_index_is_decided_by_the_system asserts that agreement on the CPU for every case.
The long solves are still run, one per route at sigma^2 = 4 (LONG_SIGMASQ), judged on what does not depend on the count: the true
residual and the distance to the direct solve.
"""
import functools
import math

import numpy as np
import torch

H = (0.31, 0.27, 0.23)        # mode spacing per axis
NPTS = 400
SIGMASQ = 150.0
LONG_SIGMASQ = 4.0            # the ill-conditioned systems of the long solves: cond 1e2..3e2, 40..280 iterations
DENSE_MAX = 2048              # the largest block a dense reference is built for


def dense_T(v):
    """v: complex tensor of shape (2 n_a - 1) per axis -> the M x M complex128 matrix T[i, j] = v[i - j + n - 1] per axis, rows and
    columns row-major over the block (d = 1..3)."""
    v = torch.as_tensor(v).to(torch.complex128)
    d = v.ndim
    ns = [(L + 1) // 2 for L in v.shape]
    ix = []
    for a, n in enumerate(ns):
        lag = torch.arange(n)[:, None] - torch.arange(n)[None, :] + n - 1          # (i_a, j_a)
        shape = [1] * (2 * d)
        shape[a], shape[d + a] = n, n
        ix.append(lag.reshape(shape))
    M = math.prod(ns)
    return v[tuple(ix)].reshape(M, M)


def dense_A(v, ws, sigmasq, variant):
    """D T D + sigma^2 I (variant 0) or D T D / sigma^2 + I (variant 1), D = diag(ws); complex128 (M, M)."""
    T = dense_T(v)
    w = torch.as_tensor(ws).to(torch.complex128).reshape(-1)
    DTD = w[:, None] * T * w[None, :]
    eye = torch.eye(T.shape[0], dtype=torch.complex128)
    return DTD + sigmasq * eye if variant == 0 else DTD / sigmasq + eye


def matvec(A):
    """u (M,) or (B, M) -> A u per row: the operator argument of the oracle's CG loops."""
    At = A.T.contiguous()
    return lambda u: u @ At


def direct_solve(A, b):
    """numpy.linalg.solve per row of b ((M,) or (B, M))."""
    bb = torch.as_tensor(b).to(torch.complex128)
    x = np.linalg.solve(A.numpy(), bb.reshape(-1, A.shape[0]).numpy().T).T
    return torch.from_numpy(np.ascontiguousarray(x)).reshape(bb.shape)


def cond(A):
    """2-norm condition number of the dense matrix: from its eigenvalues where A is Hermitian (ws real), else from its singular values."""
    a = A.numpy()
    if np.abs(a - a.conj().T).max() <= 1e-14 * np.abs(a).max():          # Hermitian up to the rounding of w_i T_ij w_j
        w = np.abs(np.linalg.eigvalsh(0.5 * (a + a.conj().T)))
        return float(w.max() / w.min())
    return float(np.linalg.cond(a))


def cg_dense(A, b, x0, tol, max_iter=None, early=True, diag=None):
    """The oracle's cg_single (b (M,)) or cg_batched (b (B, M)) on the dense matrix -> (x, iterations)."""
    from oracle import efgp_oracle as O
    fn = O.cg_single if b.ndim == 1 else O.cg_batched
    return fn(matvec(A), b, x0 if x0 is not None else torch.zeros_like(b), tol, max_iter=max_iter, early=early, diag=diag)


def row_counts(A, b, tol, diag=None):
    """Per-row iteration counts of a converged batched solve from a zero start; A: the operator (u -> A u on (B, M)).  The rows of
    cg_batched are independent, so a row's count is that of the row solved alone, less the terminating pass cg_batched counts
    (cg.py:243).  Two passes beyond the solvers' default cap of 2 M, so that a row that stops at the cap still ends on the empty
    pass; every row must have converged."""
    from oracle import efgp_oracle as O
    cap = 2 * b.shape[1]
    counts = []
    for r in range(b.shape[0]):
        xr, it = O.cg_batched(A, b[r:r + 1], torch.zeros_like(b[r:r + 1]), tol, max_iter=cap + 2, diag=diag)
        assert it - 1 <= cap and float(torch.linalg.norm(A(xr) - b[r:r + 1])) <= tol * float(torch.linalg.norm(b[r])), "row not converged"
        counts.append(it - 1)
    return counts


def conv_vector(x, ns, h=H):
    """v[k] = sum_p exp(-2 pi i sum_a h_a k_a x_pa), k_a = -(n_a - 1) .. n_a - 1: shape (2 n_a - 1) per axis, from the definition."""
    d = len(ns)
    E = [torch.exp(-2j * math.pi * h[a] * torch.arange(-(n - 1), n, dtype=torch.float64)[:, None] * x[None, :, a]) for a, n in enumerate(ns)]
    if d == 1:
        return E[0].sum(1)
    if d == 2:
        return (E[0] @ E[1].T).contiguous()
    return torch.einsum("ip,jp,kp->ijk", E[0], E[1], E[2]).contiguous()


def _flip_all(t, first):
    return torch.flip(t, dims=tuple(range(first, t.ndim)))


@functools.lru_cache(maxsize=8)
def system(ns, hermitian=False, nb=3, seed=0, sigmasq=SIGMASQ):
    """-> dict(v, ws, b (nb, M) with row 1 zero, x0 (nb, M) 0.1-scaled, diag, sigmasq, ns) for the block `ns` (d = 1..3); points, ws
    and rows do not depend on sigmasq.
    hermitian: ws real and even, b and x0 conjugate-even under k -> -k (index reversal on every axis): transforms of real data."""
    ns = tuple(int(n) for n in ns)
    d = len(ns)
    g = torch.Generator().manual_seed(1000 * seed + 97 * d + sum((a + 1) * n for a, n in enumerate(ns)))
    x = torch.rand(NPTS, d, generator=g, dtype=torch.float64) * 2 - 1
    v = conv_vector(x, ns)
    w = torch.exp(-2.5 * torch.rand(*ns, generator=g, dtype=torch.float64))

    def rows(scale):
        t = torch.complex(torch.randn(nb, *ns, generator=g, dtype=torch.float64), torch.randn(nb, *ns, generator=g, dtype=torch.float64))
        if hermitian:
            t = 0.5 * (t + _flip_all(t, 1).conj())
        return scale * t.reshape(nb, -1)

    if hermitian:
        w = 0.5 * (w + _flip_all(w, 0))
    b = rows(1.0)
    x0 = rows(0.1)
    if nb > 1:
        b[1] = 0.0
        x0[1] = 0.0
    ws = w.reshape(-1).to(torch.complex128)
    diag = NPTS * ws.abs().pow(2).real + sigmasq
    return dict(v=v, ws=ws, b=b, x0=x0, diag=diag, sigmasq=sigmasq, ns=ns, points=x)


@functools.lru_cache(maxsize=2)
def system_A(ns, hermitian, variant, sigmasq=SIGMASQ):
    """The dense matrix of system(ns, hermitian), left unchanged.  Cached for the case at hand only (its two variants): the tests
    walk the cases one after the other, and a matrix of M = 2048 is 64 MB."""
    s = system(ns, hermitian, sigmasq=sigmasq)
    return dense_A(s["v"], s["ws"], s["sigmasq"], variant)
