"""References and restated host rules of tests/test_gpu_helper_seams.py, written from the definitions (numpy / torch on the host
in float64; no product code).

Slab rules (restated from the entries so that a test can assert that its shape really crosses the seam it is named for):
  lag sums        probes per slab = min(65535, 2^28 / (32 P)), P the padded lag box (csrc/variance_ops.hip: lag_sums_general); the
                  64 x 64 route of 2-D mtot <= 32 has P = 4096
  Toeplitz apply  rows per slab   = min(65535, 2^28 / (16 Ftot))           (csrc/toeplitz_cg.hip: efgp_toeplitz_apply[_scaled])
  multi-launch CG systems per group = min(65535, 2^29 / (16 Ftot))         (csrc/cg_multi.hip: solve_multi_launch)
  gridDim.y       at most 65535 rows per launch
"""
import math

import numpy as np
import torch

GRID_ROWS = 65535
_CD = torch.complex128


def crandn(shape, g):
    return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))


def bits(t):
    """The bit patterns of a float64 / complex128 tensor (so that -0.0 and NaN payloads compare as they are stored)."""
    t = t.detach().cpu().contiguous()
    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int64)


# ---- lag sums ---------------------------------------------------------------------------------------------------------------------
def lag_length(s):
    """Transform length of a lag axis of 2 n - 1 = s lags: the next 2^k or 3 * 2^(k-1) (csrc/variance_ops.hip: lag_length)."""
    p2 = 1
    while True:
        if p2 >= s:
            return p2
        if p2 >= 2 and p2 + p2 // 2 >= s:
            return p2 + p2 // 2
        p2 *= 2


def lag_box(shape):
    """Padded lag box P of a mode box."""
    return math.prod(lag_length(2 * n - 1) for n in shape)


def lag_probes_per_slab(P):
    return max(1, min(GRID_ROWS, (1 << 28) // (32 * P)))


def lag_reference(gam, eta, shape):
    """c[r] = mean_j sum_{k - l = r} gamma_j[k] eta_j[l] on the (2 n_a - 1) box in FFT order: the torch.fft correlation of
    tests/test_gpu_variance_ops.py::test_lag_sums_match_fft_correlation (efgpnd.py:1660-1664), on the host."""
    J = gam.shape[0]
    shp = (J,) + tuple(shape)
    s = tuple(2 * n - 1 for n in shape)
    dims = tuple(range(1, len(shape) + 1))
    G = torch.fft.fftn(gam.reshape(shp), s=s, dim=dims)
    E = torch.fft.fftn(eta.reshape(shp).to(_CD), s=s, dim=dims)
    return torch.fft.ifftn(G * torch.conj(E), s=s, dim=dims).mean(dim=0)


def lag_problem(shape, J, seed):
    g = torch.Generator().manual_seed(seed)
    M = math.prod(shape)
    gam = crandn((J, M), g)
    eta = (torch.randint(0, 2, (J, M), generator=g) * 2 - 1).to(torch.float64)
    return gam, eta


# ---- Toeplitz product -------------------------------------------------------------------------------------------------------------
def toeplitz_rows_per_slab(Ftot):
    return max(1, min(GRID_ROWS, (1 << 28) // (16 * Ftot)))


def cg_systems_per_group(Ftot):
    return max(1, min(GRID_ROWS, (1 << 29) // (16 * Ftot)))


def toeplitz_reference(v, u):
    """y[i] = sum_j v[i - j + n - 1] u[j] per axis for rows u (R, M): the zero-padded torch.fft product on the host.  The linear
    convolution of the (2 n - 1) lags with the n-box has 3 n - 2 entries per axis; the product is its window [n - 1, 2 n - 1)."""
    v = v.detach().cpu().to(_CD)
    ns = [(L + 1) // 2 for L in v.shape]
    d = v.ndim
    R = u.shape[0]
    uu = u.detach().cpu().to(_CD).reshape([R] + ns)
    s = tuple(L + n - 1 for L, n in zip(v.shape, ns))
    dims = tuple(range(1, d + 1))
    conv = torch.fft.ifftn(torch.fft.fftn(v, s=s)[None] * torch.fft.fftn(uu, s=s, dim=dims), dim=dims)
    window = (slice(None),) + tuple(slice(n - 1, 2 * n - 1) for n in ns)
    return conv[window].reshape(R, -1)


def rel_rows(got, ref):
    """max |got - ref| / max |ref| over the given rows."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


# ---- generated rows ---------------------------------------------------------------------------------------------------------------
_MASK = (1 << 64) - 1
ROW_STRIDE = 0xD1342543DE82EF95          # csrc/nufft_dev.hpp: kRademacherRowStride


def mix64(z):
    """The splitmix64 finaliser of the counter-based generators (csrc/nufft_dev.hpp: efgp_mix64), in Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def rademacher(seed, row, n, index_offset=0):
    """The +-1 probe of (seed, row, point n + index_offset): the sign bit of a hash of row * stride + n in wrapping arithmetic."""
    r = mix64((seed & _MASK) ^ mix64((row * ROW_STRIDE + n + index_offset) & _MASK))
    return 1.0 if r >> 63 else -1.0


# ---- mode phases ------------------------------------------------------------------------------------------------------------------
def features(x, hs, shape):
    """(B, M) complex128: exp(2 pi i sum_a h_a k_a x_a) on the box `shape`, k_a = i_a - (n_a - 1) // 2, last axis fastest
    (efgpnd.py:1808-1811 with a spacing per axis)."""
    axes = [h * (torch.arange(n, dtype=torch.float64) - (n - 1) // 2) for h, n in zip(hs, shape)]
    xis = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, len(shape))
    ang = 2 * math.pi * (x @ xis.T)
    return torch.polar(torch.ones_like(ang), ang)


# ---- exact inner products ---------------------------------------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a                   # 2^27 + 1: Veltkamp's split of a double into two 26-bit halves
    hi = c - (c - a)
    return hi, a - hi


def exact_products(a, b):
    """(p, e) with a_i b_i = p_i + e_i exactly (Dekker's product; no overflow or underflow at the magnitudes the tests use)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_vdot_real(a, b):
    """(Re sum conj(a_i) b_i, sum |a_i| |b_i|) for real or complex host tensors: math.fsum of the exact products."""
    a = a.detach().cpu()
    b = b.detach().cpu()
    ar, ai = (a.real, a.imag) if a.is_complex() else (a, None)
    br, bi = (b.real, b.imag) if b.is_complex() else (b, None)
    terms = list(exact_products(ar.numpy(), br.numpy()))
    if ai is not None and bi is not None:
        terms += list(exact_products(ai.numpy(), bi.numpy()))
    total = math.fsum(np.concatenate(terms).tolist()) if a.numel() else 0.0
    mag = math.fsum((a.abs() * b.abs()).tolist()) if a.numel() else 0.0
    return total, mag


def signed_wide(n, g, complex_):
    """n values of both signs whose magnitudes span 1e-3 .. 1e3 (a 1e6 dynamic range)."""
    def real():
        mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 6.0 - 3.0)
        sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).to(torch.float64)
        return mag * sign
    return torch.complex(real(), real()) if complex_ else real()
