"""The operator application of cg_herm48_kernel (csrc/cg_herm.hip, DENSE), restated in numpy.

The Toeplitz product Y(k) = sum_k' v(k - k') g(k') of a conjugate-even g on a block of n x n modes (n <= 23) needs a transform
in ONE dimension only: after the row transforms G[k0][f1] = sum_k1 g(k0, k1) w48^(f1 k1) the convolution over k0 is, for every
f1, a Hermitian Toeplitz product with the coefficients c(l0, f1) = sum_l1 v(l0, l1) w48^(f1 l1), c(-l0, f1) = conj c(l0, f1).
The kernel keeps rows k0 >= 0 only (G[-k0][f1] = conj G[k0][f1]), gives each lane three output rows a0 .. a0 + 2 (a0 = 0, 3, 6, 9)
of one frequency and the 25 lags a0 - 11 .. a0 + 13 they need, and drops the imaginary part of row 0 on the way in and out.

This file states that indexing and checks it against the direct sum: the mixed form may be at most 10 x as far from it as the
2-D FFT product on the same 48 x 48 grid is (the application it replaces), and agrees with oracle.efgp_oracle.Toeplitz.
"""
import numpy as np
import pytest
import torch

F, NR, NC = 48, 12, 25


def _problem(mtot, seed):
    from oracle import efgp_oracle as O
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(300, 2, generator=g, dtype=torch.float64) * 2 - 1
    v = O.conv_vector(x, 0.4, (mtot - 1) // 2)                     # (2 n - 1)^2 lags, lag l at index l + n - 1
    u = torch.complex(torch.randn(mtot, mtot, generator=g, dtype=torch.float64), torch.randn(mtot, mtot, generator=g, dtype=torch.float64))
    u = 0.5 * (u + torch.flip(u, dims=(0, 1)).conj())              # conjugate-even: coefficients of a real function
    return v, u


def _direct(v, u):
    n = u.shape[0]
    y = np.zeros((n, n), dtype=np.complex128)
    for a in range(n):
        for b in range(n):
            # v(k - k') for all k': lags a - a', b - b' at indices a - a' + n - 1, ...
            y[a, b] = np.sum(v[a + n - 1 - np.arange(n)][:, b + n - 1 - np.arange(n)] * u)
    return y


def _fft2d48(v, u):
    n = u.shape[0]
    y = np.fft.ifft2(np.fft.fft2(v, s=(F, F)) * np.fft.fft2(u, s=(F, F)))
    return y[n - 1:2 * n - 1, n - 1:2 * n - 1]


def _coefficients(v, n):
    """cf[a0 // 3][f1][i] = c(a0 - 11 + i, f1): what the dense lane (f1, a0) holds.  Only lags l0 >= 0 are taken from the row
    transform of v; negative lags are their conjugates, lag 0 is real, lags beyond the Toeplitz vector are zero."""
    phase = np.exp(2j * np.pi * ((np.arange(F) * (n - 1)) % F) / F)       # centred lags along l1 (exponent reduced mod 48, as the kernel's table)
    rows = np.fft.fft(v, n=F, axis=1) * phase[None, :]
    cf = np.zeros((4, F, NC), dtype=np.complex128)
    for grp in range(4):
        for i in range(NC):
            l = 3 * grp - 11 + i
            if abs(l) <= n - 1:
                c = rows[abs(l) + n - 1]
                cf[grp, :, i] = np.conj(c) if l < 0 else (c.real if l == 0 else c)
    return cf


def _mixed(v, u):
    n = u.shape[0]
    h = (n - 1) // 2
    # A: rows k0 = 0..11 (zero beyond h), modes k1 at positions k1 mod 48
    g = np.zeros((NR, F), dtype=np.complex128)
    for k0 in range(h + 1):
        for k1 in range(-h, h + 1):
            g[k0, k1 % F] = u[k0 + h, k1 + h]
    G = np.fft.fft(g, axis=1)
    cf = _coefficients(v, n)
    Yh = np.zeros((NR, F), dtype=np.complex128)
    for grp in range(4):
        for o in range(3):
            acc = cf[grp, :, 11 + o] * G[0].real
            for m in range(1, NR):
                acc = acc + cf[grp, :, 11 + o - m] * G[m] + cf[grp, :, 11 + o + m] * np.conj(G[m])
            Yh[3 * grp + o] = acc
    Yh[0] = Yh[0].real
    # D: inverse row transforms, crop, mirror
    yr = np.fft.ifft(Yh, axis=1)
    y = np.zeros((n, n), dtype=np.complex128)
    for k0 in range(h + 1):
        for k1 in range(-h, h + 1):
            y[k0 + h, k1 + h] = yr[k0, k1 % F]
            if k0 > 0:
                y[h - k0, h - k1] = np.conj(yr[k0, k1 % F])
    return y


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("mtot", [23, 21, 13, 5, 3, 1])
def test_mixed_operator_matches_direct_sum_and_oracle(mtot):
    from oracle import efgp_oracle as O
    v, u = _problem(mtot, 100 + mtot)
    ref = _direct(v.numpy(), u.numpy())
    e_fft = _rel(_fft2d48(v.numpy(), u.numpy()), ref)
    y = _mixed(v.numpy(), u.numpy())
    e_mix = _rel(y, ref)
    yo = O.Toeplitz(v)(u.reshape(-1)).reshape(mtot, mtot).numpy()
    e_o = _rel(yo, ref)
    print(f"\nmtot {mtot}: against the direct sum: mixed {e_mix:.2e}, 2-D FFT on 48 x 48 {e_fft:.2e}, oracle {e_o:.2e}")
    bound = max(10.0 * e_fft, 1e-15)
    assert e_mix <= bound, (e_mix, e_fft)
    assert _rel(y, yo) <= bound + e_o, (_rel(y, yo), bound, e_o)


def test_coefficients_are_hermitian_in_the_lag():
    v, _ = _problem(23, 7)
    cf = _coefficients(v.numpy(), 23)
    # lane (f1, a0 = 0) holds lags -11..13: c(-l) = conj c(l) exactly, c(0) real
    assert np.array_equal(cf[0, :, 11 - 5], np.conj(cf[0, :, 11 + 5]))
    assert np.all(cf[0, :, 11].imag == 0.0)
    # the same lag seen from two groups is the same number: lag 2 is i = 13 for a0 = 0 and i = 4 for a0 = 9
    assert np.array_equal(cf[0, :, 13], cf[3, :, 4])
