"""The paired-lag Toeplitz products of cg_herm48_pairs_kernel (csrc/cg_herm.hip, round 9), restated in numpy.

For an output row k0 and an input row m >= 1 the per-frequency Hermitian Toeplitz product of tests/test_cg48_mixed_operator.py adds
c(k0 - m) G[m] + c(k0 + m) conj G[m], eight multiply-adds.  With G[m] = a + i b this is S a + i Q b,

    S(k0, m) = c(k0 - m) + c(k0 + m),      Q(k0, m) = c(k0 - m) - c(k0 + m),

four multiply-adds: Re += S.x a - Q.y b, Im += S.y a + Q.x b.  S and Q are rounded once, in the prologue, from the same c(l0, f1)
the 25-lag form holds (negative lags as conjugates, lag 0 real, lags beyond the Toeplitz vector zero); the m = 0 term is
c(k0) Re G[0] as before, and row 0 of the result is made real as before.

Held here: the product to the direct sum by the rule of tests/test_cg48_mixed_operator.py (at most 10 x as far from it as the
2-D FFT product on the 48 x 48 grid), the row-frequency <p, A p> on the paired Yh to the longdouble sum by the rule of
tests/test_cg48_freq_dot.py (at most 10 x the mode form's distance plus one ulp), and a whole Jacobi PCG to the same iteration
count as the 25-lag form on mtot 23, 21, 13, 5, 3, 1.
"""
import functools

import numpy as np
import pytest

import test_cg48_freq_dot as FD
from test_cg48_mixed_operator import F, NR, _coefficients, _direct, _fft2d48, _problem

SHAPES = [23, 21, 13, 5, 3, 1]


def _lag(cf, l):
    """c(l, f1), l = -11 .. 22, out of what the dense lanes of the 25-lag form hold (group a0 covers a0 - 11 .. a0 + 13)."""
    grp = 0 if l <= 13 else 3
    return cf[grp, :, l - 3 * grp + 11]


def _pair_tables(cf):
    """c0[k0][f1] = c(k0), S[k0][m - 1][f1], Q[k0][m - 1][f1]: real and imaginary parts rounded once each."""
    c0 = np.stack([_lag(cf, k0) for k0 in range(NR)])
    S = np.zeros((NR, NR - 1, F), dtype=np.complex128)
    Q = np.zeros((NR, NR - 1, F), dtype=np.complex128)
    for k0 in range(NR):
        for m in range(1, NR):
            cm, cp = _lag(cf, k0 - m), _lag(cf, k0 + m)
            S[k0, m - 1] = cm + cp
            Q[k0, m - 1] = cm - cp
    return c0, S, Q


def _product_pairs(cf, G):
    """Yh[k0][f1]: two statements for m = 0, four multiply-adds per (k0, m >= 1), the projection of row 0."""
    c0, S, Q = _pair_tables(cf)
    Yh = np.zeros((NR, F), dtype=np.complex128)
    for k0 in range(NR):
        re = c0[k0].real * G[0].real
        im = c0[k0].imag * G[0].real
        for m in range(1, NR):
            a, b = G[m].real, G[m].imag
            re = re + S[k0, m - 1].real * a
            im = im + S[k0, m - 1].imag * a
            re = re - Q[k0, m - 1].imag * b
            im = im + Q[k0, m - 1].real * b
        Yh[k0] = re + 1j * im
    Yh[0] = Yh[0].real
    return Yh


def _apply_pairs(cf, ws, p):
    """FD._apply with the paired products: A p on the rows k0 >= 0, and G, Yh of ws * p."""
    n = p.shape[0]
    h = (n - 1) // 2
    G = np.fft.fft(FD._rows(ws * p, n), axis=1)
    Yh = _product_pairs(cf, G)
    k1 = np.arange(-h, h + 1)
    y = np.fft.ifft(Yh, axis=1)[:h + 1][:, k1 % F]
    return ws[h:] * y + FD.SIG * p[h:], G, Yh


def _full(rows, n):
    h = (n - 1) // 2
    out = np.zeros((n, n), dtype=np.complex128)
    out[h:] = rows
    out[:h] = np.conj(rows[1:][::-1, ::-1])
    return out


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _direct_case(mtot):
    v, u = _problem(mtot, 100 + mtot)
    v, u = v.numpy(), u.numpy()
    return v, u, _direct(v, u), _fft2d48(v, u)


@pytest.mark.parametrize("mtot", SHAPES)
def test_lags_seen_from_both_ends_are_the_same_numbers(mtot):
    """_lag reads c(l) from group 0 or group 3; where both hold a lag they hold the same bits."""
    v, _, _, _ = _direct_case(mtot)
    cf = _coefficients(v, mtot)
    for l in range(-2, 14):
        assert np.array_equal(cf[0, :, l + 11], cf[3, :, l + 2])
    c0, S, Q = _pair_tables(cf)
    assert np.all(c0[0].imag == 0.0)
    # k0 = 0: c(-m) = conj c(m), so S is real and Q imaginary, exactly
    assert np.all(S[0].imag == 0.0) and np.all(Q[0].real == 0.0)


@pytest.mark.parametrize("mtot", SHAPES)
def test_paired_product_matches_direct_sum(mtot):
    v, u, ref, fft = _direct_case(mtot)
    h = (mtot - 1) // 2
    Ap, G, Yh = _apply_pairs(_coefficients(v, mtot), np.ones((mtot, mtot)), u)
    y = _full(Ap - FD.SIG * u[h:], mtot)
    Ap25, _, _ = FD._apply(_coefficients(v, mtot), np.ones((mtot, mtot)), u)
    y25 = _full(Ap25 - FD.SIG * u[h:], mtot)
    e_fft, e_pair, e_25 = _rel(fft, ref), _rel(y, ref), _rel(y25, ref)
    print(f"\nmtot {mtot}: against the direct sum: paired {e_pair:.2e}, 25 lags {e_25:.2e}, 2-D FFT on 48 x 48 {e_fft:.2e}")
    assert e_pair <= max(10.0 * e_fft, 1e-15), (e_pair, e_fft)


@pytest.mark.parametrize("kind", ["even", "odd_row0", "weights"])
@pytest.mark.parametrize("mtot", SHAPES)
def test_frequency_dot_on_the_paired_product(mtot, kind):
    v, ws, p = FD._vectors(mtot, kind)
    cf = _coefficients(v, mtot)
    Ap25, _, _ = FD._apply(cf, ws, p)
    Ap, G, Yh = _apply_pairs(cf, ws, p)
    modes = FD._dot_modes(p, Ap25)
    freq = FD._dot_freq(p, G, Yh)
    ref = FD._dot_longdouble(v, ws, p)
    e_modes, e_freq = abs(float(modes - ref)), abs(float(freq - ref))
    ulp = float(np.spacing(abs(float(ref))))
    print(f"\nmtot {mtot} {kind}: <p,Ap> = {float(ref):.6e}; modes (25 lags) off by {e_modes / ulp:.2f} ulp, "
          f"frequencies (paired) by {e_freq / ulp:.2f} ulp")
    assert e_freq <= 10.0 * e_modes + ulp, (e_freq, e_modes, ulp)


def _pcg(v, ws, b, tol, apply):
    """FD._pcg with the application as an argument and <p, A p> in the row-frequency domain."""
    n = b.shape[0]
    h = (n - 1) // 2
    cf = _coefficients(v, n)
    wgt = FD._wgt(n)
    dg = float(v[n - 1, n - 1].real) * ws[h:] ** 2 + FD.SIG
    x = np.zeros((h + 1, n), dtype=np.complex128)
    r = b[h:].copy()
    z = r / dg
    p = z.copy()
    rz = float(np.sum(wgt * (np.conj(r) * z).real))
    den = np.sqrt(float(np.sum(wgt * np.abs(r) ** 2))) + 1e-16
    for it in range(1, 2 * n * n + 1):
        pf = _full(p, n)
        Ap, G, Yh = apply(cf, ws, pf)
        alpha = rz / (FD._dot_freq(pf, G, Yh) + 1e-16)
        x += alpha * p
        r -= alpha * Ap
        if np.sqrt(float(np.sum(wgt * np.abs(r) ** 2))) / den < tol:
            break
        z = r / dg
        rzn = float(np.sum(wgt * (np.conj(r) * z).real))
        p = z + (rzn / (rz + 1e-16)) * p
        rz = rzn
    return _full(x, n), it


@pytest.mark.parametrize("mtot", SHAPES)
def test_whole_solve_takes_the_same_iterations_either_way(mtot):
    from test_gpu_cg_hermitian import _system
    v, T, ws, fy = _system(mtot, 17)
    v, ws = v.numpy(), ws.real.numpy().reshape(mtot, mtot)
    b = ws * fy.numpy().reshape(mtot, mtot)
    x_25, it_25 = _pcg(v, ws, b, 1e-8, FD._apply)
    x_p, it_p = _pcg(v, ws, b, 1e-8, _apply_pairs)
    print(f"\nmtot {mtot}: iterations: 25 lags {it_25}, paired {it_p}; solutions differ by {_rel(x_p, x_25):.2e}")
    assert it_25 == it_p
    assert _rel(x_p, x_25) <= 100 * 1e-8
