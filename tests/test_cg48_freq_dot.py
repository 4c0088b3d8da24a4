"""<p, A p> of cg_herm48_kernel (csrc/cg_herm.hip, FREQ_DOT) in the row-frequency domain, restated in numpy.

A = ws T ws + sigma^2 with ws real, so <p, A p> = sigma^2 <p, p> + <ws p, T ws p>.  The kernel keeps rows k0 >= 0 on 48 positions,
weighs row 0 once and the others twice, and applies T as row transforms G[k0][f1], per-frequency Toeplitz products Yh[k0][f1] and
inverse row transforms (tests/test_cg48_mixed_operator.py).  A row is supported on the 23 modes, so by Parseval along k1

    <ws p, T ws p> = sum_f1 [ Re G[0][f1] Yh[0][f1] + 2 sum_{k0 >= 1} Re(conj G[k0][f1] Yh[k0][f1]) ]

with the 1 / 48 of the inverse transform inside Yh.  Row 0 holds the modes +k1 and -k1 both and is projected on the way in (Re G[0])
and out (Yh[0] real): the identity holds for an iterate with a conjugate-odd part in row 0 as well.  Both forms are held to the
same sum in numpy.longdouble: the frequency form may be at most 10 x as far from it as the mode form, plus one ulp of the value
(the rule of tests/test_cg48_mixed_operator.py for the operator), and a whole preconditioned solve takes the same number of
iterations either way.
"""
import numpy as np
import pytest
import torch

from test_cg48_mixed_operator import F, NR, _coefficients, _problem

SIG = 0.25


def _rows(u, n):
    """rows k0 = 0..11 (zero beyond h) on 48 positions, modes k1 at k1 mod 48"""
    h = (n - 1) // 2
    g = np.zeros((NR, F), dtype=u.dtype)
    k1 = np.arange(-h, h + 1)
    g[:h + 1, k1 % F] = u[h:, :]
    return g


def _apply(cf, ws, p):
    """The kernel's application on the stored rows: A p on rows k0 >= 0 (n // 2 + 1, n), and G, Yh of ws * p."""
    n = p.shape[0]
    h = (n - 1) // 2
    G = np.fft.fft(_rows(ws * p, n), axis=1)
    Yh = np.zeros((NR, F), dtype=np.complex128)
    for grp in range(4):
        for o in range(3):
            acc = cf[grp, :, 11 + o] * G[0].real
            for m in range(1, NR):
                acc = acc + cf[grp, :, 11 + o - m] * G[m] + cf[grp, :, 11 + o + m] * np.conj(G[m])
            Yh[3 * grp + o] = acc
    Yh[0] = Yh[0].real
    yr = np.fft.ifft(Yh, axis=1)
    k1 = np.arange(-h, h + 1)
    y = yr[:h + 1][:, k1 % F]
    return ws[h:] * y + SIG * p[h:], G, Yh


def _wgt(n):
    h = (n - 1) // 2
    return np.where(np.arange(h + 1) == 0, 1.0, 2.0)[:, None]


def _dot_modes(p, Ap):
    n = p.shape[0]
    return float(np.sum(_wgt(n) * (np.conj(p[(n - 1) // 2:]) * Ap).real))


def _dot_freq(p, G, Yh):
    n = p.shape[0]
    pp = float(np.sum(_wgt(n) * np.abs(p[(n - 1) // 2:]) ** 2))
    # (the kernel's coefficients carry the inverse transform's 1 / 48; here it sits in np.fft.ifft, so it is applied to the sum)
    t = np.sum(G[0].real * Yh[0].real) + 2.0 * np.sum((np.conj(G[1:]) * Yh[1:]).real)
    return SIG * pp + float(t) / F


def _dot_longdouble(v, ws, p):
    """The same sum in extended precision: the direct Toeplitz sum on the iterate the kernel's rows stand for (rows k0 > 0 and their
    mirror images, row 0 projected onto its conjugate-even part)."""
    n = p.shape[0]
    h = (n - 1) // 2
    L, C = np.longdouble, np.clongdouble
    pe = p.astype(C).copy()
    pe[h] = (pe[h] + np.conj(pe[h, ::-1])) / 2
    pe[:h] = np.conj(pe[h + 1:][::-1, ::-1])
    g = ws.astype(L) * pe
    vl = v.astype(C)
    idx = n - 1 - np.arange(n)
    total = L(0)
    for a in range(h, n):
        w = L(1) if a == h else L(2)
        for b in range(n):
            y = np.sum(vl[a + idx][:, b + idx] * g)
            pa = p[a, b].astype(C)
            total += w * (np.conj(pa) * (ws[a, b].astype(L) * y + L(SIG) * pa)).real
    return total


def _vectors(mtot, kind):
    v, u = _problem(mtot, 200 + mtot)
    v, p = v.numpy(), u.numpy()
    h = (mtot - 1) // 2
    rng = np.random.default_rng(300 + mtot)
    ws = np.ones((mtot, mtot))
    if kind == "odd_row0":
        d = rng.standard_normal(mtot) + 1j * rng.standard_normal(mtot)
        p = p.copy()
        p[h] += 1e-3 * 0.5 * (d - np.conj(d[::-1]))                 # a conjugate-odd part in row 0
    if kind == "weights":
        w = np.exp(-2.5 * rng.random((mtot, mtot)))                  # entries down to e^-2.5, real and even: tests/test_gpu_cg_hermitian._system
        ws = 0.5 * (w + w[::-1, ::-1])
    return v, ws, p


@pytest.mark.parametrize("kind", ["even", "odd_row0", "weights"])
@pytest.mark.parametrize("mtot", [23, 21, 13, 5, 3, 1])
def test_frequency_form_matches_mode_form(mtot, kind):
    v, ws, p = _vectors(mtot, kind)
    Ap, G, Yh = _apply(_coefficients(v, mtot), ws, p)
    modes = _dot_modes(p, Ap)
    freq = _dot_freq(p, G, Yh)
    ref = _dot_longdouble(v, ws, p)
    e_modes, e_freq = abs(float(modes - ref)), abs(float(freq - ref))
    ulp = float(np.spacing(abs(float(ref))))
    print(f"\nmtot {mtot} {kind}: <p,Ap> = {float(ref):.6e}; modes off by {e_modes / ulp:.2f} ulp, frequencies by {e_freq / ulp:.2f} ulp; "
          f"the two differ by {abs(modes - freq) / abs(modes):.2e} relative")
    assert e_freq <= 10.0 * e_modes + ulp, (e_freq, e_modes, ulp)


def _pcg(v, ws, b, tol, dot):
    """The kernel's recurrence (cg.py:86-153) on the stored rows with the Jacobi diagonal; `dot(p, Ap, G, Yh)` forms <p, A p>."""
    n = b.shape[0]
    h = (n - 1) // 2
    cf = _coefficients(v, n)
    wgt = _wgt(n)
    dg = float(v[n - 1, n - 1].real) * ws[h:] ** 2 + SIG

    def full(rows):
        out = np.zeros((n, n), dtype=np.complex128)
        out[h:] = rows
        out[:h] = np.conj(rows[1:][::-1, ::-1])
        return out
    x = np.zeros((h + 1, n), dtype=np.complex128)
    r = b[h:].copy()
    z = r / dg
    p = z.copy()
    rz = float(np.sum(wgt * (np.conj(r) * z).real))
    den = np.sqrt(float(np.sum(wgt * np.abs(r) ** 2))) + 1e-16
    for it in range(1, 2 * n * n + 1):
        pf = full(p)
        Ap, G, Yh = _apply(cf, ws, pf)
        alpha = rz / (dot(pf, Ap, G, Yh) + 1e-16)
        x += alpha * p
        r -= alpha * Ap
        if np.sqrt(float(np.sum(wgt * np.abs(r) ** 2))) / den < tol:
            break
        z = r / dg
        rzn = float(np.sum(wgt * (np.conj(r) * z).real))
        p = z + (rzn / (rz + 1e-16)) * p
        rz = rzn
    return full(x), it


def test_whole_solve_takes_the_same_iterations_either_way():
    from test_gpu_cg_hermitian import _system
    v, T, ws, fy = _system(23, 17)
    v, ws = v.numpy(), ws.real.numpy().reshape(23, 23)
    b = ws * fy.numpy().reshape(23, 23)
    x_m, it_m = _pcg(v, ws, b, 1e-8, lambda p, Ap, G, Yh: _dot_modes(p, Ap))
    x_f, it_f = _pcg(v, ws, b, 1e-8, lambda p, Ap, G, Yh: _dot_freq(p, G, Yh))
    print(f"\niterations: modes {it_m}, frequencies {it_f}; solutions differ by {np.linalg.norm(x_m - x_f) / np.linalg.norm(x_m):.2e}")
    assert it_m == it_f
    assert np.linalg.norm(x_m - x_f) <= 100 * 1e-8 * np.linalg.norm(x_m)
    y = torch.from_numpy(ws.reshape(-1)) * T(torch.from_numpy((ws * x_f).reshape(-1))) + SIG * torch.from_numpy(x_f.reshape(-1))
    assert float(torch.linalg.norm(y - torch.from_numpy(b.reshape(-1))) / np.linalg.norm(b)) < 1e-7
