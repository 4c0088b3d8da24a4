"""Host checks of the path sampler's mathematics (tests/_sampling.py, the dense restatement the GPU tests compare against) and of
the argument refusals of EFGPND.sample_paths that need no device."""
import math

import pytest
import torch

import _sampling as S


def _case_1d(N=60, mtot=21, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 1, generator=g, dtype=torch.float64) * 2 - 1
    y = torch.sin(3 * x[:, 0]) + 0.3 * torch.randn(N, generator=g, dtype=torch.float64)
    h = 0.35
    k = S.mode_grid(mtot, 1)[:, 0]
    ws = torch.exp(-0.5 * (0.4 * 2 * math.pi * h * k) ** 2).to(torch.complex128) * math.sqrt(h)      # real, even, decaying
    xn = torch.linspace(-1, 1, 9, dtype=torch.float64).reshape(-1, 1)
    return x, y, h, mtot, ws, xn


def test_conjugate_index_map():
    """j -> M - 1 - j is the negated frequency on the row-major symmetric box, in 1, 2 and 3 dimensions."""
    for d, mtot in ((1, 7), (2, 5), (3, 3)):
        k = S.mode_grid(mtot, d)
        M = k.shape[0]
        assert M == mtot ** d
        idx = S.conj_index(M)
        assert torch.equal(k[idx], -k)
        assert int(idx[(M - 1) // 2]) == (M - 1) // 2 and torch.equal(k[(M - 1) // 2], torch.zeros(d, dtype=torch.float64))
        assert torch.equal(idx[idx], torch.arange(M))


def test_hermitian_rows_are_conjugate_even_with_unit_covariance():
    g = torch.Generator().manual_seed(3)
    n, M = 40000, 9
    e = S.conj_even_normal(n, M, g)
    assert torch.equal(e.flip(1).conj(), e)
    assert torch.equal(e[:, (M - 1) // 2].imag, torch.zeros(n, dtype=torch.float64))
    C = (e.T @ e.conj()) / n                                     # E e e^H = I: entries have standard error <= 1 / sqrt(n)
    assert float((C - torch.eye(M, dtype=C.dtype)).abs().max()) < 5 * math.sqrt(2.0 / n)
    # a ws fz + b e with a conjugate-even fz: the same formula entry by entry
    fz = S.conj_even_normal(4, M, g)
    ws = torch.linspace(1, 2, M, dtype=torch.float64)
    ws = (ws + ws.flip(0)).to(torch.complex128)
    fill = torch.randn(8, M, dtype=torch.float64, generator=g)
    r = S.hermitian_rows(fill, a=0.7, ws=ws, fz=fz, b=0.3)
    assert torch.allclose(r, 0.7 * ws * fz + 0.3 * S.hermitian_rows(fill), rtol=0, atol=1e-14)
    assert torch.equal(r.flip(1).conj(), r)


def test_weight_space_covariance_is_the_exact_posterior_covariance():
    """sigma^2 Phi D A^-1 D Phi^H equals K_nn - K_no (K_oo + sigma^2 I)^-1 K_on for K = F D^2 F^H: 1e-10 of the largest entry."""
    x, y, h, mtot, ws, xn = _case_1d()
    F, Fn = S.feature_matrix(x, h, mtot), S.feature_matrix(xn, h, mtot)
    for sigmasq in (0.1, 0.7):
        cw = S.weight_space_cov(F, Fn, ws, sigmasq)
        cf = S.function_space_cov(F, Fn, ws, sigmasq)
        assert float((cw - cf).abs().max()) < 1e-10 * float(cf.abs().max())
    # the mean of the weights reproduces the kernel-space posterior mean as well
    sigmasq = 0.1
    beta = S.posterior_weights(F, y, ws, sigmasq)
    D2 = (ws * ws.conj()).real.to(F.dtype)
    K_oo = ((F * D2) @ F.conj().T).real
    K_no = ((Fn * D2) @ F.conj().T).real
    mean = K_no @ torch.linalg.solve(K_oo + sigmasq * torch.eye(x.shape[0], dtype=torch.float64), y)
    got = S.paths_from_weights(Fn, ws, beta.reshape(1, -1))[0]
    assert float((got - mean).abs().max()) < 1e-10 * float(mean.abs().max())


def test_dense_sampler_has_the_posterior_law():
    """20000 draws of the restated sampler: mean, variances and one covariance within five standard errors."""
    x, y, h, mtot, ws, xn = _case_1d()
    F, Fn = S.feature_matrix(x, h, mtot), S.feature_matrix(xn, h, mtot)
    sigmasq, n = 0.2, 20000
    g = torch.Generator().manual_seed(11)
    e1 = torch.randn(n, x.shape[0], dtype=torch.float64, generator=g)
    e2 = S.conj_even_normal(n, F.shape[1], g)
    beta = S.posterior_weights(F, y, ws, sigmasq)
    paths, w = S.dense_paths(F, Fn, ws, sigmasq, beta, e1, e2)
    assert float((w.flip(1).conj() - w).abs().max()) < 1e-12
    cov = S.function_space_cov(F, Fn, ws, sigmasq)
    v = cov.diagonal()
    mean = S.paths_from_weights(Fn, ws, beta.reshape(1, -1))[0]
    assert bool(((paths.mean(0) - mean).abs() <= 5 * (v / n).sqrt()).all())
    assert bool(((paths.var(0, unbiased=True) / v - 1).abs() <= 5 * math.sqrt(2.0 / (n - 1))).all())
    d = paths - paths.mean(0)
    c01 = float((d[:, 3] * d[:, 4]).sum() / (n - 1))
    assert abs(c01 - float(cov[3, 4])) <= 5 * math.sqrt(float(cov[3, 4] ** 2 + v[3] * v[4]) / n)


def _cpu_model(**opts):
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential
    g = torch.Generator().manual_seed(0)
    x = torch.rand(50, 2, generator=g, dtype=torch.float64)
    y = torch.randn(50, generator=g, dtype=torch.float64)
    k = SquaredExponential(dimension=2, init_lengthscale=0.3, init_variance=1.0)
    return EFGPND(x, y, k, sigmasq=0.1, eps=1e-3, estimate_params=False, opts=opts), x


def test_refusals_that_need_no_device():
    m, x = _cpu_model()
    with pytest.raises(ValueError, match="nsamples"):
        m.sample_paths(x, 0)
    with pytest.raises(ValueError, match="nsamples"):
        m.sample_paths(x, -3, prior=True)
    with pytest.raises(ValueError, match="columns"):
        m.sample_paths(torch.zeros(4, 3, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="columns"):
        m.sample_paths(torch.zeros(4, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="method"):
        m.sample_posterior(x, 2, method="sparse")
    ms, _ = _cpu_model(shard_points=True)
    with pytest.raises(NotImplementedError, match="shard_points"):
        ms.sample_paths(x, 2)


def test_row_offsets_wrap_like_the_generator():
    """normal_row_offset: pair p at index n is pair 0 at index n + p * stride in wrapping 64-bit arithmetic, as a signed value."""
    from efgp_hip import normal_row_offset
    from efgp_hip.ops import NORMAL_ROW_STRIDE
    assert normal_row_offset(0) == 0 and normal_row_offset(0, 7) == 7
    for first, off in ((2, 0), (64, 5), (4096, 123456789)):
        v = normal_row_offset(first, off)
        assert -2 ** 63 <= v < 2 ** 63
        assert v % 2 ** 64 == (off + (first // 2) * NORMAL_ROW_STRIDE) % 2 ** 64
    with pytest.raises(ValueError):
        normal_row_offset(3)
