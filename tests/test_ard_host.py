"""Host checks of the ARD kernels (kernels/ard.py), the per-axis grid (utils.kernels.get_xis_nd) and the host twin of the weight
launch (efgp_spectral_weights_host_nd).  No GPU."""
import math

import numpy as np
import pytest
import torch

import _ard_dense as D
from kernels import Matern, MaternARD, SquaredExponential, SquaredExponentialARD
from utils.kernels import get_xis, get_xis_nd

# (ARD kernel with equal lengthscales, the isotropic kernel it must reduce to)
_PAIRS = [
    (lambda: SquaredExponentialARD(dimension=2, init_lengthscale=0.3, init_variance=1.7),
     lambda: SquaredExponential(dimension=2, init_lengthscale=0.3, init_variance=1.7)),
    (lambda: SquaredExponentialARD(dimension=3, init_lengthscale=0.45, init_variance=0.6),
     lambda: SquaredExponential(dimension=3, init_lengthscale=0.45, init_variance=0.6)),
    (lambda: SquaredExponentialARD(dimension=1, init_lengthscale=0.1, init_variance=1.0),
     lambda: SquaredExponential(dimension=1, init_lengthscale=0.1, init_variance=1.0)),
    (lambda: MaternARD(dimension=2, nu=0.5, init_lengthscale=0.3, init_variance=1.2),
     lambda: Matern(dimension=2, nu=0.5, init_lengthscale=0.3, init_variance=1.2)),
    (lambda: MaternARD(dimension=2, nu=1.5, init_lengthscale=0.25, init_variance=0.9),
     lambda: Matern(dimension=2, nu=1.5, init_lengthscale=0.25, init_variance=0.9)),
    (lambda: MaternARD(dimension=3, nu=2.5, init_lengthscale=0.5, init_variance=2.0),
     lambda: Matern(dimension=3, nu=2.5, init_lengthscale=0.5, init_variance=2.0)),
]
# anisotropic kernels for the derivative, grid and weight checks
_ANISO = [
    lambda: SquaredExponentialARD(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.3),
    lambda: SquaredExponentialARD(dimension=3, init_lengthscale=(0.1, 0.5, 0.3), init_variance=0.8),
    lambda: MaternARD(dimension=2, nu=1.5, init_lengthscale=(0.15, 0.6), init_variance=1.0),
    lambda: MaternARD(dimension=3, nu=2.5, init_lengthscale=(0.3, 0.2, 0.7), init_variance=1.5),
    lambda: MaternARD(dimension=1, nu=0.5, init_lengthscale=(0.2,), init_variance=0.7),
]


def _omega(d, seed=0, n=200, scale=6.0):
    g = torch.Generator().manual_seed(seed)
    om = (torch.rand(n, d, generator=g, dtype=torch.float64) * 2 - 1) * scale
    om[0] = 0.0
    return om


def test_hypers_and_validation():
    k = SquaredExponentialARD(dimension=3, init_lengthscale=(0.1, 0.2, 0.3), init_variance=2.0)
    assert k.hypers == ["lengthscale_0", "lengthscale_1", "lengthscale_2", "variance"] and k.num_hypers == 5
    assert k._gp_params_ref.hypers_names == k.hypers and k._gp_params_ref.raw.numel() == 5
    assert np.allclose(k.lengthscales, (0.1, 0.2, 0.3), rtol=1e-6) and abs(k.variance - 2.0) < 1e-6
    assert np.allclose(SquaredExponentialARD(dimension=2, init_lengthscale=0.4).lengthscales, (0.4, 0.4), rtol=1e-6)
    k.set_hyper("lengthscale_1", 0.7)
    assert abs(k.lengthscales[1] - 0.7) < 1e-6
    k.set_hyper("lengthscale", (0.3, 0.4, 0.5))
    assert np.allclose(k.lengthscales, (0.3, 0.4, 0.5), rtol=1e-6)
    with pytest.raises(ValueError):
        SquaredExponentialARD(dimension=2, init_lengthscale=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError):
        SquaredExponentialARD(dimension=2, init_lengthscale=(0.1, 0.0))
    with pytest.raises(ValueError):
        SquaredExponentialARD(dimension=0)
    for nu in (1.0, 3.5, 0.1):
        with pytest.raises(ValueError):
            MaternARD(dimension=2, nu=nu)
    with pytest.raises(ValueError, match="dimension 1"):
        k.kernel(torch.tensor([0.1]))
    k1 = MaternARD(dimension=1, nu=1.5, init_lengthscale=0.2, init_variance=1.1)
    r = torch.linspace(0, 1, 7, dtype=torch.float64)
    iso = Matern(dimension=1, nu=1.5, init_lengthscale=0.2, init_variance=1.1)
    assert float((k1.kernel(r) - iso.kernel(r)).abs().max()) < 1e-12


@pytest.mark.parametrize("make", _ANISO)
def test_kernel_matrix_matches_a_double_loop(make):
    k = make()
    d = k.dimension
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(7, d, generator=g, dtype=torch.float64), torch.rand(5, d, generator=g, dtype=torch.float64)
    ell, var, nu = k.lengthscales, k.variance, k.nu
    K = k.kernel_matrix(x, y)
    for i in range(7):
        for j in range(5):
            r = math.sqrt(sum(((float(x[i, a]) - float(y[j, a])) / ell[a]) ** 2 for a in range(d)))
            if isinstance(k, SquaredExponentialARD):
                ref = var * math.exp(-0.5 * r * r)
            elif nu == 0.5:
                ref = var * math.exp(-r)
            elif nu == 1.5:
                ref = var * (1 + math.sqrt(3) * r) * math.exp(-math.sqrt(3) * r)
            else:
                ref = var * (1 + math.sqrt(5) * r + 5 * r * r / 3) * math.exp(-math.sqrt(5) * r)
            assert abs(float(K[i, j]) - ref) < 1e-13 * var
    if d > 1:
        with pytest.raises(ValueError):
            k.kernel_matrix(x[:, :1], y)


@pytest.mark.parametrize("pair", _PAIRS)
def test_equal_lengthscales_reduce_to_the_isotropic_class(pair):
    ard, iso = pair[0](), pair[1]()
    d = ard.dimension
    om = _omega(d, scale=3.0 / ard.lengthscales[0] / (2 * math.pi))
    S, Si = ard.spectral_density(om), iso.spectral_density(om)
    assert S.shape == (om.shape[0],)
    assert float((S - Si).abs().max()) < 1e-12 * float(Si.abs().max())
    G, Gi = ard.spectral_grad(om), iso.spectral_grad(om)
    assert G.shape == (om.shape[0], d + 1)
    big = float(Gi.abs().max())
    assert float((G[:, :d].sum(1) - Gi[:, 0]).abs().max()) < 1e-12 * big          # sum_j dS/dl_j = isotropic dS/dl
    assert float((G[:, d] - Gi[:, 1]).abs().max()) < 1e-12 * big
    x = torch.rand(6, d, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert float((ard.kernel_matrix(x, x) - iso.kernel_matrix(x, x)).abs().max()) < 1e-12


@pytest.mark.parametrize("make", _ANISO)
def test_spectral_grad_agrees_with_central_differences(make):
    """Step 1e-6 l: the quotient's own error is ~ (1e-6)^2 of third derivatives plus 1e-16 / 1e-6 of rounding, about 1e-10."""
    k = make()
    d = k.dimension
    om = _omega(d, seed=2, scale=2.0 / min(k.lengthscales) / (2 * math.pi))
    base = dict(zip(k.hypers, k.get_hypers()))
    k._params_dict.update(base)
    k._gp_params_ref = None                              # from here on the kernel reads these exact floats
    G = k.spectral_grad(om)
    big = G.abs().max(0).values
    for i, name in enumerate(k.hypers):
        step = 1e-6 * base[name]
        vals = []
        for s in (+1, -1):
            k._params_dict[name] = base[name] + s * step
            vals.append(k.spectral_density(om))
        k._params_dict[name] = base[name]
        fd = (vals[0] - vals[1]) / (2 * step)
        assert float((fd - G[:, i]).abs().max()) < 1e-6 * float(big[i]), name


@pytest.mark.parametrize("make", _ANISO)
def test_get_xis_nd_is_per_axis_get_xis(make):
    k = make()
    d = k.dimension
    Ls = [1.0, 0.3, 0.45][:d]
    for eps, trunc in ((1e-3, None), (1e-6, None), (1e-4, 1e-2)):
        hs, shape = get_xis_nd(k, eps, Ls, trunc_eps=trunc)
        assert len(hs) == d and len(shape) == d
        for j in range(d):
            ell, var = k.lengthscales[j], k.variance
            if isinstance(k, SquaredExponentialARD):
                iso = SquaredExponential(dimension=d, init_lengthscale=ell, init_variance=var)
            else:
                iso = Matern(dimension=d, nu=k.nu, init_lengthscale=ell, init_variance=var)
            iso._gp_params_ref = None
            _, h, n = get_xis(iso, eps, Ls[j], use_integral=True, trunc_eps=trunc)
            assert hs[j] == h and shape[j] == n and n % 2 == 1
    with pytest.raises(ValueError):
        get_xis_nd(k, 1e-3, Ls + [1.0])


@pytest.mark.parametrize("pair", _PAIRS)
def test_equal_lengthscales_on_a_square_box_give_the_isotropic_grid(pair):
    ard, iso = pair[0](), pair[1]()
    for eps, L in ((1e-2, 1.0), (1e-4, 1.0), (1e-6, 2.3)):
        _, h, mtot = get_xis(iso, eps, L, use_integral=True)
        hs, shape = get_xis_nd(ard, eps, [L] * ard.dimension)
        assert hs == (h,) * ard.dimension and shape == (mtot,) * ard.dimension           # bit for bit


def test_issue_blocks():
    """The blocks of the quadrature check: SE (0.08, 0.5) on [0,1] x [0,0.3] at 1e-4, Matern-3/2 (0.15, 0.6) on [0,1] x [0,0.4]."""
    k = SquaredExponentialARD(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.0)
    assert get_xis_nd(k, 1e-4, [1.0, 0.3])[1] == (27, 9)
    m = MaternARD(dimension=2, nu=1.5, init_lengthscale=(0.15, 0.6), init_variance=1.0)
    assert get_xis_nd(m, 1e-3, [1.0, 0.4])[1] == (45, 17)
    # the per-axis grid reproduces the ARD kernel to the tolerance, as the isotropic grid does for the isotropic kernel
    g = torch.Generator().manual_seed(0)
    x = torch.rand(120, 2, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.3], dtype=torch.float64)
    hs, shape = get_xis_nd(k, 1e-4, [1.0, 0.3])
    assert D.kernel_error(k, x, hs, shape) < 2e-4


@pytest.mark.parametrize("make", _ANISO)
def test_host_weights_match_the_kernel_classes(make):
    from efgp_hip import spectral_weights_host_nd
    k = make()
    d = k.dimension
    hs, shape = get_xis_nd(k, 1e-3, [1.0, 0.3, 0.45][:d])
    ws, dp = spectral_weights_host_nd(k.ard_kind, k.nu, k.lengthscales, k.variance, hs, shape, want_grad=True)
    ws_ref, dp_ref = D.weights(k, hs, shape)
    assert ws.shape == (math.prod(shape),) and dp.shape == (math.prod(shape), d + 1)
    assert float(ws.imag.abs().max()) == 0.0 and float(dp.imag.abs().max()) == 0.0
    assert np.abs(ws.real.numpy() - ws_ref).max() < 1e-12 * np.abs(ws_ref).max()
    assert np.abs(dp.real.numpy() - dp_ref).max() < 1e-12 * np.abs(dp_ref).max()
    ws2, none = spectral_weights_host_nd(k.ard_kind, k.nu, k.lengthscales, k.variance, hs, shape)
    assert none is None and torch.equal(ws2, ws)


def test_host_weights_argument_checks():
    from efgp_hip import spectral_weights_host_nd
    with pytest.raises(ValueError):
        spectral_weights_host_nd(0, 0.0, (0.1, 0.2), 1.0, (0.5, 0.5), (9, 8))           # even mode count
    with pytest.raises(ValueError):
        spectral_weights_host_nd(1, 2.0, (0.1, 0.2), 1.0, (0.5, 0.5), (9, 9))           # nu not built in
    with pytest.raises(ValueError):
        spectral_weights_host_nd(0, 0.0, (0.1, -0.2), 1.0, (0.5, 0.5), (9, 9))
    with pytest.raises(ValueError):
        spectral_weights_host_nd(0, 0.0, (0.1, 0.2), 1.0, (0.5,), (9, 9))


def test_estimate_hyperparameters_is_per_axis():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(300, 2, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.1], dtype=torch.float64)
    y = torch.sin(4 * x[:, 0])
    ells, var, noise = SquaredExponentialARD(dimension=2).estimate_hyperparameters(x, y)
    dj = [(x[:, j, None] - x[None, :, j]).abs() for j in range(2)]
    assert np.allclose(ells, [0.5 * float(torch.median(d_[d_ > 0])) for d_ in dj])
    assert abs(var - float(torch.var(y))) < 1e-12 and abs(noise - 0.2 * var) < 1e-12
    ells_m, _, _ = MaternARD(dimension=2, nu=1.5).estimate_hyperparameters(x, y)
    assert np.allclose(ells_m, [float(torch.median(d_[d_ > 0])) for d_ in dj])


def test_log_marginal_is_the_dense_one():
    k = SquaredExponentialARD(dimension=2, init_lengthscale=(0.2, 0.6), init_variance=1.1)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(40, 2, generator=g, dtype=torch.float64)
    y = torch.sin(3 * x[:, 0]) + 0.1 * torch.randn(40, generator=g, dtype=torch.float64)
    ref = D.exact_gp(k, x, y, 0.05, x[:2])[2]
    assert abs(k.log_marginal(x, y, 0.05) - ref) < 1e-6 * abs(ref)      # the class adds sigma^2 I in torch's default dtype
