"""The dense restatement of the posterior gradient (tests/_jet_dense.py) checked on the CPU before the GPU tests lean on it: its
derivative rows against torch.autograd through its own dense mean, its value variance against the existing dense helper
(tests/_ard_dense.py), its probe estimator against its exact one; and the argument checks of `efgp_hip.mode_jet_rows` that need no
device."""
import math

import numpy as np
import pytest
import torch

import _ard_dense as D
import _jet_dense as JD

CASES = [((0.41,), (9,)), ((0.35, 0.27), (7, 5)), ((0.3, 0.22, 0.4), (3, 5, 3))]


def _case(hs, shape, N=60, NS=17):
    g = torch.Generator().manual_seed(len(shape))
    d = len(shape)
    x = torch.rand(N, d, generator=g, dtype=torch.float64)
    xn = torch.rand(NS, d, generator=g, dtype=torch.float64)
    y = torch.sin(4 * x[:, 0]) + 0.1 * torch.randn(N, generator=g, dtype=torch.float64)
    xi = JD.frequencies(hs, shape)
    ws = torch.exp(-0.5 * (xi ** 2).sum(dim=1)) * math.sqrt(math.prod(hs))           # real, even, positive
    return x, y, xn, ws, 0.07


@pytest.mark.parametrize("hs,shape", CASES)
def test_mean_gradient_is_autograd_of_the_dense_mean(hs, shape):
    x, y, xn, ws, sig = _case(hs, shape)
    beta = JD.fit(JD.features(x, hs, shape), y, ws, sig)
    Fn = JD.features(xn, hs, shape)
    grad = JD.mean_gradient(JD.feature_derivatives(Fn, hs, shape), ws, beta)
    xa = xn.clone().requires_grad_(True)
    JD.mean(JD.features(xa, hs, shape), ws, beta).sum().backward()            # point n enters its own mean only
    err = float((grad - xa.grad).abs().max() / xa.grad.abs().max())
    assert tuple(grad.shape) == tuple(xn.shape)
    assert err <= 1e-10, err
    # the per-axis phase tables give the same sums
    g = ws.to(torch.complex128) * beta
    xi = JD.frequencies(hs, shape)
    for a in range(len(shape)):
        tab = JD.exact_type2(xn, hs, shape, torch.complex(torch.zeros(len(xi), dtype=torch.float64), 2 * math.pi * xi[:, a]) * g)
        assert float((tab - grad[:, a]).abs().max() / grad[:, a].abs().max()) <= 1e-10


@pytest.mark.parametrize("hs,shape", CASES)
def test_value_variance_is_the_existing_dense_helpers(hs, shape):
    x, y, xn, ws, sig = _case(hs, shape)
    F, Fn = JD.features(x, hs, shape), JD.features(xn, hs, shape)
    assert np.abs(F.numpy() - D.features(x, hs, shape)).max() <= 1e-12
    C = JD.covariance(F, ws, sig)
    want = D.variance_regular(F.numpy(), Fn.numpy(), ws.numpy(), sig)
    got = JD.variance(Fn, C).numpy()
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    g = torch.Generator().manual_seed(9)
    eta = (torch.randint(0, 2, (5, len(ws)), generator=g) * 2 - 1).to(torch.float64)
    want = D.variance_lag_sums(F.numpy(), Fn.numpy(), ws.numpy(), sig, eta.numpy())
    got = JD.variance_probes(F, Fn, ws, sig, eta).numpy()
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


def test_probe_estimator_of_the_gradient_variance_is_exact_for_complete_probes():
    """With probes whose second moment is the identity (the columns of a Hadamard matrix), the estimator equals
    diag(Phi' C Phi'^H)."""
    hs, shape = (0.35, 0.27), (4, 2)
    x, y, xn, ws, sig = _case(hs, shape)
    H = torch.tensor([[1.0]])
    while H.shape[0] < 8:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    F, Fn = JD.features(x, hs, shape), JD.features(xn, hs, shape)
    dFn = JD.feature_derivatives(Fn, hs, shape)
    want = JD.gradient_variance(dFn, JD.covariance(F, ws, sig))
    got = JD.gradient_variance_probes(F, dFn, ws, sig, H.to(torch.float64))
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-10
    assert bool((want > 0).all())


def test_mode_jet_rows_refuses_bad_sizes_before_the_device():
    import efgp_hip
    from efgp_hip import mode_jet_rows
    from efgp_hip.lib import _SIGNATURES
    assert "efgp_mode_jet_rows" in efgp_hip.declared_symbols() and len(_SIGNATURES["efgp_mode_jet_rows"][1]) == 10
    f = torch.zeros((2, 30), dtype=torch.complex128)
    with pytest.raises(ValueError, match="mode_scale has 29 entries, the mode box .* has 30"):
        mode_jet_rows(f, (6, 5), 0.3, mode_scale=torch.ones(29, dtype=torch.complex128))
    with pytest.raises(ValueError, match="36 entries per row"):
        mode_jet_rows(f, (6, 6), 0.3)
    with pytest.raises(ValueError, match="1, 2 or 3"):
        mode_jet_rows(f, (1, 2, 3, 5), 0.3)
    with pytest.raises(ValueError, match="1, 2 or 3"):
        mode_jet_rows(f, (), 0.3)
