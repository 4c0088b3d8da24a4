"""EFGPND.predict_gradient / predict_gradient_grid, EFGPNDMulti's and the gradient of the draws, on the model cases of
tests/test_gpu_multi_output.py (a: SE 2-D 13 x 13, b: Matern-3/2 27 x 27, c: SE 1-D 31, d: SE 3-D 9^3, e: SE-ARD 15 x 13; N = 300..500,
nufft_eps = 1e-9, cg_tolerance = 1e-10, eps = 1e-3).  rel(a, b) = max|a - b| / max|b|.

Bounds.
* Transform only: every partial against the exact sums of the modes 2 pi i xi_a ws beta (tests/_nudft.type2; the per-axis tables of
  tests/_jet_dense.exact_type2 on the ARD grid), rel <= 2 nufft_eps + 1e-13; the mean of return_mean=True against predict's alike.
* Raster: against the exact sums at the meshgrid, 1e-11 sum |modes| -- the bar tests/test_gpu_predict_grid.py holds the mean map to;
  against predict_gradient at the meshgrid points, 4 nufft_eps max|grad_a| (DESIGN.md section 13's raster-against-points figure).
* Dense solve (tests/_jet_dense.py): the mean gradient, the regular variance of the partials and their stochastic variance with
  injected probes, each per axis at most 10 x the error of predict's own mean / regular variance / probe-injected stochastic variance
  against the same helper in the same run: the derivative weights the high modes, where the CG residual lives.
* Multi-output: column b against a fresh single-output model, 4 x the single models' own error against the dense helper.
* Draws: gradient=True returns the draws of gradient=False within 2 nufft_eps, and the gradient of draw 0 is the exact sum of its
  returned weights within the same bar.
"""
import functools
import math

import numpy as np
import pytest
import torch

import _ard_dense as D
import _jet_dense as JD
import _nudft as E
import _raster
import test_gpu_multi_output as MO

pytestmark = pytest.mark.gpu

NUFFT_EPS = MO.NUFFT_EPS
CASES = ["a", "b", "c", "d", "e"]
_rel, _np = MO._rel, MO._np


@functools.lru_cache(maxsize=None)
def _fitted(case):
    """(model on column 0, hs, shape, ws, beta as CPU tensors)."""
    _, Y, _ = MO._data(case)
    m = MO._single_model(case, Y[:, 0]).fit()
    st = m._fit_state
    MO._check_route(case, st)
    return m, tuple(float(h) for h in st["hs"]), tuple(int(n) for n in st["shape"]), st["ws"].detach().cpu(), st["beta"].detach().cpu()


def _derivative_modes(hs, shape, coef):
    """(d, M): 2 pi i xi_a coef."""
    xi = JD.frequencies(hs, shape)
    return torch.stack([torch.complex(torch.zeros(len(xi), dtype=torch.float64), 2 * math.pi * xi[:, a]) * coef for a in range(len(shape))])


def _exact(case, pts, hs, shape, modes):
    """Re of the exact sum of one row of modes at pts (CPU) -> (N,)."""
    if case == "e":                                          # one spacing per axis: the helper's per-axis tables
        return JD.exact_type2(pts, hs, shape, modes)
    return E.type2(pts, hs[0], modes, shape).real


# ---- 1. the transform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_partials_are_the_exact_sums_of_the_derivative_modes(case):
    m, hs, shape, ws, beta = _fitted(case)
    xn = MO._data(case)[2]
    d = len(shape)
    grad, var = m.predict_gradient(xn.cuda(), return_variance=False)
    assert tuple(grad.shape) == (50, d) == tuple(var.shape) and grad.dtype == torch.float64 and bool(torch.isnan(var).all())
    modes = _derivative_modes(hs, shape, ws * beta)
    errs = [_rel(_np(grad[:, a]), _exact(case, xn, hs, shape, modes[a]).numpy()) for a in range(d)]
    mean, grad2, _ = m.predict_gradient(xn.cuda(), return_variance=False, return_mean=True)
    ref_mean, _ = m.predict(xn.cuda(), return_variance=False)
    e_mean = _rel(_np(mean), _np(ref_mean))
    print(f"\ncase {case} grid {shape}: partials against the exact sums {errs}, mean against predict {e_mean:.2e} "
          f"(bound {2 * NUFFT_EPS + 1e-13:.2e})")
    assert torch.equal(grad2, grad)
    assert max(errs) <= 2 * NUFFT_EPS + 1e-13
    assert e_mean <= 2 * NUFFT_EPS + 1e-13


# ---- 2. rasters -----------------------------------------------------------------------------------------------------------------------
def _axes(case):
    g = torch.Generator().manual_seed(77)
    box = MO._SHAPES[case][1]
    lens = (6, 4, 3) if len(box) == 3 else (7, 5)
    return [torch.rand(n, generator=g, dtype=torch.float64) ** 2 * b for n, b in zip(lens, box)]          # unequally spaced, unsorted


@pytest.mark.parametrize("case", ["a", "d", "e"])
def test_gradient_maps_are_exact_and_agree_with_the_points(case):
    m, hs, shape, ws, beta = _fitted(case)
    axes = _axes(case)
    n_axis, d = tuple(len(a) for a in axes), len(shape)
    mean, grad, var = m.predict_gradient_grid(axes, return_variance=False, return_mean=True)
    assert tuple(grad.shape) == (d,) + n_axis == tuple(var.shape) and tuple(mean.shape) == n_axis and bool(torch.isnan(var).all())
    ref_mean, _ = m.predict_grid(axes, return_variance=False)
    assert torch.equal(mean, ref_mean) or _rel(_np(mean), _np(ref_mean)) <= 1e-13
    pts = _raster.meshgrid_points(axes)
    modes = _derivative_modes(hs, shape, ws * beta)
    pgrad, _ = m.predict_gradient(pts.cuda(), return_variance=False)
    for a in range(d):
        want = _exact(case, pts, hs, shape, modes[a]).reshape(n_axis)
        e_exact = float((grad[a].cpu() - want).abs().max()) / float(modes[a].abs().sum())
        diff = float((grad[a].reshape(-1) - pgrad[:, a]).abs().max())
        bound = 4 * NUFFT_EPS * float(pgrad[:, a].abs().max())
        print(f"\ncase {case} axis {a} raster {n_axis}: against the exact sums {e_exact:.2e} of sum |modes| (bound 1e-11); against "
              f"predict_gradient {diff:.2e} (bound {bound:.2e})")
        assert e_exact <= 1e-11
        assert diff <= bound


def test_variance_maps_are_the_point_variances():
    m, hs, shape, _, _ = _fitted("a")
    axes = _axes("a")
    pts = _raster.meshgrid_points(axes).cuda()
    probes = _probes(math.prod(shape), 6)
    _, gv = m.predict_gradient_grid(axes, variance_probes=probes)
    _, pv = m.predict_gradient(pts, variance_probes=probes)
    assert tuple(gv.shape) == (2, 7, 5)
    for a in range(2):
        assert float((gv[a].reshape(-1) - pv[:, a]).abs().max()) <= 4 * NUFFT_EPS * float(pv[:, a].abs().max())
    _, gr = m.predict_gradient_grid(axes, variance_method="regular")
    _, pr = m.predict_gradient(pts, variance_method="regular")
    assert torch.equal(gr.reshape(2, -1).T, pr)                  # the same 8192-cell blocks, the same solves


# ---- 3. against a dense solve -------------------------------------------------------------------------------------------------------
def _probes(M, J, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (J, M), generator=g) * 2 - 1).to(torch.float64)


@functools.lru_cache(maxsize=None)
def _dense(case):
    """The helper's quantities at the case's 50 new points, column 0, on the model's grid: dict of CPU tensors."""
    _, hs, shape, _, _ = _fitted(case)
    x, Y, xn = MO._data(case)
    sig = MO._SIG[case]
    ws = torch.as_tensor(D.weights(MO._kernel(case), hs, shape)[0])
    F, Fn = JD.features(x, hs, shape), JD.features(xn, hs, shape)
    dFn = JD.feature_derivatives(Fn, hs, shape)
    beta = JD.fit(F, Y[:, 0], ws, sig)
    C = JD.covariance(F, ws, sig)
    eta = _probes(len(ws), 6)
    return dict(mean=JD.mean(Fn, ws, beta), grad=JD.mean_gradient(dFn, ws, beta), var=JD.variance(Fn, C),
                grad_var=JD.gradient_variance(dFn, C), var_probes=JD.variance_probes(F, Fn, ws, sig, eta),
                grad_var_probes=JD.gradient_variance_probes(F, dFn, ws, sig, eta), eta=eta, F=F, dFn=dFn, ws=ws)


@pytest.mark.parametrize("case", CASES)
def test_gradient_and_its_variances_against_the_dense_solve(case):
    m, hs, shape, _, _ = _fitted(case)
    xn = MO._data(case)[2].cuda()
    dn = _dense(case)
    d = len(shape)
    mean, var_reg = m.predict(xn, variance_method="regular")
    _, var_st = m.predict(xn, variance_probes=dn["eta"])
    y_mean, y_reg, y_st = _rel(_np(mean), dn["mean"].numpy()), _rel(_np(var_reg), dn["var"].numpy()), _rel(_np(var_st), dn["var_probes"].numpy())
    grad, gv_reg = m.predict_gradient(xn, variance_method="regular")
    _, gv_st = m.predict_gradient(xn, variance_probes=dn["eta"])
    assert tuple(gv_reg.shape) == (50, d) == tuple(gv_st.shape)
    e_grad = [_rel(_np(grad[:, a]), dn["grad"][:, a].numpy()) for a in range(d)]
    e_reg = [_rel(_np(gv_reg[:, a]), dn["grad_var"][:, a].numpy()) for a in range(d)]
    e_st = [_rel(_np(gv_st[:, a]), dn["grad_var_probes"][:, a].numpy()) for a in range(d)]
    print(f"\ncase {case} grid {shape} against the dense solve (gradient per axis | predict's own):\n"
          f"  mean                {e_grad} | {y_mean:.2e}\n  regular variance    {e_reg} | {y_reg:.2e}\n"
          f"  stochastic variance {e_st} | {y_st:.2e}")
    assert bool((dn["grad_var"] > 0).all())
    assert max(e_grad) <= 10 * y_mean, f"mean gradient {e_grad}, predict's mean {y_mean:.2e}: ratio {max(e_grad) / y_mean:.1f}"
    assert max(e_reg) <= 10 * y_reg, f"regular variance {e_reg}, predict's {y_reg:.2e}: ratio {max(e_reg) / y_reg:.1f}"
    assert max(e_st) <= 10 * y_st, f"stochastic variance {e_st}, predict's {y_st:.2e}: ratio {max(e_st) / y_st:.1f}"


# ---- 4. many outputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single_gradients():
    """Case a, columns 0..2: the gradient of a fresh single-output model per column and its error against the dense helper."""
    x, Y, xn = MO._data("a")
    dn = _dense("a")
    grads, errs = [], []
    for b in range(3):
        g, _ = MO._single_model("a", Y[:, b]).predict_gradient(xn.cuda(), return_variance=False)
        beta = JD.fit(dn["F"], Y[:, b], dn["ws"], MO._SIG["a"])
        grads.append(g.cpu())
        errs.append(_rel(_np(g), JD.mean_gradient(dn["dFn"], dn["ws"], beta).numpy()))
    return torch.stack(grads, dim=1), max(errs)


@pytest.mark.parametrize("scales", [(1.0, 1.0, 1.0), (1.0, 1e-6, 1e6)], ids=["plain", "scaled"])
def test_multi_output_columns_are_the_single_output_gradients(scales):
    x, Y, xn = MO._data("a")
    singles, e_single = _single_gradients()
    sc = torch.tensor(scales, dtype=torch.float64)
    multi = MO._multi_model("a", Y[:, :3] * sc[None, :])
    mean, grad, var = multi.predict_gradient(xn.cuda(), variance_probes=_probes(math.prod(_fitted("a")[2]), 6), return_mean=True)
    assert tuple(mean.shape) == (50, 3) and tuple(grad.shape) == (50, 3, 2) and tuple(var.shape) == (50, 2)
    ref_mean, _ = multi.predict(xn.cuda(), return_variance=False)
    assert _rel(_np(mean), _np(ref_mean)) <= 2 * NUFFT_EPS + 1e-13
    errs = [_rel(_np(grad[:, b]), singles[:, b].numpy() * scales[b]) for b in range(3)]
    print(f"\ncolumns x {scales}: against single-output models {errs}; their own error against the dense solve {e_single:.2e}")
    assert max(errs) <= 4 * e_single
    _, v1 = MO._single_model("a", Y[:, 0]).predict_gradient(xn.cuda(), variance_probes=_probes(math.prod(_fitted("a")[2]), 6))
    assert _rel(_np(var), _np(v1)) <= 4 * e_single              # shared by the outputs: the single model's, from the same probes
    axes = _axes("a")
    gmean, ggrad, gvar = multi.predict_gradient_grid(axes, return_variance=False, return_mean=True)
    assert tuple(gmean.shape) == (3, 7, 5) and tuple(ggrad.shape) == (3, 2, 7, 5) and tuple(gvar.shape) == (2, 7, 5)
    pgrad, _ = multi.predict_gradient(_raster.meshgrid_points(axes).cuda(), return_variance=False)
    for b in range(3):
        for a in range(2):
            assert float((ggrad[b, a].reshape(-1) - pgrad[:, b, a]).abs().max()) <= 4 * NUFFT_EPS * float(pgrad[:, b, a].abs().max())


# ---- 5. draws -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", [False, True], ids=["posterior", "prior"])
def test_draws_come_with_their_exact_gradients(prior):
    m, hs, shape, ws, _ = _fitted("a")
    xn = MO._data("a")[2]
    seed, tol = 20250317, 1e-6
    draws, grads, state = m.sample_paths(xn.cuda(), 3, seed=seed, prior=prior, cg_tolerance=tol, gradient=True, return_state=True)
    ref = m.sample_paths(xn.cuda(), 3, seed=seed, prior=prior, cg_tolerance=tol)
    assert tuple(draws.shape) == (3, 50) and tuple(grads.shape) == (3, 50, 2)
    e_draw = _rel(_np(draws), _np(ref))
    modes = _derivative_modes(hs, shape, ws * state["weights"][0].cpu())
    errs = [_rel(_np(grads[0, :, a]), E.type2(xn, hs[0], modes[a], shape).real.numpy()) for a in range(2)]
    print(f"\nprior={prior}: draws against gradient=False {e_draw:.2e}; gradient of draw 0 against the exact sums of its weights {errs}")
    assert e_draw <= 2 * NUFFT_EPS
    assert max(errs) <= 2 * NUFFT_EPS
    axes = _axes("a")
    gd, gg = m.sample_paths_grid(axes, 3, seed=seed, prior=prior, cg_tolerance=tol, gradient=True)
    gref = m.sample_paths_grid(axes, 3, seed=seed, prior=prior, cg_tolerance=tol)
    assert tuple(gd.shape) == (3, 7, 5) and tuple(gg.shape) == (3, 2, 7, 5)
    assert _rel(_np(gd), _np(gref)) <= 2 * NUFFT_EPS
    pts = _raster.meshgrid_points(axes)
    for a in range(2):
        want = E.type2(pts, hs[0], modes[a], shape).real.reshape(7, 5)
        assert float((gg[0, a].cpu() - want).abs().max()) <= 1e-11 * float(modes[a].abs().sum())


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    m, _, _, _, _ = _fitted("a")
    x, Y, xn = MO._data("a")
    with pytest.raises(ValueError, match="columns"):
        m.predict_gradient(xn[:, :1].cuda())
    with pytest.raises(ValueError, match="Variance method"):
        m.predict_gradient(xn.cuda(), variance_method="exact")
    with pytest.raises(ValueError, match="Variance method"):
        m.predict_gradient_grid(_axes("a"), variance_method="exact")
    with pytest.raises(ValueError, match="axes"):
        m.predict_gradient_grid(_axes("a")[:1])
    from efgpnd import EFGPND
    sharded = EFGPND(x.cuda(), Y[:, 0].cuda(), MO._kernel("a"), sigmasq=0.1, eps=MO.EPS, nufft_eps=NUFFT_EPS, estimate_params=False,
                     opts={"shard_points": True})
    with pytest.raises(NotImplementedError, match="shard_points"):
        sharded.predict_gradient(xn.cuda())
    with pytest.raises(NotImplementedError, match="shard_points"):
        sharded.predict_gradient_grid(_axes("a"))
    from efgp_hip import mode_jet_rows
    with pytest.raises(ValueError, match="mode_scale has 5 entries"):
        mode_jet_rows(m._fit_state["beta"], m._fit_state["shape"], 0.5, mode_scale=torch.ones(5, dtype=torch.complex128, device="cuda"))
