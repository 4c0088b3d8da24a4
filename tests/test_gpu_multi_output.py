"""EFGPNDMulti (efgpnd_multi.py) on the GPU against the dense restatement (tests/_multi_dense.py) and against B single-output EFGPND
models, which are the existing path and the yardstick.

Cases, the smallest at which each route can go wrong (every one asserts the route it is meant to take):
  a  N = 400, d = 2, squared exponential, block <= 23 x 23 (the 48 x 48 solve route)       B = 1, 2, 3, 5
  b  N = 400, d = 2, Matern-3/2, mtot in 25..31 (the 64 x 64 route)                        B = 3
  c  N = 500, d = 1, squared exponential                                                    B = 4
  d  N = 300, d = 3, squared exponential, mtot <= 9                                         B = 3
  e  N = 400, d = 2, SquaredExponentialARD on a 2 : 1 box (per-axis grid)                   B = 2
B = 3 and B = 5 leave an unpaired real row in the type-1 transform.  nufft_eps = 1e-9 and cg_tolerance = 1e-10 throughout, so that
solver stopping rules do not decide a comparison.  rel(a, b) = max|a - b| / max|b|.

Bounds.  Fit: e_multi_b <= 4 max_b' e_single_b' -- the 2 x transform-tolerance contract once for the row transform and once for the
yardstick's pair transform; both error columns are printed.  Means and variances of a multi-output model against a single-output one
are linear maps of the coefficients (and, for the variance, of the same Toeplitz vector through the same probes), so they are held
to the same figure.  Gradient: 10 x the change of the yardstick's own sum when its tolerances go from (nufft_eps, cg_tol) to
(nufft_eps / 10, cg_tol / 100), in the maximum norm over the entries -- only stopping rules, the transform route and the
summation order differ.
"""
import functools
import math

import numpy as np
import pytest
import torch

import _ard_dense as D
import _multi_dense as MD

pytestmark = pytest.mark.gpu

NUFFT_EPS, CG_TOL, EPS = 1e-9, 1e-10, 1e-3
OPTS = {"cg_tolerance": CG_TOL, "mean_cg_warm_start": False}


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _np(t):
    return t.detach().cpu().numpy()


def _kernel(case):
    import kernels
    return {"a": lambda: kernels.SquaredExponential(dimension=2, init_lengthscale=0.2, init_variance=1.3),
            "b": lambda: kernels.Matern(dimension=2, nu=1.5, init_lengthscale=0.3, init_variance=1.0),
            "c": lambda: kernels.SquaredExponential(dimension=1, init_lengthscale=0.05, init_variance=1.3),
            "d": lambda: kernels.SquaredExponential(dimension=3, init_lengthscale=0.4, init_variance=1.0),
            "e": lambda: kernels.SquaredExponentialARD(dimension=2, init_lengthscale=(0.3, 0.2), init_variance=1.3)}[case]()


_SHAPES = {"a": (400, (1.0, 1.0)), "b": (400, (1.0, 1.0)), "c": (500, (1.0,)), "d": (300, (1.0, 1.0, 1.0)), "e": (400, (2.0, 1.0))}
_SIG = {"a": 0.1, "b": 0.2, "c": 0.1, "d": 0.15, "e": 0.1}
_BMAX = {"a": 5, "b": 3, "c": 4, "d": 3, "e": 2}


def _check_route(case, st):
    """The grid a case is meant to land on."""
    shape = tuple(st["shape"])
    if case == "a":
        assert len(shape) == 2 and max(shape) <= 23, shape
    elif case == "b":
        assert len(shape) == 2 and 25 <= shape[0] <= 31, shape
    elif case == "c":
        assert len(shape) == 1, shape
    elif case == "d":
        assert len(shape) == 3 and max(shape) <= 9, shape
    else:
        assert st["ard"] and shape[0] != shape[1], shape


@functools.lru_cache(maxsize=None)
def _data(case):
    """x in the case's box (two points at opposite corners: the box sides are exact), B_max smooth columns plus noise, 50 new points."""
    N, box = _SHAPES[case]
    g = torch.Generator().manual_seed(ord(case))
    b = torch.tensor(box, dtype=torch.float64)
    x = torch.rand(N, len(box), generator=g, dtype=torch.float64) * b
    x[0], x[1] = 0.0, b
    cols = [torch.sin((5 + 2 * j) * x[:, 0] + j) * torch.cos((2 + j) * x[:, -1]) * (1.0 + 0.5 * j)
            + 0.2 * torch.randn(N, generator=g, dtype=torch.float64) for j in range(_BMAX[case])]
    xn = torch.rand(50, len(box), generator=g, dtype=torch.float64) * b
    return x, torch.stack(cols, dim=1), xn


def _single_model(case, y):
    from efgpnd import EFGPND
    x = _data(case)[0]
    return EFGPND(x.cuda(), y.cuda(), _kernel(case), sigmasq=_SIG[case], eps=EPS, nufft_eps=NUFFT_EPS, estimate_params=False,
                  opts=dict(OPTS))


def _multi_model(case, Y, **opts):
    from efgpnd_multi import EFGPNDMulti
    x = _data(case)[0]
    return EFGPNDMulti(x.cuda(), Y.cuda(), _kernel(case), sigmasq=_SIG[case], eps=EPS, nufft_eps=NUFFT_EPS, estimate_params=False,
                       opts=dict(OPTS, **opts))


@functools.lru_cache(maxsize=None)
def _yardstick(case):
    """Per column of the case: the dense coefficients on the model's grid and the error of a fresh single-output EFGPND against
    them.  Computed once per case and shared.  -> (dense beta (B_max, M), e_single (B_max,), hs, shape)."""
    x, Y, _ = _data(case)
    sig = _SIG[case]
    errs, dense = [], None
    for b in range(Y.shape[1]):
        m = _single_model(case, Y[:, b]).fit()
        st = m._fit_state
        if dense is None:
            _check_route(case, st)
            hs, shape = tuple(st["hs"]), tuple(st["shape"])
            F = D.features(x, hs, shape)
            ws, _ = D.weights(_kernel(case), hs, shape)
            dense = MD.fit(F, Y, ws, sig)
        errs.append(_rel(_np(m._beta), dense[b]))
    return dense, np.asarray(errs), hs, shape


def _fit_errors(model, dense_rows):
    beta = _np(model._beta)
    return np.asarray([_rel(beta[b], dense_rows[b]) for b in range(beta.shape[0])])


# ---- 1. fit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B", [("a", 1), ("a", 2), ("a", 3), ("a", 5), ("b", 3), ("c", 4), ("d", 3), ("e", 2)])
def test_fit_matches_the_dense_solve_as_well_as_single_output_models_do(case, B):
    dense, e_single, hs, shape = _yardstick(case)
    Y = _data(case)[1][:, :B]
    model = _multi_model(case, Y).fit()
    st = model._fit_state
    _check_route(case, st)
    assert tuple(st["shape"]) == shape and tuple(model._beta.shape) == (B, math.prod(shape))
    e_multi = _fit_errors(model, dense)
    stats = model.last_fit_stats
    print(f"\ncase {case} B = {B} grid {shape}: e_multi {e_multi.tolist()} e_single {e_single.tolist()} iters {stats['mean_cg_iters']}")
    assert len(stats["mean_cg_iters"]) == B and all(v > 0 for v in stats["mean_cg_iters"]) and stats["feature_count"] == math.prod(shape)
    assert np.all(e_multi <= 4 * e_single.max()), f"e_multi {e_multi.tolist()} e_single {e_single.tolist()}"


# ---- 2. column scales ---------------------------------------------------------------------------------------------------------------
def test_columns_of_very_different_scales_and_a_zero_column():
    """Columns times 1, 1e-6, 1e6 and 0: every column is held to the bound relative to its own scale (the yardstick is the single-output
    error on the unscaled columns: a relative error does not depend on the units, and a single-output fit of the 1e-6 column would
    measure the CG kernels' absolute guard instead)."""
    dense, e_single, _, _ = _yardstick("a")
    x, Y, xn = _data("a")
    scales = torch.tensor([1.0, 1e-6, 1e6, 0.0], dtype=torch.float64)
    model = _multi_model("a", Y[:, :4] * scales[None, :]).fit()
    beta = _np(model._beta)
    assert np.all(np.isfinite(beta)) and np.all(beta[3] == 0)
    e_multi = np.asarray([_rel(beta[b], dense[b] * float(scales[b])) for b in range(3)])
    print(f"\nscaled columns: e_multi {e_multi.tolist()} e_single {e_single.tolist()} iters {model.last_fit_stats['mean_cg_iters']}")
    assert np.all(e_multi <= 4 * e_single.max()), f"e_multi {e_multi.tolist()} e_single {e_single.tolist()}"
    mean, var = model.predict(xn.cuda(), hutchinson_probes=16)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(var).all())
    assert bool((mean[:, 3] == 0).all())
    lm = model.log_marginal(probes=8, steps=10)
    assert lm.shape == (4,) and bool(torch.isfinite(lm).all())
    grad = model.compute_gradients(trace_samples=2, nufft_eps=NUFFT_EPS, cg_tol=CG_TOL, apply_gradients=False)
    assert bool(torch.isfinite(grad).all())


# ---- 3. B = 1 -------------------------------------------------------------------------------------------------------------------------
def test_one_output_is_the_single_output_model():
    _, e_single, _, _ = _yardstick("a")
    x, Y, xn = _data("a")
    single = _single_model("a", Y[:, 0])
    multi = _multi_model("a", Y[:, :1])
    torch.manual_seed(7)
    m1, v1 = single.predict(xn.cuda(), hutchinson_probes=64)
    torch.manual_seed(7)
    mB, vB = multi.predict(xn.cuda(), hutchinson_probes=64)
    assert tuple(mB.shape) == (50, 1) and tuple(vB.shape) == (50,)
    e_mean, e_var = _rel(_np(mB[:, 0]), _np(m1)), _rel(_np(vB), _np(v1))
    print(f"\nB = 1 against EFGPND: mean {e_mean:.2e} variance {e_var:.2e} bound {4 * e_single.max():.2e}")
    assert e_mean <= 4 * e_single.max() and e_var <= 4 * e_single.max()


# ---- 4. predict ---------------------------------------------------------------------------------------------------------------------
def test_predict_shapes_raster_and_shared_variance():
    _, e_single, _, _ = _yardstick("a")
    x, Y, xn = _data("a")
    multi = _multi_model("a", Y[:, :3])
    torch.manual_seed(11)
    mean, var = multi.predict(xn.cuda(), hutchinson_probes=64)
    assert tuple(mean.shape) == (50, 3) and tuple(var.shape) == (50,)
    torch.manual_seed(11)
    _, v0 = _single_model("a", Y[:, 0]).predict(xn.cuda(), hutchinson_probes=64)
    e_var = _rel(_np(var), _np(v0))
    # the raster: exact on its side, the point transform within the 2 x tolerance contract on the other
    ax = [torch.linspace(0.05, 0.95, 7, dtype=torch.float64), torch.linspace(0.1, 0.9, 5, dtype=torch.float64)]
    gmean, gvar = multi.predict_grid(ax, return_variance=False)
    assert tuple(gmean.shape) == (3, 7, 5) and tuple(gvar.shape) == (7, 5)
    pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 2)
    pmean, _ = multi.predict(pts.cuda(), return_variance=False)
    diff = float((gmean.reshape(3, -1).T - pmean).abs().max())
    bound = 4 * NUFFT_EPS * float(pmean.abs().max())
    print(f"\nraster against points: {diff:.2e} (bound {bound:.2e}); variance against EFGPND {e_var:.2e} (bound {4 * e_single.max():.2e})")
    assert diff <= bound
    assert e_var <= 4 * e_single.max()
    torch.manual_seed(11)
    _, gv = multi.predict_grid(ax, hutchinson_probes=64)
    assert tuple(gv.shape) == (7, 5) and bool(torch.isfinite(gv).all())
    torch.manual_seed(3)                 # the SLQ probes: the keyword of predict returns what log_marginal returns
    with_lm = multi.predict(xn.cuda(), return_variance=False, compute_log_marginal=True)
    torch.manual_seed(3)
    lm = multi.log_marginal()
    assert len(with_lm) == 3 and tuple(lm.shape) == (3,) and bool(torch.isfinite(lm).all())
    assert float((with_lm[2] - lm).abs().max()) <= 1e-12 * float(lm.abs().max())        # same probes, same arithmetic, to rounding


# ---- 5. gradient --------------------------------------------------------------------------------------------------------------------
def _single_gradient_sum(case, Y, seed, nufft_eps, cg_tol):
    total = None
    for b in range(Y.shape[1]):
        torch.manual_seed(seed)
        g = _single_model(case, Y[:, b]).compute_gradients(trace_samples=5, nufft_eps=nufft_eps, cg_tol=cg_tol, apply_gradients=False)
        total = g.detach().cpu().double() if total is None else total + g.detach().cpu().double()
    return total


@pytest.mark.parametrize("case,B", [("a", 3), ("c", 4), ("d", 3), ("e", 2)])
def test_joint_gradient_is_the_sum_of_single_output_gradients(case, B):
    Y = _data(case)[1][:, :B]
    seed = 1234
    model = _multi_model(case, Y)
    torch.manual_seed(seed)
    joint = model.compute_gradients(trace_samples=5, nufft_eps=NUFFT_EPS, cg_tol=CG_TOL, apply_gradients=False).detach().cpu().double()
    coarse = _single_gradient_sum(case, Y, seed, NUFFT_EPS, CG_TOL)
    fine = _single_gradient_sum(case, Y, seed, NUFFT_EPS / 10, CG_TOL / 100)
    sens = float((coarse - fine).abs().max())
    diff = float((joint - coarse).abs().max())
    print(f"\ncase {case} B = {B}: joint {joint.tolist()} sum of singles {coarse.tolist()}\n  difference {diff:.3e}; yardstick's sensitivity "
          f"{sens:.3e} (allowed {10 * sens:.3e})")
    assert joint.shape == coarse.shape and bool(torch.isfinite(joint).all())
    assert diff <= 10 * sens, f"difference {diff:.3e}, 10 x sensitivity {10 * sens:.3e}"
    st = model.last_gradient_stats
    assert st["n_outputs"] == B and tuple(st["rows"].shape) == (B, 4)


# ---- 6. training --------------------------------------------------------------------------------------------------------------------
def test_training_lowers_the_joint_objective():
    x = _data("a")[0]
    Y = torch.as_tensor(MD.draw_columns(x, (0.2, 0.2), 1.0, 0.05, seed=3, B=3))
    import kernels
    from efgpnd_multi import EFGPNDMulti
    kern = kernels.SquaredExponential(dimension=2, init_lengthscale=0.35, init_variance=0.4)
    model = EFGPNDMulti(x.cuda(), Y.cuda(), kern, sigmasq=0.3, eps=EPS, nufft_eps=NUFFT_EPS, estimate_params=False,
                        opts={"cg_tolerance": CG_TOL})

    def objective():
        torch.manual_seed(5)                 # fixed probes of the log-determinant
        return -float(model.log_marginal(probes=50, steps=25).sum())

    first = objective()
    model.optimize_hyperparameters(lr=0.1, max_iters=5, trace_samples=10)
    last = objective()
    hyp = [float(v) for v in model.kernel.get_hypers()] + [float(model.sigmasq.detach())]
    print(f"\njoint negative log marginal: {first:.4f} -> {last:.4f}; hypers {hyp}")
    assert all(math.isfinite(v) and v > 0 for v in hyp)
    assert math.isfinite(first) and math.isfinite(last) and last <= first


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    from efgpnd_multi import EFGPNDMulti
    x, Y, _ = _data("a")
    bad = Y[:, :2].clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="Y has non-finite"):
        EFGPNDMulti(x.cuda(), bad.cuda(), _kernel("a"), sigmasq=0.1, estimate_params=False)
    with pytest.raises(ValueError, match="Y must be 2-D"):
        EFGPNDMulti(x.cuda(), Y[:, 0].cuda(), _kernel("a"), sigmasq=0.1, estimate_params=False)
    with pytest.raises(NotImplementedError, match="shard_points"):
        EFGPNDMulti(x.cuda(), Y[:, :2].cuda(), _kernel("a"), sigmasq=0.1, estimate_params=False, opts={"shard_points": True})


def test_initial_estimate_is_the_geometric_mean_over_columns():
    from efgpnd_multi import EFGPNDMulti
    x, Y, _ = _data("a")
    model = EFGPNDMulti(x.cuda(), Y[:, :3].cuda(), "SE")
    singles = [_kernel("a").estimate_hyperparameters(x, Y[:, b]) for b in range(3)]
    want_var = math.exp(sum(math.log(s[1]) for s in singles) / 3)
    assert abs(float(model.kernel.get_hyper("variance")) - want_var) <= 1e-6 * want_var
    assert abs(float(model.sigmasq.detach()) - 0.2 * want_var) <= 1e-6 * want_var
