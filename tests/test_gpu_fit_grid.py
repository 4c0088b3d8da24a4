"""EFGPND.from_grid: a model fitted from observations on a rectilinear raster, through efgp_hip.RasterPlan (exact separable sums),
against a dense solve of the normal equations and against the point route on the materialised observed cells.

Rasters 12 x 9, 7 x 6 x 5 and 40 cells with non-uniform, unsorted axes, about 20 % of the cells masked (the cells that carry the
axes' extremes stay observed, so both routes see one bounding box), and the hole-free variant of each; sigma^2 = 0.5 and variance
1, so the systems are well conditioned (kappa <= (N max|ws|^2 + 0.5) / 0.5).

Bounds.  beta against the dense solve: the gridded error is at most max(point route's error at nufft_eps = 1e-9, 1e-9) -- the
raster route has no window error.  Fy, v against the point route: 2e-9 sum|y| and 2e-9 N, the transforms' standing "2 x requested
tolerance".  Means and the "regular" variance: 4e-9 kappa relative to the largest value (2e-9 on each side of a solve of condition
kappa).  Gradients and the log marginal likelihood: 10 x the difference of the point route against itself between nufft_eps = 1e-9
and 1e-11, measured in the test on the same data and probes -- that difference is the window error the raster route removes.
Measured on MI355X: see DESIGN.md section 12.
"""
import math

import pytest
import torch

import _raster

pytestmark = pytest.mark.gpu

SIG, CG_TOL, NUFFT_EPS = 0.5, 1e-12, 1e-9
N_AXIS = {"1d": (40,), "2d": (12, 9), "3d": (7, 6, 5)}
CONFIGS = [("2d", "se"), ("2d", "matern"), ("2d", "ard"), ("3d", "matern"), ("3d", "ard"), ("1d", "se"), ("1d", "matern")]
ALL = [(r, k, m) for r, k in CONFIGS for m in (True, False)]
IDS = [f"{r}-{k}-{'masked' if m else 'full'}" for r, k, m in ALL]
_CACHE = {}


def _kernel(name, d):
    import kernels
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    if name == "se":
        return SquaredExponential(dimension=d, init_lengthscale=0.3, init_variance=1.0), 1e-2
    if name == "matern":
        return Matern(dimension=d, nu=1.5, init_lengthscale=0.5, init_variance=1.0), 5e-2
    return kernels.SquaredExponentialARD(dimension=d, init_lengthscale=(0.3, 0.5, 0.4)[:d], init_variance=1.0), 1e-2


def _data(raster, masked):
    """(axes, Y, mask) on the CPU: unsorted non-uniform axes in [0, side_a], the extremes observed."""
    key = ("data", raster, masked)
    if key not in _CACHE:
        n_axis = N_AXIS[raster]
        g = torch.Generator().manual_seed(11 + len(n_axis))
        sides = (1.0, 0.8, 0.9)[:len(n_axis)]
        axes = [torch.rand(n, generator=g, dtype=torch.float64) * s for n, s in zip(n_axis, sides)]
        pts = _raster.meshgrid_points(axes)
        Y = (torch.sin(5 * pts[:, 0]) * torch.cos(2 * pts[:, -1]) + math.sqrt(SIG) * torch.randn(pts.shape[0], generator=g, dtype=torch.float64))
        Y = Y.reshape(n_axis)
        mask = torch.ones(n_axis, dtype=torch.bool)
        if masked:
            mask = torch.rand(n_axis, generator=g) >= 0.2
            mask[tuple(int(a.argmin()) for a in axes)] = True
            mask[tuple(int(a.argmax()) for a in axes)] = True
        _CACHE[key] = (axes, Y, mask)
    return _CACHE[key]


def _grid_model(raster, kname, masked, fit=True, **opts):
    from efgpnd import EFGPND
    axes, Y, mask = _data(raster, masked)
    kern, eps = _kernel(kname, len(axes))
    m = EFGPND.from_grid([a.cuda() for a in axes], Y.cuda(), kern, mask=mask.cuda() if masked else None, sigmasq=SIG, eps=eps,
                         nufft_eps=NUFFT_EPS, estimate_params=False, opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False, **opts})
    return m.fit() if fit else m


def _point_model(raster, kname, masked, nufft_eps=NUFFT_EPS, fit=True):
    from efgpnd import EFGPND
    axes, Y, mask = _data(raster, masked)
    kern, eps = _kernel(kname, len(axes))
    keep = mask.reshape(-1)
    x = _raster.meshgrid_points(axes)[keep]
    m = EFGPND(x.cuda(), Y.reshape(-1)[keep].cuda(), kern, sigmasq=SIG, eps=eps, nufft_eps=nufft_eps, estimate_params=False,
               opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False})
    return m.fit() if fit else m


def _pair(raster, kname, masked):
    key = ("pair", raster, kname, masked)
    if key not in _CACHE:
        _CACHE[key] = (_grid_model(raster, kname, masked), _point_model(raster, kname, masked))
    return _CACHE[key]


def _dense_beta(model, raster, masked):
    """The solution of (D F*F D + sigma^2 I) beta = D F* y over the observed cells, in complex128 on the CPU."""
    axes, Y, mask = _data(raster, masked)
    st = model._fit_state
    shape, hs = tuple(st["shape"]), tuple(st["hs"])
    tabs = _raster.tables(axes, hs, shape, isign=+1)
    spec = {1: "ik->ik", 2: "ik,jl->ijkl", 3: "ik,jl,nm->ijnklm"}[len(shape)]
    F = torch.einsum(spec, *tabs).reshape(mask.numel(), -1)[mask.reshape(-1)]
    ws = st["ws"].detach().cpu().reshape(-1)
    A = ws[:, None] * (F.conj().T @ F) * ws[None, :] + SIG * torch.eye(ws.numel(), dtype=torch.complex128)
    rhs = ws * (F.conj().T @ Y.reshape(-1)[mask.reshape(-1)].to(torch.complex128))
    return torch.linalg.solve(A, rhs)


def _kappa(model):
    st = model._fit_state
    return (model._devdata["N"] * float(st["ws"].abs().max()) ** 2 + SIG) / SIG


@pytest.mark.parametrize("raster,kname,masked", ALL, ids=IDS)
def test_beta_against_the_dense_solve(raster, kname, masked):
    """The gridded error in beta is at most max(the point route's error at nufft_eps = 1e-9, 1e-9).

    Measured on MI355X (relative 2-norm): gridded 1e-15 .. 2e-11, point route 6e-11 .. 4e-9.  The point route's 2-D and 3-D
    figures (5.6e-10 .. 4e-9) are not its window error (its F* y is within 8e-11 of a dense F* y) but the mean solve's: the CG
    kernels guard <r, z> and <p, A p> with an absolute 1e-16, which stalls them near |r| = 1e-8, and for data of order one the
    solve runs to its cap of 2 M iterations with a relative residual near 1e-10.  The gridded fit solves for 2^k y and scales
    beta back (exact), which takes that floor away; without it both routes sat at 5e-10 .. 4e-9."""
    mg, mp = _pair(raster, kname, masked)
    assert mg.last_fit_stats["route"] == "raster" and "route" not in mp.last_fit_stats
    assert mg._devdata["points"] is None and mg._devdata["x"] is None
    assert tuple(mg._fit_state["shape"]) == tuple(mp._fit_state["shape"]) and tuple(mg._fit_state["hs"]) == tuple(mp._fit_state["hs"])
    truth = _dense_beta(mg, raster, masked)
    eg = float((mg._fit_state["beta"].cpu().reshape(-1) - truth).norm() / truth.norm())
    ep = float((mp._fit_state["beta"].cpu().reshape(-1) - truth).norm() / truth.norm())
    print(f"\n{raster} {kname} masked={masked} M={truth.numel()}: beta error gridded {eg:.2e}, point route {ep:.2e}")
    assert eg <= max(ep, 1e-9)


@pytest.mark.parametrize("raster,kname,masked", ALL, ids=IDS)
def test_fit_state_and_predictions_against_the_point_route(raster, kname, masked):
    mg, mp = _pair(raster, kname, masked)
    axes, Y, mask = _data(raster, masked)
    N = int(mask.sum())
    assert mg._devdata["N"] == N == mp._devdata["N"]
    ysum = float(Y[mask].abs().sum())
    e_fy = float((mg._fit_state["Fy"] - mp._fit_state["Fy"]).abs().max())
    e_v = float((mg._fit_state["v"] - mp._fit_state["v"]).abs().max())
    print(f"\n{raster} {kname} masked={masked}: |Fy diff| {e_fy:.2e} (bound {2e-9 * ysum:.2e}), |v diff| {e_v:.2e} (bound {2e-9 * N:.2e})")
    assert e_fy <= 2e-9 * ysum and e_v <= 2e-9 * N
    bound = 4e-9 * _kappa(mg)
    assert bound <= 1e-6
    g = torch.Generator().manual_seed(5)
    sides = torch.tensor([float(a.max()) for a in axes], dtype=torch.float64)
    x_new = (torch.rand(50, len(axes), generator=g, dtype=torch.float64) * sides).cuda()
    mean_g, var_g = mg.predict(x_new, variance_method="regular")
    mean_p, var_p = mp.predict(x_new, variance_method="regular")
    e_mean = float((mean_g - mean_p).abs().max() / mean_p.abs().max())
    e_var = float((var_g - var_p).abs().max() / var_p.abs().max())
    new_axes = [torch.rand(n, generator=g, dtype=torch.float64) * s for n, s in zip((7, 5, 4), sides.tolist())]
    map_g, _ = mg.predict_grid(new_axes if len(axes) > 1 else new_axes[0], return_variance=False)
    map_p, _ = mp.predict_grid(new_axes if len(axes) > 1 else new_axes[0], return_variance=False)
    e_map = float((map_g - map_p).abs().max() / map_p.abs().max())
    print(f"kappa bound {bound:.2e}: predict mean {e_mean:.2e}, regular variance {e_var:.2e}, predict_grid mean {e_map:.2e}")
    assert e_mean <= bound and e_var <= bound and e_map <= bound
    sv_g = mg.predict(x_new, variance_method="stochastic", hutchinson_probes=16)[1]
    assert tuple(sv_g.shape) == (50,) and bool(torch.isfinite(sv_g).all())
    assert mg._devdata["points"] is None


GRAD_CASES = [("2d", "se", True), ("2d", "ard", False), ("3d", "matern", True), ("1d", "se", True)]


@pytest.mark.parametrize("raster,kname,masked", GRAD_CASES, ids=[f"{r}-{k}-{'masked' if m else 'full'}" for r, k, m in GRAD_CASES])
def test_gradient_and_log_marginal_against_the_point_route(raster, kname, masked):
    """Supplied probes_Z (T, cells) on the raster -- the point model gets the columns of the observed cells -- and probes_V; fixed
    Lanczos probe vectors.  Tolerance: 10 x |point route at 1e-9 - point route at 1e-11|, measured here; on MI355X that difference
    was 1e-12 .. 3e-10 of the gradient's largest entry and the gridded model sat within it."""
    axes, Y, mask = _data(raster, masked)
    mg = _grid_model(raster, kname, masked, fit=False)
    p9, p11 = _point_model(raster, kname, masked, 1e-9, fit=False), _point_model(raster, kname, masked, 1e-11, fit=False)
    T, g = 4, torch.Generator().manual_seed(9)
    Z = (torch.randint(0, 2, (T, mask.numel()), generator=g) * 2 - 1).to(torch.float64)
    mg.fit()
    M = mg._fit_state["ws"].numel()
    V = (torch.randint(0, 2, (T, M), generator=g) * 2 - 1).to(torch.float64)
    LZ = (torch.randint(0, 2, (8, M), generator=g) * 2 - 1).to(torch.float64)
    common = dict(trace_samples=T, cg_tol=1e-12, probes_V=V.cuda(), apply_gradients=False, compute_log_marginal=True,
                  log_marginal_probe_vectors=LZ.cuda(), log_marginal_steps=10)
    gg, lg = mg.compute_gradients(probes_Z=Z.cuda(), nufft_eps=1e-9, **common)
    Zp = Z[:, mask.reshape(-1)].contiguous().cuda()
    g9, l9 = p9.compute_gradients(probes_Z=Zp, nufft_eps=1e-9, **common)
    g11, l11 = p11.compute_gradients(probes_Z=Zp, nufft_eps=1e-11, **common)
    assert mg._devdata["points"] is None
    scale = float(g11.abs().max())
    self_diff = float((g9 - g11).abs().max())
    diff = float((gg - g11).abs().max())
    l_self, l_diff = abs(float(l9) - float(l11)), abs(float(lg) - float(l11))
    print(f"\n{raster} {kname} masked={masked}: gradient {g11.tolist()}\n  point route 1e-9 vs 1e-11: {self_diff:.2e} ({self_diff / scale:.2e} rel); "
          f"gridded vs point 1e-11: {diff:.2e} ({diff / scale:.2e} rel)\n  log marginal {float(l11):.6f}: point self {l_self:.2e}, gridded {l_diff:.2e}")
    assert diff <= 10 * self_diff
    assert l_diff <= 10 * l_self


def test_generated_probes_give_a_repeatable_gradient():
    """Z generated from probe_seed inside RasterPlan.type1_rademacher (V, which lives on the mode grid, is supplied)."""
    mg = _grid_model("2d", "se", True)
    M = mg._fit_state["ws"].numel()
    V = (torch.randint(0, 2, (4, M), generator=torch.Generator().manual_seed(2)) * 2 - 1).to(torch.float64).cuda()
    a = mg.compute_gradients(trace_samples=4, probe_seed=17, probes_V=V, apply_gradients=False)
    b = mg.compute_gradients(trace_samples=4, probe_seed=17, probes_V=V, apply_gradients=False)
    c = mg.compute_gradients(trace_samples=4, probe_seed=18, probes_V=V, apply_gradients=False)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and not torch.equal(a, c)
    assert mg._devdata["points"] is None


@pytest.mark.parametrize("raster", ["2d", "3d", "1d"])
def test_samples(raster):
    mg, _ = _pair(raster, "se" if raster != "3d" else "matern", True)
    axes, _, _ = _data(raster, True)
    d = len(axes)
    g = torch.Generator().manual_seed(3)
    x_new = (torch.rand(5, d, generator=g, dtype=torch.float64) * 0.8).cuda()
    a = mg.sample_paths(x_new, 8, seed=3)
    b = mg.sample_paths(x_new, 8, seed=3)
    assert tuple(a.shape) == (8, 5) and torch.equal(a, b)
    assert mg._devdata["points"] is None
    new_axes = [torch.rand(n, generator=g, dtype=torch.float64) * 0.8 for n in (6, 4, 3)[:d]]
    maps = mg.sample_paths_grid(new_axes if d > 1 else new_axes[0], 3, seed=4)
    assert tuple(maps.shape) == (3,) + tuple(len(a) for a in new_axes) and bool(torch.isfinite(maps).all())
    draws = mg.sample_paths(x_new, 2000, seed=12, cg_tolerance=1e-8)
    mean, _ = mg.predict(x_new, return_variance=False)
    se = draws.std(dim=0) / math.sqrt(2000)
    z = ((draws.mean(dim=0) - mean).abs() / se).max().item()
    print(f"\n{raster}: sample mean of 2000 draws within {z:.2f} standard errors of the posterior mean")
    assert z <= 5
    post = mg.sample_posterior(x_new, 4, method="efgp", seed=5)
    assert post.shape == (5, 4)


@pytest.mark.parametrize("raster", ["2d", "3d", "1d"])
def test_nan_cells_are_the_mask(raster):
    from efgpnd import EFGPND
    axes, Y, mask = _data(raster, True)
    kern1, eps = _kernel("se", len(axes))
    kern2, _ = _kernel("se", len(axes))
    Ynan = Y.clone()
    Ynan[~mask] = float("nan")
    Yany = Y.clone()
    Yany[~mask] = 1e6
    opts = {"cg_tolerance": CG_TOL}
    a = EFGPND.from_grid([x.cuda() for x in axes], Ynan.cuda(), kern1, sigmasq=SIG, eps=eps, estimate_params=False, opts=opts).fit()
    b = EFGPND.from_grid([x.cuda() for x in axes], Yany.cuda(), kern2, mask=mask.cuda(), sigmasq=SIG, eps=eps, estimate_params=False, opts=opts).fit()
    assert a.last_fit_stats["route"] == "raster" == b.last_fit_stats["route"]
    assert a._devdata["N"] == int(mask.sum()) == b._devdata["N"]
    assert torch.equal(torch.view_as_real(a._fit_state["beta"]), torch.view_as_real(b._fit_state["beta"]))


def test_refusals_name_the_gridded_model():
    from efgpnd import EFGPND
    axes, Y, mask = _data("2d", True)
    ax = [x.cuda() for x in axes]
    kern, eps = _kernel("se", 2)
    with pytest.raises(NotImplementedError, match="gridded model"):
        EFGPND.from_grid(ax, Y.cuda(), kern, sigmasq=SIG, eps=eps, estimate_params=False, opts={"shard_points": True})
    with pytest.raises(ValueError, match="no observed cell"):
        EFGPND.from_grid(ax, Y.cuda(), kern, mask=torch.zeros_like(mask).cuda(), sigmasq=SIG, eps=eps, estimate_params=False)
    with pytest.raises(ValueError, match="no observed cell"):
        EFGPND.from_grid(ax, torch.full_like(Y, float("nan")).cuda(), kern, sigmasq=SIG, eps=eps, estimate_params=False)
    with pytest.raises(ValueError, match="Y has shape"):
        EFGPND.from_grid(ax, Y.T.contiguous().cuda(), kern, sigmasq=SIG, eps=eps, estimate_params=False)
    with pytest.raises(ValueError, match="axes"):
        EFGPND.from_grid(ax[:1], Y.cuda(), kern, sigmasq=SIG, eps=eps, estimate_params=False)
    with pytest.raises(ValueError, match="mask must be"):
        EFGPND.from_grid(ax, Y.cuda(), kern, mask=mask.to(torch.float64).cuda(), sigmasq=SIG, eps=eps, estimate_params=False)
    mg, _ = _pair("2d", "se", True)
    with pytest.raises(NotImplementedError, match="gridded model"):
        mg.compute_gradients(trace_samples=2, trace_mode="reference", apply_gradients=False)
    with pytest.raises(NotImplementedError, match="gridded model"):
        mg.compute_gradients(trace_samples=2, pointwise_alpha=True, apply_gradients=False)
    with pytest.raises(NotImplementedError, match="gridded model"):
        mg.sample_posterior(torch.zeros(3, 2, dtype=torch.float64).cuda(), 2, method="dense")
    from efgp_hip import RasterPlan
    with pytest.raises(NotImplementedError):
        RasterPlan(ax, 0.5).type2(torch.ones(3, 3, dtype=torch.complex128).cuda(), (3, 3))


def test_optimisation_runs_and_moves_the_parameters():
    from efgpnd import EFGPND
    axes, Y, mask = _data("2d", True)
    kern, eps = _kernel("se", 2)
    m = EFGPND.from_grid([x.cuda() for x in axes], Y.cuda(), kern, mask=mask.cuda(), eps=eps, estimate_params=True)
    before = m._gp_params.raw.detach().clone()
    m.optimize_hyperparameters(max_iters=3, trace_samples=4)
    after = m._gp_params.raw.detach()
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    assert m.last_fit_stats["route"] == "raster" and m._devdata["points"] is None
    mean, _ = m.predict_grid(axes, return_variance=False)
    assert tuple(mean.shape) == tuple(Y.shape) and bool(torch.isfinite(mean).all())
