"""EFGPND.predict_grid / sample_paths_grid against the exact sums of tests/_nudft.py and against predict / sample_paths at the
meshgrid points.  Models of N = 2000 points at nufft_eps = 1e-9 and cg_tolerance = 1e-10.

Bounds: the raster transform against the exact sums, 1e-11 sum |ws beta| (tests/test_gpu_raster.py; an ARD grid is brought to one
spacing by rescaling the axes, a fourth rounding of the phase: 2 pi 70 * 4 * 2^-53 = 2e-13 per term); against the NUFFT routes,
2 nufft_eps sum |modes| -- the project's standing claim for every transform.
"""
import math

import pytest
import torch

import _nudft as E
import _raster

pytestmark = pytest.mark.gpu

NUFFT_EPS, CG_TOL, N = 1e-9, 1e-10, 2000
DRAW_TOL = 1e-6        # the noise solves of the draws: their broad right-hand sides do not reach 1e-10 within the iteration cap


def _kernel(case):
    import kernels
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    if case == "se2d":
        return SquaredExponential(dimension=2, init_lengthscale=0.3, init_variance=1.5), (1.0, 1.0), 1e-3, 0.1
    if case == "maternard2d":
        return kernels.MaternARD(dimension=2, nu=1.5, init_lengthscale=(0.3, 0.6), init_variance=1.0), (2.0, 1.0), 1e-2, 0.1
    if case == "se1d":
        return SquaredExponential(dimension=1, init_lengthscale=0.2, init_variance=1.3), (1.0,), 1e-4, 0.15
    return Matern(dimension=3, nu=1.5, init_lengthscale=0.5, init_variance=1.3), (1.0, 1.0, 1.0), 1e-2, 0.2


AXIS_LENGTHS = {"se2d": (19, 33), "maternard2d": (17, 30), "se1d": (70,), "matern3d": (7, 18, 5)}
_CACHE = {}


def _model(case, dtype=torch.float64, **opts):
    """(model, axes on the CPU): N points in the box (two of them its corners), axes inside it, unsorted."""
    from efgpnd import EFGPND
    key = (case, dtype, tuple(sorted(opts)))
    if key in _CACHE:
        return _CACHE[key]
    kern, box, eps, sig = _kernel(case)
    g = torch.Generator().manual_seed(31 + len(box))
    b = torch.tensor(box, dtype=torch.float64)
    x = torch.rand(N, len(box), generator=g, dtype=torch.float64) * b
    x[0], x[1] = 0.0, b
    y = torch.sin(5 * x[:, 0]) * torch.cos(2 * x[:, -1]) + math.sqrt(sig) * torch.randn(N, generator=g, dtype=torch.float64)
    axes = [torch.rand(n, generator=g, dtype=torch.float64) * b[a] for a, n in enumerate(AXIS_LENGTHS[case])]
    m = EFGPND(x.to(dtype).cuda(), y.to(dtype).cuda(), kern, sigmasq=sig, eps=eps, nufft_eps=NUFFT_EPS, estimate_params=False,
               opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False, **opts})
    if not opts:
        m.fit()
    _CACHE[key] = (m, axes)
    return m, axes


def _points(axes):
    return _raster.meshgrid_points(axes).cuda()


def _exact(axes, hs, shape, f, modeord=0, mode_scale=None):
    """Exact real sums at the meshgrid points -> (*n_axis), and sum |f scale|; axes rescaled to the first spacing."""
    pts = _raster.meshgrid_points([a * (hs[i] / hs[0]) for i, a in enumerate(axes)])
    f = f.detach().cpu().reshape(shape)
    sc = None if mode_scale is None else mode_scale.detach().cpu().reshape(shape)
    val = E.type2(pts, hs[0], f, shape, modeord=modeord, mode_scale=sc).real
    return val.reshape(tuple(len(a) for a in axes)), float((f if sc is None else f * sc).abs().sum())


CASES = ["se2d", "maternard2d", "se1d", "matern3d"]


@pytest.mark.parametrize("case", CASES)
def test_mean_is_the_exact_sum_and_agrees_with_predict(case):
    m, axes = _model(case)
    st = m._fit_state
    hs, shape = tuple(st["hs"]), tuple(st["shape"])
    for a, ax in enumerate(axes):
        assert hs[a] * (shape[a] // 2) * float(ax.abs().max()) <= 70
    mean, var = m.predict_grid(axes if case != "se1d" else axes[0], return_variance=False)
    n_axis = tuple(len(a) for a in axes)
    assert tuple(mean.shape) == n_axis == tuple(var.shape) and mean.dtype == torch.float64 and mean.device == m.device
    assert bool(torch.isnan(var).all()) and var.dtype == torch.float64 and var.device == m.device
    want, mag = _exact(axes, hs, shape, st["beta"], mode_scale=st["ws"])
    e_exact = float((mean.cpu() - want).abs().max()) / mag
    ref, _ = m.predict(_points(axes), return_variance=False)
    e_nufft = float((mean.reshape(-1) - ref).abs().max()) / mag
    print(f"\n{case} modes {shape} raster {n_axis}: against the exact sums {e_exact:.2e}, against predict {e_nufft:.2e} (of sum |ws beta|)")
    assert e_exact <= 1e-11
    assert e_nufft <= 2 * NUFFT_EPS


def test_float32_data_gives_float32_maps():
    m, axes = _model("se2d", dtype=torch.float32)
    mean, var = m.predict_grid([a.numpy() for a in axes], variance_probes=_probes(m, 4))
    assert mean.dtype == var.dtype == torch.float32 and mean.device == var.device == m.device
    assert tuple(mean.shape) == tuple(var.shape) == AXIS_LENGTHS["se2d"]
    ref, _ = m.predict(_points(axes).float(), return_variance=False)
    assert float((mean.reshape(-1) - ref).abs().max()) <= 1e-4 * float(ref.abs().max())      # both rounded to float32 on the way out


def _probes(m, J, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (J, m._fit_state["ws"].numel()), generator=g) * 2 - 1).to(torch.float64)


@pytest.mark.parametrize("case", CASES)
def test_stochastic_variance_agrees_with_predict(case):
    from efgpnd import create_A_var, diag_sums_nd
    m, axes = _model(case)
    st = m._fit_state
    probes = _probes(m, 6)
    _, var = m.predict_grid(axes, variance_probes=probes)
    _, ref = m.predict(_points(axes), variance_probes=probes)
    c = diag_sums_nd(create_A_var(st["ws"], m._toeplitz, st["sig"], torch.complex128), 6, m._xis.to(torch.float64),
                     m.opts.get("max_cg_iterations", 1000), CG_TOL, st["ws"], probes=probes, shape=st["shape"] if st["ard"] else None)
    mag = float(c.abs().sum())
    lag_box = tuple(2 * n - 1 for n in st["shape"])
    assert tuple(c.shape) == lag_box
    want, _ = _exact(axes, tuple(st["hs"]), lag_box, c, modeord=1)
    e_exact = float((var.cpu() - want).abs().max()) / mag
    e_nufft = float((var.reshape(-1) - ref).abs().max()) / mag
    print(f"\n{case} lag box {lag_box}: against the exact sums {e_exact:.2e}, against predict {e_nufft:.2e} (of sum |c|)")
    assert tuple(var.shape) == AXIS_LENGTHS[case]
    assert e_nufft <= 2 * NUFFT_EPS


@pytest.mark.parametrize("case", CASES)
def test_regular_variance_is_predicts(case):
    m, axes = _model(case)
    assert math.prod(AXIS_LENGTHS[case]) < 8192
    _, var = m.predict_grid(axes, variance_method="regular")
    _, ref = m.predict(_points(axes), variance_method="regular")
    assert tuple(var.shape) == AXIS_LENGTHS[case]
    assert torch.equal(var.reshape(-1), ref)


@pytest.mark.parametrize("prior", [False, True], ids=["posterior", "prior"])
@pytest.mark.parametrize("case", CASES)
def test_draws_are_those_of_sample_paths(case, prior):
    m, axes = _model(case)
    st = m._fit_state
    seed = 20240611
    ref, state = m.sample_paths(_points(axes), 4, seed=seed, prior=prior, cg_tolerance=DRAW_TOL, return_state=True)
    again = m.sample_paths(_points(axes), 4, seed=seed, prior=prior, cg_tolerance=DRAW_TOL)
    assert torch.equal(again, ref)                                               # the refactored sampler reproduces itself
    got = m.sample_paths_grid(axes, 4, seed=seed, prior=prior, cg_tolerance=DRAW_TOL)
    assert tuple(got.shape) == (4,) + AXIS_LENGTHS[case] and got.dtype == torch.float64 and got.device == m.device
    assert m.last_sample_stats["seed"] == seed and m.last_sample_stats["nsamples"] == 4
    mag = float((st["ws"].reshape(1, -1) * state["weights"]).abs().sum(dim=1).max())
    err = float((got.reshape(4, -1) - ref).abs().max()) / mag
    want = torch.stack([_exact(axes, tuple(st["hs"]), tuple(st["shape"]), w, mode_scale=st["ws"])[0] for w in state["weights"]])
    e_exact = float((got.cpu() - want).abs().max()) / mag
    print(f"\n{case} prior={prior}: against sample_paths {err:.2e}, against the exact sums of its weights {e_exact:.2e} (of max sum |ws w|)")
    assert err <= 2 * NUFFT_EPS
    assert e_exact <= 1e-11


def test_refusals():
    m, axes = _model("se2d")
    with pytest.raises(ValueError, match="axes"):
        m.predict_grid(axes[:1])
    with pytest.raises(ValueError, match="axes"):
        m.sample_paths_grid(axes + axes[:1], 2)
    with pytest.raises(ValueError, match="empty"):
        m.predict_grid([axes[0], axes[1][:0]])
    bad = axes[1].clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        m.predict_grid([axes[0], bad])
    with pytest.raises(ValueError, match="non-finite"):
        m.sample_paths_grid([axes[0], bad], 2)
    with pytest.raises(ValueError, match="1-D"):
        m.predict_grid([axes[0], axes[1].reshape(-1, 1)])
    with pytest.raises(ValueError, match="nsamples"):
        m.sample_paths_grid(axes, 0)
    with pytest.raises(ValueError, match="Variance method"):
        m.predict_grid(axes, variance_method="exact")
    sharded, _ = _model("se2d", shard_points=True)
    with pytest.raises(NotImplementedError, match="shard_points"):
        sharded.predict_grid(axes)
    with pytest.raises(NotImplementedError, match="shard_points"):
        sharded.sample_paths_grid(axes, 2)
