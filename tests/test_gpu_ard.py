"""GPU tests of the ARD kernels on per-axis Fourier grids: the `_nd` entry points against their formulas, and EFGPND with an ARD
kernel (fit, mean, both variances, gradient, training, draws) against the dense restatements of tests/_ard_dense.py.

Where a bound is "what the isotropic model achieves against the same kind of reference, times a margin", the isotropic figure is
measured in the same test on the code paths that existed before the ARD kernels, and every figure is printed before it is
asserted.  rel(a, b) = max|a - b| / max|b| throughout.
"""
import math

import numpy as np
import pytest
import torch

import _ard_dense as D
import _cg_routes as R
import _nudft as E

pytestmark = pytest.mark.gpu

_CD = torch.complex128


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _np(t):
    return t.detach().cpu().numpy()


def _data(N, box, seed, n_new=40, noise=0.2):
    """N points in the box (two of them its opposite corners, so the box sides are exact), a smooth target plus noise, new points."""
    g = torch.Generator().manual_seed(seed)
    b = torch.tensor(box, dtype=torch.float64)
    x = torch.rand(N, len(box), generator=g, dtype=torch.float64) * b
    x[0], x[1] = 0.0, b
    y = torch.sin(9 * x[:, 0]) * torch.cos(2 * x[:, -1]) + noise * torch.randn(N, generator=g, dtype=torch.float64)
    xn = torch.rand(n_new, len(box), generator=g, dtype=torch.float64) * b
    return x, y, xn


def _model(kernel, x, y, sig, eps, cg_tol=1e-10, nufft_eps=1e-9, **opts):
    from efgpnd import EFGPND
    return EFGPND(x.cuda(), y.cuda(), kernel, sigmasq=sig, eps=eps, nufft_eps=nufft_eps, estimate_params=False,
                  opts={"cg_tolerance": cg_tol, "mean_cg_warm_start": False, **opts})


def _grid_of(model):
    """(hs, shape) of a fitted model, isotropic or ARD."""
    st = model._fit_state
    return tuple(st["hs"]), tuple(st["shape"])


def _restate(model, kernel, x, y, xn, sig, want_var=True):
    """Mean (and 'regular' variance) of the dense feature-space restatement on the model's own grid."""
    hs, shape = _grid_of(model)
    F, Fn = D.features(x, hs, shape), D.features(xn, hs, shape)
    ws, _ = D.weights(kernel, hs, shape)
    m = D.mean(Fn, ws, D.fit(F, y, ws, sig))
    return m, (D.variance_regular(F, Fn, ws, sig) if want_var else None)


# ---- entry points -----------------------------------------------------------------------------------------------------------------
_KERNELS = {
    "se1": lambda: ("SquaredExponentialARD", dict(dimension=1, init_lengthscale=(0.1,), init_variance=1.3)),
    "se2": lambda: ("SquaredExponentialARD", dict(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.3)),
    "se3": lambda: ("SquaredExponentialARD", dict(dimension=3, init_lengthscale=(0.1, 0.5, 0.3), init_variance=0.8)),
    "m2": lambda: ("MaternARD", dict(dimension=2, nu=1.5, init_lengthscale=(0.15, 0.6), init_variance=1.0)),
    "m3": lambda: ("MaternARD", dict(dimension=3, nu=2.5, init_lengthscale=(0.3, 0.2, 0.7), init_variance=1.5)),
}


def _kernel(name):
    import kernels
    cls, kw = _KERNELS[name]()
    return getattr(kernels, cls)(**kw)


@pytest.mark.parametrize("name,hs,shape", [("se1", (0.7,), (9,)), ("se2", (0.744, 0.409), (27, 9)), ("m2", (0.556, 0.278), (27, 9)),
                                           ("se2", (0.9, 0.31), (3, 11)), ("m2", (0.9, 0.31), (3, 11)),
                                           ("se3", (0.73, 0.42, 0.66), (5, 3, 7)), ("m3", (0.73, 0.42, 0.66), (5, 3, 7))])
def test_device_weights_equal_the_host_twin(name, hs, shape):
    from efgp_hip import spectral_weights_host_nd, spectral_weights_nd
    k = _kernel(name)
    dev = torch.device("cuda", 0)
    ws, dp = spectral_weights_nd(dev, k.ard_kind, k.nu, k.lengthscales, k.variance, hs, shape, want_grad=True)
    wh, dh = spectral_weights_host_nd(k.ard_kind, k.nu, k.lengthscales, k.variance, hs, shape, want_grad=True)
    assert ws.shape == wh.shape and dp.shape == dh.shape == (math.prod(shape), len(shape) + 1)
    assert float(ws.imag.abs().max()) == 0.0 and float(dp.imag.abs().max()) == 0.0
    e_ws, e_dp = _rel(_np(ws.real), wh.real.numpy()), _rel(_np(dp.real), dh.real.numpy())
    print(f"\n{name} {shape}: ws {e_ws:.2e} dprime {e_dp:.2e}")
    assert e_ws < 1e-12 and e_dp < 1e-12
    ws_only, none = spectral_weights_nd(dev, k.ard_kind, k.nu, k.lengthscales, k.variance, hs, shape)
    assert none is None and torch.equal(ws_only, ws)                       # same values with and without the derivative rows


def _brute_lag_sums(gamma, eta, shape):
    """c[r] = mean_j sum_{k - l = r} gamma_j[k] eta_j[l], stored at r mod (2 n - 1) per axis."""
    k = D.mode_numbers(shape).astype(np.int64)
    box = tuple(2 * n - 1 for n in shape)
    out = np.zeros(box, dtype=np.complex128)
    for j in range(gamma.shape[0]):
        for a in range(len(k)):
            r = (k[a][None, :] - k) % np.asarray(box)[None, :]
            np.add.at(out, tuple(r.T), gamma[j, a] * eta[j])
    return out / gamma.shape[0]


@pytest.mark.parametrize("shape", [(5, 3), (3, 5, 7)])
def test_lag_sums_nd_equal_the_brute_force_correlation(shape):
    from efgp_hip import lag_sums
    g = torch.Generator().manual_seed(sum(shape))
    M = math.prod(shape)
    gamma = torch.complex(torch.randn(3, M, generator=g, dtype=torch.float64), torch.randn(3, M, generator=g, dtype=torch.float64))
    eta = (torch.randint(0, 2, (3, M), generator=g) * 2 - 1).to(torch.float64)
    out = lag_sums(gamma.cuda(), eta.cuda(), tuple(shape), len(shape))
    assert tuple(out.shape) == tuple(2 * n - 1 for n in shape)
    err = _rel(_np(out), _brute_lag_sums(gamma.numpy(), eta.numpy(), shape))
    print(f"\nlag sums {shape}: {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("shape,hs", [((7, 3), (0.7, 0.4)), ((3, 5, 3), (0.9, 0.35, 0.6))])
def test_variance_kernels_nd_equal_their_formulas(shape, hs):
    from efgp_hip import variance_contract, variance_rhs
    g = torch.Generator().manual_seed(sum(shape) + 1)
    d, M = len(shape), math.prod(shape)
    x = torch.rand(4, d, generator=g, dtype=torch.float64) * 2 - 0.5
    ws = torch.complex(torch.rand(M, generator=g, dtype=torch.float64), 0.1 * torch.randn(M, generator=g, dtype=torch.float64))
    gam = torch.complex(torch.randn(4, M, generator=g, dtype=torch.float64), torch.randn(4, M, generator=g, dtype=torch.float64))
    F = D.features(x, hs, shape)
    rhs = variance_rhs(x.cuda(), tuple(hs), tuple(shape), ws.cuda())
    e_rhs = _rel(_np(rhs), ws.numpy()[None, :] * F.conj())
    full = (F * ws.numpy()[None, :] * gam.numpy()).sum(1).real
    sign = np.where(full > 0, 1.0, -1.0)                       # both signs of the sum: the clamp at zero and the value
    gam2 = gam * torch.as_tensor(sign)[:, None]
    out = variance_contract(x.cuda(), tuple(hs), tuple(shape), ws.cuda(), gam2.cuda())
    e_out = _rel(_np(out), np.abs(full))
    out_neg = variance_contract(x.cuda(), tuple(hs), tuple(shape), ws.cuda(), (-gam2).cuda())
    print(f"\nvariance kernels {shape}: rhs {e_rhs:.2e} contract {e_out:.2e}")
    assert e_rhs < 1e-12 and e_out < 1e-12 and float(out_neg.abs().max()) == 0.0
    with pytest.raises(ValueError):
        variance_rhs(x.cuda(), tuple(hs), tuple(n + 1 for n in shape), torch.zeros(math.prod(n + 1 for n in shape), dtype=_CD).cuda())


@pytest.mark.parametrize("tol", [1e-4, 6e-8, 1e-10])
def test_per_axis_plan_holds_the_exact_sums(tol):
    """efgp_nufft_create_nd with h = (0.7, 0.4) at modes (27, 9): type 1 and type 2 within 2 x tolerance (+ 1e-13) of the exact
    sums, the contract of tests/test_gpu_nufft_options.py.  The exact sums with a spacing per axis are those with spacing 1 at the
    points (h_a x_a)."""
    from efgp_hip import NufftPlan
    hs, shape, N = (0.7, 0.4), (27, 9), 400
    g = torch.Generator().manual_seed(4)
    x = torch.rand(N, 2, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.3], dtype=torch.float64)
    c = torch.complex(torch.randn(N, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64))
    f = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))
    xs = x * torch.tensor(hs, dtype=torch.float64)
    plan = NufftPlan(x.cuda(), hs, tol)
    bar = 2 * tol + 1e-13

    def l2(a, b):
        return float(torch.linalg.norm((a.cpu() - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))

    e1 = l2(plan.type1(c.cuda(), shape), E.type1(xs, 1.0, c, shape))
    e2 = l2(plan.type2(f.cuda(), shape), E.type2(xs, 1.0, f, shape))
    e1r = l2(plan.type1(c.real.contiguous().cuda(), shape), E.type1(xs, 1.0, c.real, shape))
    print(f"\nper-axis plan tol {tol:g}: type 1 {e1:.2e} (real rows {e1r:.2e}) type 2 {e2:.2e} (bar {bar:.1e})")
    assert e1 < bar and e2 < bar and e1r < bar
    with pytest.raises(ValueError):
        NufftPlan(x.cuda(), (0.7, 0.4, 0.1), tol)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_equal_lengthscales_pin_the_isotropic_model():
    """ARD(l, l) on the unit square against the isotropic model: same grid bit for bit, ws to 1e-12, and the predictive mean within
    10 x the change of the ISOTROPIC model's mean when its cg_tol goes from 1e-6 to 1e-8 (two converged solves of one system differ
    by their truncation errors; the ARD weights differ from the isotropic ones in the last bits, which the solve amplifies)."""
    from kernels import SquaredExponential, SquaredExponentialARD
    x, y, xn = _data(400, [1.0, 1.0], 11)
    sig, eps, ell = 0.05, 1e-4, 0.3
    means = {}
    for tag, tol in (("iso", 1e-6), ("iso_tight", 1e-8), ("ard", 1e-6)):
        k = (SquaredExponentialARD if tag == "ard" else SquaredExponential)(dimension=2, init_lengthscale=ell, init_variance=1.0)
        m = _model(k, x, y, sig, eps, cg_tol=tol)
        means[tag] = (_np(m.predict(xn.cuda(), return_variance=False)[0]), m)
    iso, ard = means["iso"][1], means["ard"][1]
    assert ard.last_fit_stats["hs"] == (iso._fit_state["h"],) * 2 and ard.last_fit_stats["shape"] == (iso._fit_state["mtot"],) * 2
    assert ard.last_fit_stats["feature_count"] == iso.last_fit_stats["feature_count"]
    e_ws = _rel(_np(ard._fit_state["ws"].real), _np(iso._fit_state["ws"].real))
    yard = _rel(means["iso"][0], means["iso_tight"][0])
    got = _rel(means["ard"][0], means["iso"][0])
    print(f"\nequal-l pin: block {ard.last_fit_stats['shape']} ws {e_ws:.2e}; isotropic mean moves {yard:.2e} for cg_tol 1e-6 -> 1e-8; "
          f"ARD vs isotropic {got:.2e} (bound {10 * yard:.2e})")
    assert e_ws < 1e-12
    assert got <= 10 * yard


@pytest.mark.parametrize("eps", [1e-4, 1e-6])
def test_anisotropic_fit(eps):
    """SE, l = (0.08, 0.5) on [0, 1] x [0, 0.3], N = 300, 40 new points: (a) mean and 'regular' variance against the dense
    feature-space restatement, (b) mean against the dense exact GP; each within 5 x what the isotropic model (l = 0.3, same N, eps,
    noise) reaches against the same kind of reference (the anisotropic block has another condition number)."""
    from kernels import SquaredExponential, SquaredExponentialARD
    x, y, xn = _data(300, [1.0, 0.3], 1)
    sig = 0.04
    fig = {}
    for tag in ("iso", "ard"):
        k = SquaredExponential(dimension=2, init_lengthscale=0.3, init_variance=1.0) if tag == "iso" else \
            SquaredExponentialARD(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.0)
        m = _model(k, x, y, sig, eps)
        mean, var = m.predict(xn.cuda(), variance_method="regular")
        rm, rv = _restate(m, k, x, y, xn, sig)
        em, _, _ = D.exact_gp(k, x, y, sig, xn)
        fig[tag] = (_rel(_np(mean), rm), _rel(_np(var), rv), _rel(_np(mean), em), _grid_of(m)[1], int(m.last_fit_stats["mean_cg_iters"]))
    for tag, (a, b, c, shape, its) in fig.items():
        print(f"\neps {eps:g} {tag}: block {shape} route {R.route(shape, True)} cg iters {its}; mean vs restatement {a:.2e}, variance vs "
              f"restatement {b:.2e}, mean vs exact GP {c:.2e}")
    print(f"ratios ARD / isotropic: {[round(fig['ard'][q] / fig['iso'][q], 3) for q in range(3)]}")
    assert fig["ard"][3] == ((27, 9) if eps == 1e-4 else (35, 11))
    assert R.route(fig["ard"][3], True)[0] == "generic"                    # one workgroup per system, the generic kernel
    for q in range(3):
        assert fig["ard"][q] <= 5 * fig["iso"][q], q


def _mean_against_restatement(d, box, ard_ells, eps, N, seed, want_shape=None, want_route=None):
    from kernels import SquaredExponential, SquaredExponentialARD
    x, y, xn = _data(N, box, seed)
    sig = 0.04
    out = {}
    for tag in ("iso", "ard"):
        k = SquaredExponential(dimension=d, init_lengthscale=0.3, init_variance=1.0) if tag == "iso" else \
            SquaredExponentialARD(dimension=d, init_lengthscale=ard_ells, init_variance=1.0)
        m = _model(k, x, y, sig, eps)
        mean = m.predict(xn.cuda(), return_variance=False)[0]
        rm, _ = _restate(m, k, x, y, xn, sig, want_var=False)
        out[tag] = (_rel(_np(mean), rm), _grid_of(m)[1], int(m.last_fit_stats["mean_cg_iters"]))
        print(f"\n{d}-D {tag}: block {out[tag][1]} route {R.route(out[tag][1], True)} cg iters {out[tag][2]} mean vs restatement {out[tag][0]:.2e}")
    if want_shape is not None:
        assert out["ard"][1] == want_shape
    if want_route is not None:
        assert R.route(out["ard"][1], True)[0] in want_route
    assert out["ard"][0] <= 5 * out["iso"][0]


def test_fit_on_the_cooperative_grid():
    """l = (0.04, 0.018) on [0, 1] x [0, 0.5] at eps 1e-2: block (37, 41), 2 n - 1 = (73, 81): the cooperative 2-D solver on (96, 96)."""
    _mean_against_restatement(2, [1.0, 0.5], (0.04, 0.018), 1e-2, 300, 21, want_shape=(37, 41), want_route=("coop_herm", "coop"))


def test_fit_3d_non_cubic():
    _mean_against_restatement(3, [1.0, 0.5, 0.4], (0.1, 0.5, 0.3), 1e-3, 200, 22, want_shape=(23, 7, 9))


def test_matern_ard_fit():
    """MaternARD(3/2), l = (0.15, 0.6) on [0, 1] x [0, 0.4], eps 1e-3: block (45, 17); mean and 'regular' variance against the
    restatement within 5 x the isotropic Matern-3/2 (l = 0.3) figures."""
    from kernels import Matern, MaternARD
    x, y, xn = _data(300, [1.0, 0.4], 31)
    sig, eps = 0.04, 1e-3
    fig = {}
    for tag in ("iso", "ard"):
        k = Matern(dimension=2, nu=1.5, init_lengthscale=0.3, init_variance=1.0) if tag == "iso" else \
            MaternARD(dimension=2, nu=1.5, init_lengthscale=(0.15, 0.6), init_variance=1.0)
        m = _model(k, x, y, sig, eps)
        mean, var = m.predict(xn.cuda(), variance_method="regular")
        rm, rv = _restate(m, k, x, y, xn, sig)
        fig[tag] = (_rel(_np(mean), rm), _rel(_np(var), rv), _grid_of(m)[1])
        print(f"\nMatern-3/2 {tag}: block {fig[tag][2]} route {R.route(fig[tag][2], True)} mean {fig[tag][0]:.2e} variance {fig[tag][1]:.2e}")
    assert fig["ard"][2] == (45, 17)
    assert fig["ard"][0] <= 5 * fig["iso"][0] and fig["ard"][1] <= 5 * fig["iso"][1]


def test_stochastic_variance_with_given_probes():
    """The lag-sum estimator with injected probes against the restatement's with the same probes, to the NUFFT tolerance contract of
    tests/test_gpu_nufft_options.py: relative l2 error below 2 x nufft_eps + 1e-13, a real-only output judged on the scale of the
    complex sums it is the real part of (here sum_r c[r] exp(2 pi i sum_a r_a h_a x_a) before its real part is taken).  The solves
    run to 1e-11, far below the transform's tolerance."""
    from kernels import SquaredExponentialARD
    x, y, xn = _data(300, [1.0, 0.3], 1)
    sig, nufft_eps, J = 0.04, 1e-6, 8
    k = SquaredExponentialARD(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.0)
    m = _model(k, x, y, sig, 1e-4, cg_tol=1e-11, nufft_eps=nufft_eps).fit()
    hs, shape = _grid_of(m)
    eta = (torch.randint(0, 2, (J, math.prod(shape)), generator=torch.Generator().manual_seed(8)) * 2 - 1).to(torch.float64)
    _, var = m.predict(xn.cuda(), variance_method="stochastic", hutchinson_probes=J, variance_probes=eta.cuda())
    F, Fn = D.features(x, hs, shape), D.features(xn, hs, shape)
    ws, _ = D.weights(k, hs, shape)
    ref = D.variance_lag_sums(F, Fn, ws, sig, eta, complex_sums=True)
    err = float(np.linalg.norm(_np(var) - ref.real) / np.linalg.norm(ref))
    on_real = float(np.linalg.norm(_np(var) - ref.real) / np.linalg.norm(ref.real))
    bar = 2 * nufft_eps + 1e-13
    print(f"\nstochastic variance, block {shape}: {err:.2e} on the scale of the complex sums (bar {bar:.1e}); {on_real:.2e} on the scale "
          f"of their real parts")
    assert err < bar


def _rel_each(a, b):
    """Every component on its own magnitude: max_i |a_i - b_i| / |b_i| (a wrong small row shows)."""
    a, b = np.asarray(a), np.asarray(b)
    return float((np.abs(a - b) / np.abs(b)).max())


def _gradient(kernel, x, y, sig, eps, Z, V):
    from efgpnd import efgpnd_gradient_batched
    st = {}
    g = efgpnd_gradient_batched(x.cuda(), y.cuda(), torch.tensor(sig, dtype=torch.float64), kernel, eps, Z.shape[0], nufft_eps=1e-9,
                                cg_tol=1e-11, probes_Z=Z.cuda(), probes_V=V.cuda(), stats_out=st)
    return _np(g), st


def _probes(T, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randint(0, 2, (T, N), generator=g) * 2 - 1).to(torch.float64),
            (torch.randint(0, 2, (T, M), generator=g) * 2 - 1).to(torch.float64))


def _iso_grid(k, eps, L):
    from utils.kernels import get_xis
    _, h, mtot = get_xis(k, eps, L, use_integral=True)
    return (h,) * k.dimension, (mtot,) * k.dimension


@pytest.mark.parametrize("d,box,ells,N", [(2, [1.0, 0.3], (0.08, 0.5), 300), (3, [1.0, 0.5, 0.4], (0.1, 0.5, 0.3), 150)])
def test_gradient_with_given_probes(d, box, ells, N):
    """All d + 2 components against the restatement's estimator with the same probes (T = 4).  Bound: 10 x the agreement the
    isotropic kernel (l = 0.3) reaches against the same restatement through the entry-by-entry native tail -- on the scale of the
    largest component, and again with every component judged on its own magnitude."""
    from kernels import SquaredExponential, SquaredExponentialARD
    from utils.kernels import get_xis_nd
    x, y, _ = _data(N, box, 40 + d)
    sig, eps, T = 0.04, 1e-3, 4
    iso = SquaredExponential(dimension=d, init_lengthscale=0.3, init_variance=1.0)
    ard = SquaredExponentialARD(dimension=d, init_lengthscale=ells, init_variance=1.0)
    fig = {}
    for tag, k, (hs, shape) in (("iso", iso, _iso_grid(iso, eps, max(box))), ("ard", ard, get_xis_nd(ard, eps, box))):
        Z, V = _probes(T, N, math.prod(shape), 50 + d)
        g, st = _gradient(k, x, y, sig, eps, Z, V)
        assert st["feature_count"] == math.prod(shape) and tuple(st["shape"]) == tuple(shape)
        ws, dp = D.weights(k, hs, shape)
        ref, _, _ = D.gradient_estimator(D.features(x, hs, shape), y, ws, dp, sig, Z, V, k.get_hypers()[-1])
        assert g.shape == ref.shape == (k.num_hypers,)
        fig[tag] = (_rel(g, ref), _rel_each(g, ref))
        print(f"\n{d}-D gradient {tag}: block {shape} grad {np.round(g, 4)} restatement {np.round(ref, 4)}: {fig[tag][0]:.2e} of the "
              f"largest component, {fig[tag][1]:.2e} per component; differences {g - ref}")
    assert ard.num_hypers == d + 2
    assert fig["ard"][0] <= 10 * fig["iso"][0]
    assert fig["ard"][1] <= 10 * fig["iso"][1]


def test_gradient_with_equal_lengthscales_sums_to_the_isotropic_one():
    from kernels import SquaredExponential, SquaredExponentialARD
    x, y, _ = _data(300, [1.0, 1.0], 61)
    sig, eps, T, ell = 0.04, 1e-3, 4, 0.3
    iso = SquaredExponential(dimension=2, init_lengthscale=ell, init_variance=1.0)
    ard = SquaredExponentialARD(dimension=2, init_lengthscale=ell, init_variance=1.0)
    hs, shape = _iso_grid(iso, eps, 1.0)
    Z, V = _probes(T, 300, math.prod(shape), 62)
    gi, _ = _gradient(iso, x, y, sig, eps, Z, V)
    ga, st = _gradient(ard, x, y, sig, eps, Z, V)
    assert tuple(st["shape"]) == shape and tuple(st["hs"]) == hs
    ws, dp = D.weights(iso, hs, shape)
    ref, _, _ = D.gradient_estimator(D.features(x, hs, shape), y, ws, dp, sig, Z, V, 1.0)
    yard, yard_each = _rel(gi, ref), _rel_each(gi, ref)
    folded = np.array([ga[0] + ga[1], ga[2], ga[3]])
    got, got_each = _rel(folded, gi), _rel_each(folded, gi)
    print(f"\nequal-l gradient: isotropic {np.round(gi, 5)} ARD {np.round(ga, 5)}; folded vs isotropic {got:.2e} (isotropic vs "
          f"restatement {yard:.2e}, bound {10 * yard:.2e}); per component {np.abs(folded - gi) / np.abs(gi)} (isotropic vs restatement "
          f"{yard_each:.2e}, bound {10 * yard_each:.2e})")
    assert got <= 10 * yard
    assert got_each <= 10 * yard_each                # sum_j d/dl_j, the variance entry and the noise entry, each on its own scale


def test_training_separates_the_lengthscales():
    """y from the squared-exponential ARD GP with l = (0.08, 0.5), variance 1, noise 0.05 at 400 points of the unit square; start at
    (0.2, 0.2), variance 1, noise 0.1; 30 Adam steps of 0.1 on the log parameters.  The same loop with the dense exact gradient
    (tests/_ard_dense.py dense_adam_se_ard, run on the CPU) ends at l = (0.0728, 0.5368): l_0 / l_1 = 0.1356.  The threshold is
    halfway in log ratio between 1 and that: sqrt(0.1356) = 0.368."""
    from kernels import SquaredExponentialARD
    g = torch.Generator().manual_seed(7)
    x = torch.rand(400, 2, generator=g, dtype=torch.float64)
    y = torch.as_tensor(D.draw_se_ard(x, (0.08, 0.5), 1.0, 0.05, seed=3))
    k = SquaredExponentialARD(dimension=2, init_lengthscale=(0.2, 0.2), init_variance=1.0)
    from efgpnd import EFGPND
    m = EFGPND(x.cuda(), y.cuda(), k, sigmasq=0.1, eps=1e-3, nufft_eps=1e-6, estimate_params=False)
    torch.manual_seed(0)
    m.optimize_hyperparameters(lr=0.1, max_iters=30, trace_samples=10)
    l0, l1 = m.kernel.lengthscales
    print(f"\ntrained lengthscales ({l0:.4f}, {l1:.4f}), ratio {l0 / l1:.4f} (dense exact gradient: 0.1356; threshold 0.368); "
          f"block {m.last_fit_stats['shape']}")
    assert l0 / l1 < 0.368


def test_prior_draws_have_the_ard_kernel():
    """sample_paths(prior=True) on block (27, 9): 2000 draws at 6 points; means, variances and every covariance within the 5
    standard-error bands tests/test_gpu_sampling.py uses (the quadrature error of the grid, 1e-4, is far inside them)."""
    from kernels import SquaredExponentialARD
    x, y, xn = _data(300, [1.0, 0.3], 1, n_new=6)
    k = SquaredExponentialARD(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.0)
    m = _model(k, x, y, 0.04, 1e-4).fit()
    assert m.last_fit_stats["shape"] == (27, 9)
    ns = 2000
    paths = m.sample_paths(xn.cuda(), ns, seed=2, prior=True).cpu()
    assert paths.shape == (ns, 6)
    K = k.kernel_matrix(xn, xn)
    v = K.diagonal()
    sm, sv = paths.mean(0), paths.var(0, unbiased=True)
    print("\nprior mean / s.e.:", [round(float(t), 2) for t in sm / (v / ns).sqrt()])
    print("prior variance deviation / s.e.:", [round(float(t), 2) for t in (sv / v - 1) / math.sqrt(2 / (ns - 1))])
    assert bool((sm.abs() <= 5 * (v / ns).sqrt()).all())
    assert bool(((sv / v - 1).abs() <= 5 * math.sqrt(2 / (ns - 1))).all())
    dlt = paths - sm
    for i in range(6):
        for j in range(i):
            c = float(K[i, j])
            sc = float((dlt[:, i] * dlt[:, j]).sum() / (ns - 1))
            assert abs(sc - c) <= 5 * math.sqrt((c * c + float(v[i] * v[j])) / ns), (i, j)


def test_posterior_draws_and_log_marginal_run_on_the_per_axis_grid():
    """Posterior draws scatter around the mean with the 'regular' variance (5 standard-error bands, 512 draws), and the log
    determinant of logdet_slq with given probes equals sum_p z_p^T log(I + D T D / sigma^2) z_p / P + n log sigma^2 of the dense
    operator: 60 Lanczos steps integrate log over a spectrum that clusters at 1 far below the 1e-6 asked here."""
    from efgpnd import logdet_slq
    from kernels import SquaredExponentialARD
    x, y, xn = _data(300, [1.0, 0.3], 1, n_new=6)
    sig = 0.04
    k = SquaredExponentialARD(dimension=2, init_lengthscale=(0.08, 0.5), init_variance=1.0)
    m = _model(k, x, y, sig, 1e-4, cg_tol=1e-8).fit()
    mean, var = m.predict(xn.cuda(), variance_method="regular")
    ns = 512
    paths = m.sample_posterior(xn.cuda(), ns, method="efgp", seed=5)              # (B, ns) numpy
    assert paths.shape == (6, ns)
    dm = np.abs(paths.mean(1) - _np(mean))
    assert (dm <= 5 * np.sqrt(_np(var) / ns) + 2e-9 * np.abs(_np(mean)).max()).all()
    assert (np.abs(paths.var(1, ddof=1) / _np(var) - 1) <= 5 * math.sqrt(2 / (ns - 1))).all()
    hs, shape = _grid_of(m)
    P, M = 16, math.prod(shape)
    zs = (torch.randint(0, 2, (P, M), generator=torch.Generator().manual_seed(9)) * 2 - 1).to(torch.float64)
    got = logdet_slq(m._fit_state["ws"], sig, m._toeplitz, probes=P, steps=60, n=300, probe_vectors=zs.cuda())
    F = D.features(x, hs, shape)
    ws, _ = D.weights(k, hs, shape)
    lam, U = np.linalg.eigh(D.operator_mean(F, ws, sig) / sig)
    ref = float(np.mean([(np.abs(U.conj().T @ z) ** 2 * np.log(lam)).sum() for z in zs.numpy()])) + 300 * math.log(sig)
    print(f"\nlog det with given probes: {got:.8f} dense {ref:.8f}")
    assert abs(got - ref) <= 1e-6 * abs(ref)
