"""GPU checks of GP path sampling on the HIP operators: the counter-based normal generator, Gaussian strengths generated inside
the spreaders (efgp_nufft_type1_normal against efgp_normal_fill), the right-hand-side kernel (efgp_hermitian_normal_rows) and
EFGPND.sample_paths against the dense restatement of tests/_sampling.py.

All seeds are fixed.  Statistical bounds are five standard errors of the estimator, derived from its sample count; with fixed
seeds the outcome is deterministic."""
import math

import numpy as np
import pytest
import torch

import _sampling as S

pytestmark = pytest.mark.gpu

BOUND = 8.5717            # sqrt(2 * 53 * ln 2): the generator's bound (csrc/nufft_dev.hpp kNormalBound)
EPS64 = 2.0 ** -52


def _rel(a, b):
    a = a.detach().cpu()
    b = b.detach().cpu()
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


def _points(N, d, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, d, generator=g, dtype=torch.float64) * (hi - lo) + lo


# ------------------------------------------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------------------------------------------
def test_generator_is_a_function_of_its_counter():
    from efgp_hip import normal_fill
    dev = torch.device("cuda", 0)
    n = 1_000_000
    Z = normal_fill(dev, 2024, 4, n)
    assert Z.shape == (4, n) and Z.dtype == torch.float64
    assert torch.equal(Z, normal_fill(dev, 2024, 4, n))                          # repeatable bit for bit
    k = 12345
    Zk = normal_fill(dev, 2024, 4, n - k, index_offset=k)                        # index_offset = k shifts a row by k
    assert torch.equal(Zk, Z[:, k:])
    assert torch.equal(normal_fill(dev, 2024, 3, n), Z[:3])                      # row r does not depend on the row count
    assert torch.equal(normal_fill(dev, 2024, 1, n), Z[:1])
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(Z[a], Z[b])
    Z2 = normal_fill(dev, 2025, 4, n)
    assert not torch.equal(Z, Z2) and float((Z == Z2).double().mean()) < 1e-3
    assert torch.isfinite(Z).all()


def test_generator_moments_and_distribution():
    """4 rows = 2 pairs of 1e6 values, n = 4e6 in total."""
    from efgp_hip import normal_fill
    dev = torch.device("cuda", 0)
    z = normal_fill(dev, 77, 4, 1_000_000).reshape(-1)
    n = z.numel()
    assert n == 4_000_000
    zmax = float(z.abs().max())
    mean = float(z.mean())
    c = z - mean
    var = float((c ** 2).mean())
    skew = float((c ** 3).mean()) / var ** 1.5
    kurt = float((c ** 4).mean()) / var ** 2 - 3.0
    zs, _ = torch.sort(z)
    cdf = 0.5 * (1.0 + torch.erf(zs / math.sqrt(2.0)))
    i = torch.arange(1, n + 1, dtype=torch.float64, device=dev)
    ks = float(torch.maximum((i / n - cdf).max(), (cdf - (i - 1) / n).max()))
    print(f"normal generator: max|z| {zmax:.4f} mean {mean:.3e} var-1 {var - 1:.3e} skew {skew:.3e} kurt {kurt:.3e} "
          f"KS sqrt(n) {ks * math.sqrt(n):.3f}")
    assert zmax <= BOUND
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1) < 5 * math.sqrt(2 / n)
    assert abs(skew) < 5 * math.sqrt(6 / n)
    assert abs(kurt) < 5 * math.sqrt(24 / n)
    assert ks < 2.69 / math.sqrt(n)                                              # Kolmogorov distance, the 1e-6 level


def test_generator_rows_are_uncorrelated():
    """Each correlation is estimated from n = 4e6 products (8 rows of 1e6, so that every estimator has that count): the two rows
    of a pair (4 pairs), neighbouring pairs (row r against the same and against the other element of the next pair), and the
    Rademacher rows of the same seed (against the normals and against their squares)."""
    from efgp_hip import normal_fill, rademacher_fill
    dev = torch.device("cuda", 0)
    seed, m = 4242, 1_000_000
    Z = normal_fill(dev, seed, 8, m)
    Zn = (Z - Z.mean(1, keepdim=True)) / Z.std(1, keepdim=True)
    n = 4 * m

    def corr(a, b):
        return float((a * b).sum()) / n
    r_pair = corr(Zn[0:8:2], Zn[1:8:2])                                          # rows 2p and 2p + 1, p = 0..3
    r_next_same = corr(Zn[0:4], Zn[2:6])                                         # row r and row r + 2: same element of the next pair
    r_next_cross = corr(Zn[[0, 1, 2, 3]], Zn[[3, 2, 5, 4]])                      # the other element of the next pair
    R = rademacher_fill(dev, seed, 4, m)
    r_rad = corr(Zn[0:4], R)
    r_rad_sq = corr(Zn[0:4] ** 2 - 1.0, R) / math.sqrt(2.0)                      # the radius shares no bits with the signs either
    print(f"normal generator correlations x sqrt(n): pair {r_pair * math.sqrt(n):.3f} next {r_next_same * math.sqrt(n):.3f} "
          f"{r_next_cross * math.sqrt(n):.3f} rademacher {r_rad * math.sqrt(n):.3f} {r_rad_sq * math.sqrt(n):.3f}")
    for r in (r_pair, r_next_same, r_next_cross, r_rad, r_rad_sq):
        assert abs(r) < 5 / math.sqrt(n)


# ------------------------------------------------------------------------------------------------------------------------------
# fused transform
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-5, 1e-7])
@pytest.mark.parametrize("layout", [True, False])
@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_type1_normal_2d(T, layout, tol):
    """Generated normal rows through the MFMA spreader of a layout plan and the LDS spreader of a plain plan: against the
    materialised rows through a plain plan (4 tol), against the exact sums (2 tol), repeatable, with an index offset, and row r
    independent of the row count."""
    from efgp_hip import NufftPlan, PointSet, normal_fill
    from oracle import efgp_oracle as O
    N, h, nm = 50000, 0.31, 23
    x = _points(N, 2, 31 + T)
    xd = x.cuda()
    plan = NufftPlan(xd, h, tol, points=PointSet(xd)) if layout else NufftPlan(xd, h, tol)
    plain = NufftPlan(xd, h, tol)
    seed, off = 990 + T, 7
    FZ = plan.type1_normal(seed, T, (nm, nm), index_offset=off)
    Z = normal_fill(xd.device, seed, T, N, index_offset=off)
    assert _rel(FZ, plain.type1(Z, (nm, nm)).reshape(T, nm, nm)) < 4 * tol
    Zc = Z.cpu()
    for b in range(T):
        assert _rel(FZ[b], O.nudft_type1(x, h, Zc[b], (nm, nm))) < 2 * tol
    assert torch.equal(FZ, plan.type1_normal(seed, T, (nm, nm), index_offset=off))
    F0 = plan.type1_normal(seed, T, (nm, nm))                                    # offset 0: other draws
    assert _rel(F0, plain.type1(normal_fill(xd.device, seed, T, N), (nm, nm)).reshape(T, nm, nm)) < 4 * tol
    assert _rel(F0, FZ) > 0.1
    F1 = plan.type1_normal(seed, T + 1, (nm, nm), index_offset=off)
    for b in range(T):
        assert _rel(F1[b], FZ[b]) < 4 * tol
    if T >= 2:                                   # 2-D: every row of both calls rides in a pair grid (an odd count pads its last pair)
        assert torch.equal(F1[:T], FZ)


@pytest.mark.parametrize("d,N,h,nm,T,tol", [
    (1, 30000, 0.2, 41, 3, 1e-7),                # 1-D, LDS spreader: one pair pass and a single-row pass
    (3, 20000, 0.3, 9, 3, 1e-5),                 # 3-D, fine grid in LDS
    (3, 40000, 0.12, 21, 4, 1e-5),               # 3-D, fine grid beyond LDS: tile-sorted spreader
    (3, 6000, 0.12, 21, 3, 1e-5),                # 3-D, beyond LDS with few points: global fixed-point atomics
    (2, 50000, 0.12, 71, 5, 1e-7),               # 2-D plain plan, fine grid beyond LDS
])
def test_type1_normal_other_spread_paths(d, N, h, nm, T, tol):
    from efgp_hip import NufftPlan, normal_fill
    from oracle import efgp_oracle as O
    x = _points(N, d, 5 + d)
    xd = x.cuda()
    plan = NufftPlan(xd, h, tol)
    shape = (nm,) * d
    seed, off = 31337, 11
    FZ = plan.type1_normal(seed, T, shape, index_offset=off)
    Z = normal_fill(xd.device, seed, T, N, index_offset=off)
    assert _rel(FZ, plan.type1(Z, shape).reshape(FZ.shape)) < 4 * tol
    Zc = Z.cpu()
    for b in range(T):
        assert _rel(FZ[b], O.nudft_type1(x, h, Zc[b], shape)) < 2 * tol
    assert torch.equal(FZ, plan.type1_normal(seed, T, shape, index_offset=off))
    F1 = plan.type1_normal(seed, T + 1, shape, index_offset=off)
    for b in range(T):
        assert _rel(F1[b], FZ[b]) < 4 * tol


def test_type1_normal_rows_numbered_across_calls_and_empty_plan():
    """normal_row_offset continues the row numbering in a second call; a plan without points returns zeros; bad counts raise."""
    from efgp_hip import NufftPlan, PointSet, normal_fill, normal_row_offset
    N, h, nm, tol = 40000, 0.31, 23, 1e-7
    xd = _points(N, 2, 77).cuda()
    plan = NufftPlan(xd, h, tol, points=PointSet(xd))
    full = plan.type1_normal(5, 6, (nm, nm))
    tail = plan.type1_normal(5, 2, (nm, nm), index_offset=normal_row_offset(4))
    assert torch.equal(tail, full[4:6])
    assert torch.equal(normal_fill(xd.device, 5, 2, N, index_offset=normal_row_offset(4)), normal_fill(xd.device, 5, 6, N)[4:6])
    empty = NufftPlan(torch.zeros(0, 2, dtype=torch.float64, device="cuda"), h, tol)
    out = empty.type1_normal(5, 3, (nm, nm))
    assert out.shape == (3, nm, nm) and float(out.abs().max()) == 0.0
    with pytest.raises(ValueError):
        plan.type1_normal(5, 0, (nm, nm))


# ------------------------------------------------------------------------------------------------------------------------------
# right-hand sides on the mode grid
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(41,), (23, 23), (9, 9, 9)])
def test_hermitian_normal_rows(shape):
    from efgp_hip import hermitian_normal_rows, normal_fill, normal_row_offset
    dev = torch.device("cuda", 0)
    M = int(np.prod(shape))
    nrows, seed, a, b = 5, 808, 0.37, 0.21
    fill = normal_fill(dev, seed, 2 * nrows, M)
    g = torch.Generator().manual_seed(1)
    fz = S.conj_even_normal(nrows, M, g).to(dev) * 40.0
    k = S.mode_grid(shape[0], len(shape)).to(dev)
    ws = torch.exp(-0.05 * (k ** 2).sum(1)).to(torch.complex128)                 # real and even
    out = hermitian_normal_rows(dev, seed, nrows, M, a=a, ws=ws, fz=fz, b=b)
    ref = S.hermitian_rows(fill, a=a, ws=ws, fz=fz, b=b)
    assert out.shape == (nrows, M) and out.dtype == torch.complex128
    for s in range(nrows):
        assert float((out[s] - ref[s]).abs().max()) <= 64 * EPS64 * float(ref[s].abs().max())
    assert torch.equal(out.flip(1).conj(), out)                                  # conjugate-even bit for bit
    c = (M - 1) // 2
    assert torch.equal(out[:, c].imag, torch.zeros(nrows, dtype=torch.float64, device=dev))
    e = hermitian_normal_rows(dev, seed, nrows, M, a=0.0, b=b)                   # null ws / fz: b * e
    ref_e = S.hermitian_rows(fill, b=b)
    for s in range(nrows):
        assert float((e[s] - ref_e[s]).abs().max()) <= 64 * EPS64 * float(ref_e[s].abs().max())
    assert torch.equal(e.flip(1).conj(), e)
    assert torch.equal(e[:, c].real, b * fill[0::2, c])                          # the centre is p[centre], real
    # rows are numbered through the offset: rows 2.. of this call are the rows of a call that starts at pair 2
    assert torch.equal(hermitian_normal_rows(dev, seed, 3, M, a=0.0, b=b, index_offset=normal_row_offset(4)), e[2:])
    with pytest.raises(ValueError):
        hermitian_normal_rows(dev, seed, nrows, M, a=a, ws=ws, fz=None, b=b)
    with pytest.raises(ValueError):
        hermitian_normal_rows(dev, seed, 2, 10, a=0.0, b=1.0)                    # an even mode count has no centre


# ------------------------------------------------------------------------------------------------------------------------------
# model, small and exact
# ------------------------------------------------------------------------------------------------------------------------------
CG_TOL, NUFFT_EPS, NS = 1e-8, 1e-7, 5


def _small_model(case):
    from efgpnd import EFGPND
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    if case == "se1d":
        d, N, kern, eps, sig = 1, 500, SquaredExponential(dimension=1, init_lengthscale=0.2, init_variance=1.3), 1e-4, 0.15
    elif case == "se2d":
        d, N, kern, eps, sig = 2, 1000, SquaredExponential(dimension=2, init_lengthscale=0.3, init_variance=1.5), 1e-3, 0.1
    else:
        d, N, kern, eps, sig = 3, 500, Matern(dimension=3, nu=1.5, init_lengthscale=0.5, init_variance=1.3), 1e-2, 0.2
    g = torch.Generator().manual_seed(17 + d)
    x = torch.rand(N, d, generator=g, dtype=torch.float64) * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(2 * x[:, -1]) + math.sqrt(sig) * torch.randn(N, generator=g, dtype=torch.float64)
    xn = torch.rand(40, d, generator=g, dtype=torch.float64) * 2 - 1
    m = EFGPND(x.cuda(), y.cuda(), kern, sigmasq=sig, eps=eps, nufft_eps=NUFFT_EPS, estimate_params=False,
               opts={"cg_tolerance": CG_TOL})
    return m, x.cuda(), xn.cuda()


@pytest.mark.parametrize("case", ["se1d", "se2d", "matern3d"])
def test_sample_paths_state_is_exact(case):
    from efgp_hip import normal_fill
    from efgpnd import _derive_seed, create_A_mean
    m, x, xn = _small_model(case)
    m.fit()
    st0, stats0 = m._fit_state, m.last_fit_stats
    seed = 20240607
    paths, state = m.sample_paths(xn, NS, seed=seed, return_state=True)
    assert m._fit_state is st0 and m.last_fit_stats == stats0                    # no refit
    st = m._fit_state
    N, M, sig, ws, dev = x.shape[0], st["ws"].numel(), st["sig"], st["ws"].reshape(-1), x.device
    assert paths.shape == (NS, xn.shape[0]) and paths.dtype == torch.float64 and paths.device == x.device
    assert state["seed"] == seed and state["weights"].shape == (NS, M) and len(state["cg_iters"]) == NS
    assert torch.isfinite(paths).all()
    # rhs = sigma D F* e1 + sigma^2 e2 from the materialised noise and the explicit feature matrix
    F = S.feature_matrix(x, st["h"], st["mtot"])
    e1 = normal_fill(dev, _derive_seed(seed, 1), NS, N)
    e2 = S.hermitian_rows(normal_fill(dev, _derive_seed(seed, 2), 2 * NS, M))
    rhs = S.sampler_rhs(F, ws, sig, e1, e2)
    A = create_A_mean(st["ws"], m._toeplitz, sig, torch.complex128)
    Fn = S.feature_matrix(xn, st["h"], st["mtot"])
    exact = S.paths_from_weights(Fn, ws, state["weights"])
    for s in range(NS):
        r_rhs = _rel(state["rhs"][s], rhs[s])
        r_res = _rel(A(state["delta"][s].reshape(st["beta"].shape)).reshape(-1), state["rhs"][s])
        r_path = _rel(paths[s], exact[s])
        print(f"{case} row {s}: rhs {r_rhs:.2e} residual {r_res:.2e} paths {r_path:.2e} iters {state['cg_iters'][s]}")
        assert r_rhs < 2 * NUFFT_EPS
        assert r_res < 1.05 * CG_TOL
        assert r_path < 2 * NUFFT_EPS
        assert 0 < state["cg_iters"][s] < m.opts.get("max_cg_iterations", 1000)
    assert torch.equal(state["weights"], state["delta"] + st["beta"].reshape(1, M))
    assert torch.equal(state["delta"].flip(1).conj(), state["delta"])
    assert m.last_sample_stats["seed"] == seed and m.last_sample_stats["cg_iters"] == state["cg_iters"]
    # against the dense solve of the same system: a relative error of the right-hand side (2 nufft_eps) and of the residual
    # (1.05 cg_tolerance) moves the solution by at most cond(A) times their sum
    _, w_dense = S.dense_paths(F, Fn, ws, sig, st["beta"].reshape(-1), e1, e2)
    cond = float(torch.linalg.cond(S.operator_A(F, ws, sig)))
    for s in range(NS):
        assert _rel(state["delta"][s], w_dense[s] - st["beta"].reshape(-1)) < cond * (2 * NUFFT_EPS + 1.05 * CG_TOL)


@pytest.mark.parametrize("case", ["se1d", "se2d", "matern3d"])
def test_sample_paths_seeding(case):
    m, x, xn = _small_model(case)
    a = m.sample_paths(xn, NS, seed=11)
    st0, stats0 = m._fit_state, m.last_fit_stats
    assert torch.equal(a, m.sample_paths(xn, NS, seed=11))
    assert m._fit_state is st0 and m.last_fit_stats == stats0
    assert not torch.equal(a, m.sample_paths(xn, NS, seed=12))
    torch.manual_seed(7)
    b = m.sample_paths(xn, NS)
    seed_b = m.last_sample_stats["seed"]
    torch.manual_seed(7)
    assert torch.equal(b, m.sample_paths(xn, NS))
    assert m.last_sample_stats["seed"] == seed_b and 0 <= seed_b < 2 ** 63
    assert not torch.equal(b, m.sample_paths(xn, NS))                            # the default generator moved on
    a3 = m.sample_paths(xn, 3, seed=11)
    for s in range(3):
        assert _rel(a3[s], a[s]) < 4 * NUFFT_EPS + 2 * CG_TOL
    p = m.sample_paths(xn, NS, seed=11, prior=True)
    assert p.shape == a.shape and torch.equal(p, m.sample_paths(xn, NS, seed=11, prior=True)) and not torch.equal(p, a)
    p3, ps = m.sample_paths(xn, 3, seed=11, prior=True, return_state=True)
    for s in range(3):
        assert _rel(p3[s], p[s]) < 4 * NUFFT_EPS
    assert ps["delta"] is None and ps["rhs"] is None and ps["cg_iters"] is None and ps["weights"].shape[0] == 3


def test_sample_paths_blocks_continue_the_row_numbering(monkeypatch):
    """Rows are numbered across blocks: a call cut into blocks of 4 rows draws what the single-block call draws."""
    import efgpnd
    m, x, xn = _small_model("se2d")
    a, sa = m.sample_paths(xn, 11, seed=3, return_state=True)
    p = m.sample_paths(xn, 11, seed=3, prior=True)
    monkeypatch.setitem(efgpnd._SAMPLE_BLOCK, 2, 4)
    b, sb = m.sample_paths(xn, 11, seed=3, return_state=True)
    assert m.last_sample_stats["blocks"] == 3
    for s in range(11):
        assert _rel(sb["rhs"][s], sa["rhs"][s]) < 4 * NUFFT_EPS
        assert _rel(b[s], a[s]) < 4 * NUFFT_EPS + 2 * CG_TOL
    assert torch.equal(m.sample_paths(xn, 11, seed=3, prior=True), p)


def test_sample_paths_follows_refits():
    """The plan over the training points depends on the grid spacing h: after the lengthscale changes twice, with a predict (a
    refit) in between, the next draw's right-hand sides are those of the NEW grid, checked against its explicit feature matrix."""
    from efgp_hip import normal_fill
    from efgpnd import _derive_seed
    m, x, xn = _small_model("se2d")
    m.sample_paths(xn, NS, seed=1)
    h0 = m._fit_state["h"]
    seen = {h0}
    for scale in (0.6, 0.7):
        m.kernel.set_hyper("lengthscale", scale * m.kernel.get_hyper("lengthscale"))
        m.predict(xn, return_variance=False)                                     # refit: a new _fit_state, a new h
        seen.add(m._fit_state["h"])
    assert len(seen) == 3
    m.kernel.set_hyper("lengthscale", 0.8 * m.kernel.get_hyper("lengthscale"))
    seed = 77
    paths, state = m.sample_paths(xn, NS, seed=seed, return_state=True)         # refits itself
    st = m._fit_state
    assert st["h"] not in seen
    N, M, ws = x.shape[0], st["ws"].numel(), st["ws"].reshape(-1)
    F = S.feature_matrix(x, st["h"], st["mtot"])
    e1 = normal_fill(x.device, _derive_seed(seed, 1), NS, N)
    e2 = S.hermitian_rows(normal_fill(x.device, _derive_seed(seed, 2), 2 * NS, M))
    rhs = S.sampler_rhs(F, ws, st["sig"], e1, e2)
    exact = S.paths_from_weights(S.feature_matrix(xn, st["h"], st["mtot"]), ws, state["weights"])
    for s in range(NS):
        assert _rel(state["rhs"][s], rhs[s]) < 2 * NUFFT_EPS
        assert _rel(paths[s], exact[s]) < 2 * NUFFT_EPS
    # and back on a grid spacing seen before, with the layout the model holds by now
    m.kernel.set_hyper("lengthscale", 0.3)
    paths0, state0 = m.sample_paths(xn, NS, seed=seed, return_state=True)
    st = m._fit_state
    F = S.feature_matrix(x, st["h"], st["mtot"])
    M, ws = st["ws"].numel(), st["ws"].reshape(-1)
    e2 = S.hermitian_rows(normal_fill(x.device, _derive_seed(seed, 2), 2 * NS, M))
    rhs = S.sampler_rhs(F, ws, st["sig"], e1, e2)
    for s in range(NS):
        assert _rel(state0["rhs"][s], rhs[s]) < 2 * NUFFT_EPS


def test_capped_solves_are_reported():
    """Rows that reach max_cg_iterations are listed in last_sample_stats and in the state, and return_state=True warns."""
    import warnings
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential
    m0, x, xn = _small_model("se2d")
    y = m0._device_data()["y"]
    kern = SquaredExponential(dimension=2, init_lengthscale=0.3, init_variance=1.5)
    m = EFGPND(x, y, kern, sigmasq=0.1, eps=1e-3, nufft_eps=NUFFT_EPS, estimate_params=False,
               opts={"cg_tolerance": CG_TOL, "max_cg_iterations": 50})          # these systems take 223-248 iterations
    m.sample_paths(xn, NS, seed=20240607)
    stats = m.last_sample_stats
    assert stats["cg_max_iterations"] == 50 and stats["cg_capped"] == list(range(NS)) and all(v >= 50 for v in stats["cg_iters"])
    with pytest.warns(RuntimeWarning, match="max_cg_iterations"):
        _, state = m.sample_paths(xn, NS, seed=20240607, return_state=True)
    assert state["cg_capped"] == list(range(NS)) and state["cg_max_iterations"] == 50
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, ok = m0.sample_paths(xn, NS, seed=20240607, return_state=True)       # default cap 1000: nothing capped, no warning
    assert ok["cg_capped"] == [] and ok["cg_max_iterations"] == 1000
    assert m0.last_sample_stats["cg_capped"] == []
    _, pr = m0.sample_paths(xn, NS, seed=1, prior=True, return_state=True)
    assert pr["cg_capped"] is None and "cg_capped" not in m0.last_sample_stats


def test_normal_fill_many_rows():
    """More pairs than one launch's gridDim.y holds: the rows continue across the launches."""
    from efgp_hip import normal_fill, normal_row_offset
    dev = torch.device("cuda", 0)
    nrows, n = 2 * 65535 + 5, 7
    Z = normal_fill(dev, 3, nrows, n)
    assert Z.shape == (nrows, n) and torch.isfinite(Z).all()
    assert torch.equal(Z[:6], normal_fill(dev, 3, 6, n))
    first = 2 * 65535 - 2
    assert torch.equal(Z[first:], normal_fill(dev, 3, nrows - first, n, index_offset=normal_row_offset(first)))


def test_sample_posterior_methods():
    """method="dense" (the default) returns what the dense sampler returned before the method argument existed, for the same
    torch seed; method="efgp" returns the same convention from sample_paths."""
    m, x, xn = _small_model("se1d")
    ns = 4
    torch.manual_seed(5)
    got = m.sample_posterior(xn, ns)
    # the dense sampler restated: dense kernel matrices, a Cholesky factor, one randn on the data's device
    k = m.kernel.kernel
    sig = m.sigmasq.detach()
    K_no = k(torch.cdist(xn, x, p=2))
    K_oo = k(torch.cdist(x, x, p=2)) + sig * torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    K_nn = k(torch.cdist(xn, xn, p=2))
    cov = K_nn - K_no @ torch.linalg.solve(K_oo, K_no.T)
    cov = cov + 1e-10 * torch.eye(xn.shape[0], dtype=xn.dtype, device=xn.device)
    chol = torch.linalg.cholesky(cov)
    torch.manual_seed(5)
    Zs = torch.randn(xn.shape[0], ns, dtype=x.dtype, device=x.device)
    mean, _ = m.predict(xn, return_variance=False)
    want = (mean.unsqueeze(1) + chol @ Zs).detach().cpu().numpy()
    assert isinstance(got, np.ndarray) and got.shape == (xn.shape[0], ns)
    assert np.array_equal(got, want)
    torch.manual_seed(5)
    assert np.array_equal(m.sample_posterior(xn, ns, method="dense"), want)
    e = m.sample_posterior(xn, ns, method="efgp", seed=9)
    assert isinstance(e, np.ndarray) and e.shape == (xn.shape[0], ns) and e.dtype == np.float64
    assert np.array_equal(e, m.sample_paths(xn, ns, seed=9).T.cpu().numpy())


def test_sample_paths_refusals():
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential
    m, x, xn = _small_model("se2d")
    with pytest.raises(ValueError, match="nsamples"):
        m.sample_paths(xn, 0)
    with pytest.raises(ValueError, match="columns"):
        m.sample_paths(xn[:, :1].contiguous(), 2)
    with pytest.raises(ValueError, match="method"):
        m.sample_posterior(xn, 2, method="other")
    ms = EFGPND(x, torch.zeros(x.shape[0], dtype=torch.float64, device=x.device), SquaredExponential(dimension=2), sigmasq=0.1,
                estimate_params=False, opts={"shard_points": True})
    with pytest.raises(NotImplementedError, match="shard_points"):
        ms.sample_paths(xn, 2)


# ------------------------------------------------------------------------------------------------------------------------------
# model, statistical
# ------------------------------------------------------------------------------------------------------------------------------
def _stat_model():
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential
    g = torch.Generator().manual_seed(101)
    N, ell = 2000, 0.3
    x = torch.rand(N, 2, generator=g, dtype=torch.float64) * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, 1]) + 0.5 * torch.randn(N, generator=g, dtype=torch.float64)
    xn = torch.rand(16, 2, generator=g, dtype=torch.float64) * 2.4 - 1.2           # some of them outside the data's box
    xn[1] = xn[0] + torch.tensor([0.12, -0.05], dtype=torch.float64)             # two pairs closer than one lengthscale
    xn[3] = xn[2] + torch.tensor([-0.08, 0.1], dtype=torch.float64)
    kern = SquaredExponential(dimension=2, init_lengthscale=ell, init_variance=1.0)
    m = EFGPND(x.cuda(), y.cuda(), kern, sigmasq=0.25, eps=1e-3, nufft_eps=NUFFT_EPS, estimate_params=False,
               opts={"cg_tolerance": 1e-6})
    return m, x.cuda(), xn.cuda()


def test_posterior_draws_have_the_posterior_moments():
    m, x, xn = _stat_model()
    ns = 2048
    mean, v = m.predict(xn, variance_method="regular")
    paths = m.sample_paths(xn, ns, seed=1)
    assert m.last_sample_stats["blocks"] == ns // 64
    st = m._fit_state
    ws = st["ws"].reshape(-1)
    C = S.weight_space_cov(S.feature_matrix(x, st["h"], st["mtot"]), S.feature_matrix(xn, st["h"], st["mtot"]), ws, st["sig"])
    assert float((C.diagonal() - v).abs().max()) < 1e-3 * float(v.max())         # the 'regular' variance is this diagonal
    sm, sv = paths.mean(0), paths.var(0, unbiased=True)
    dm = (sm - mean).abs()
    print("posterior mean deviation / s.e.:", [round(float(t), 2) for t in dm / (v / ns).sqrt()])
    print("posterior variance deviation / s.e.:", [round(float(t), 2) for t in (sv / v - 1) / math.sqrt(2 / (ns - 1))])
    assert bool((dm <= 5 * (v / ns).sqrt() + 2 * NUFFT_EPS * mean.abs().max()).all())
    assert bool(((sv / v - 1).abs() <= 5 * math.sqrt(2 / (ns - 1))).all())
    d = paths - sm
    for i, j in ((0, 1), (2, 3)):
        assert float((xn[i] - xn[j]).norm()) < 0.3
        c = float(C[i, j])
        sc = float((d[:, i] * d[:, j]).sum() / (ns - 1))
        se = math.sqrt((c * c + float(v[i] * v[j])) / ns)
        print(f"pair ({i},{j}): correlation {c / math.sqrt(float(v[i] * v[j])):.3f} deviation {abs(sc - c) / se:.2f} s.e.")
        assert abs(sc - c) <= 5 * se


def test_prior_draws_have_the_feature_kernel():
    m, x, xn = _stat_model()
    ns = 4096
    paths = m.sample_paths(xn, ns, seed=2, prior=True)
    st = m._fit_state
    K = S.prior_cov(S.feature_matrix(xn, st["h"], st["mtot"]), st["ws"].reshape(-1))
    v = K.diagonal()
    sm, sv = paths.mean(0), paths.var(0, unbiased=True)
    print("prior mean / s.e.:", [round(float(t), 2) for t in sm / (v / ns).sqrt()])
    print("prior variance deviation / s.e.:", [round(float(t), 2) for t in (sv / v - 1) / math.sqrt(2 / (ns - 1))])
    assert bool((sm.abs() <= 5 * (v / ns).sqrt()).all())
    assert bool(((sv / v - 1).abs() <= 5 * math.sqrt(2 / (ns - 1))).all())
    d = paths - sm
    for i, j in ((0, 1), (2, 3)):
        c = float(K[i, j])
        sc = float((d[:, i] * d[:, j]).sum() / (ns - 1))
        assert abs(sc - c) <= 5 * math.sqrt((c * c + float(v[i] * v[j])) / ns)


# ------------------------------------------------------------------------------------------------------------------------------
# full size
# ------------------------------------------------------------------------------------------------------------------------------
def test_sample_paths_at_full_size():
    """N = 1e6, BASELINE configs[1] (2-D SE, l = 0.2, eps = 1e-4: 23 x 23 modes, CG tolerance 1e-4), layout on, 8 draws.

    max_cg_iterations: the noise right-hand sides excite every mode, so their solves are bounded by CG's worst case
    sqrt(cond) ln(2 / tol) / 2 with cond = (N max ws^2 + sigma^2) / sigma^2 = 3.0e5 here: 2712 iterations (measured: 785-1055).
    The default cap of 1000 lies below that bound, so the model is given 3000."""
    from efgpnd import EFGPND, create_A_mean
    from kernels.squared_exponential import SquaredExponential
    N, tol, nufft_tol, mtot = 1_000_000, 1e-4, 1e-7, 23
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(N, 2, generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, 1]) + 0.2 * torch.randn(N, generator=g, dtype=torch.float64, device="cuda")
    k = SquaredExponential(dimension=2, init_lengthscale=0.2, init_variance=2.0)
    m = EFGPND(x, y, k, sigmasq=0.2, eps=1e-4, nufft_eps=nufft_tol, estimate_params=False,
               opts={"cg_tolerance": tol, "mean_cg_warm_start": False, "point_layout": True, "max_cg_iterations": 3000})
    idx = torch.randint(0, N, (128,), generator=torch.Generator().manual_seed(5)).cuda()
    xn = x[idx].contiguous()
    paths, state = m.sample_paths(xn, 8, seed=99, return_state=True)
    st = m._fit_state
    assert st["mtot"] == mtot and m._devdata["points"] is not None
    assert paths.shape == (8, 128) and torch.isfinite(paths).all()
    cond = float(N * (st["ws"].abs() ** 2).max() / st["sig"] + 1.0)
    assert 0.5 * math.sqrt(cond) * math.log(2 / tol) < m.opts["max_cg_iterations"]
    print("full size: cond", cond, "cg_iters", state["cg_iters"])
    assert all(0 < it < m.opts["max_cg_iterations"] for it in state["cg_iters"])
    assert torch.equal(state["delta"].flip(1).conj(), state["delta"])          # Fourier coefficients of real functions
    A = create_A_mean(st["ws"], m._toeplitz, st["sig"], torch.complex128)
    exact = S.paths_from_weights(S.feature_matrix(xn, st["h"], mtot), st["ws"].reshape(-1), state["weights"])
    for s in range(8):
        r_res = _rel(A(state["delta"][s].reshape(st["beta"].shape)).reshape(-1), state["rhs"][s])
        r_path = float((paths[s] - exact[s]).abs().max() / paths[s].abs().max())
        print(f"full size row {s}: residual {r_res:.2e} paths {r_path:.2e}")
        assert r_res < 1.05 * tol
        assert r_path < 5 * nufft_tol
    # the draws scatter around the mean with the posterior's scale (tiny at a million observations) and not beyond six of its
    # standard deviations (1024 values: beyond six has probability 2e-6)
    mean, v = m.predict(xn, variance_method="regular")
    dev = (paths - mean).abs() / v.sqrt()
    print("full size: largest deviation in posterior s.d.", float(dev.max()), "posterior s.d. up to", float(v.max().sqrt()))
    assert 0 < float(dev.max()) < 6
