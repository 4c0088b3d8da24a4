"""Polya-Gamma negative-binomial GP regressor on the MI355X: seeded fits against the reference's own regressor
(tests/golden/pgnb_*.npz, made by tools/gen_golden_pgnb.py with the exact-NUDFT stand-in), reproducibility, the two new
kernels and the device digamma against torch restatements (tests/_pgnb.py), an unseeded device-probe fit and one learnt-r fit
at N = 1e6."""
import glob
import json
import os
import time

import numpy as np
import pytest
import torch

from _pgnb import gauss_hermite, nb_estep_restated, total_count_grad_terms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pgnb_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in GOLDEN]

# Tolerances against the reference: the goldens are exact NUDFTs, the fits run at nufft_eps = 1e-7 and cg_tol = 1e-6.
REL = 1e-5
# CG counts: within 2 of the reference's.  NB systems (delta ~ (y + r) / 4) take 15..53 iterations against the classifier's
# 10..16, and near cg_tol their residual falls slowly enough that the 1e-7 perturbation of the NUFFT moves the stopping
# iteration by 2 now and then (measured on the MI355X: the final E-step of pgnb_se2d_fixed_n1000, 38 against 40, one M-step
# count of pgnb_se1d_learn_n500) while every fitted value stays within 1e-6 of the reference.
CG_SLACK = 2
R_VALUES = (0.05, 1.0, 37.5)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _dtype(name):
    return {"torch.float32": torch.float32, "torch.float64": torch.float64}[name]


def fit_golden(g, **over):
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    params = json.loads(str(g["params"]))
    params.update(device="cuda", store_history=True)
    params.update(over)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(_dtype(str(g["torch_default_dtype"])))      # the dtype the reference's hyper-parameters lived in
    try:
        return PolyagammaGPNegativeBinomialRegressor(**params).fit(g["X"], g["y"])
    finally:
        torch.set_default_dtype(prev)


_FITS = {}


def seeded(path):
    if path not in _FITS:
        g = np.load(path)
        _FITS[path] = (g, fit_golden(g))
    return _FITS[path]


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_seeded_fit_matches_reference(path):
    g, reg = seeded(path)
    hist = {k: np.array([r[k] for r in reg.history_]) for k in reg.history_[0]}
    assert list(reg.history_[0].keys()) == list(g["history_keys"])
    assert all(list(r.keys()) == list(g["history_keys"]) for r in reg.history_)
    dev = {k: rel(hist[k], g["history_" + k]) for k in ("lengthscale", "variance", "grad_lengthscale", "grad_variance",
                                                         "total_count", "grad_total_count", "mean_count_mae")}
    for attr in ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        dev[attr] = rel(getattr(reg, attr), g[attr])
    for attr in ("training_mean_absolute_error_", "total_count_", "lengthscale_", "variance_"):
        dev[attr] = rel(getattr(reg, attr), g[attr])
    Xt = g["X_test"]
    dev["decision_function"] = rel(reg.decision_function(Xt), g["decision_function"])
    dev["predictive_variance"] = rel(reg.predictive_variance(Xt), g["predictive_variance"])
    dev["predict"] = rel(reg.predict(Xt), g["predict"])
    de = np.abs(hist["e_cg_iters"] - g["history_e_cg_iters"]).max()
    dm = np.abs(hist["m_cg_iters"] - g["history_m_cg_iters"]).max()
    print(f"\n{os.path.basename(path)}: " + " ".join(f"{k}={v:.1e}" for k, v in dev.items()) +
          f" d_e_cg={de} d_m_cg={dm} r={reg.total_count_:.6f} ref={float(g['total_count_']):.6f} "
          f"mae={reg.training_mean_absolute_error_:.6f} cg_e={hist['e_cg_iters'].astype(int).tolist()} "
          f"ref {g['history_e_cg_iters'].astype(int).tolist()} cg_m={hist['m_cg_iters'].astype(int).tolist()} "
          f"ref {g['history_m_cg_iters'].astype(int).tolist()}")
    assert len(reg.history_) == len(g["history_iter"])
    for k, v in dev.items():
        assert v <= REL, (k, v)
    assert de <= CG_SLACK and dm <= CG_SLACK
    np.testing.assert_array_equal(hist["total_count_updated"], g["history_total_count_updated"])
    assert reg.training_metric_ == reg.training_mean_absolute_error_ and reg.shape_parameter_ == reg.total_count_
    # mean count on the training inputs = r exp(mean + var / 2) of the posterior marginals
    from polyagamma_classification import negative_binomial_gaussian_mean
    expect = negative_binomial_gaussian_mean(torch.from_numpy(reg.posterior_mean_), torch.from_numpy(reg.posterior_var_diag_),
                                             total_count=reg.total_count_).numpy()
    assert np.array_equal(reg.predict(g["X"]), expect)
    solves = reg.last_fit_stats["solves"]
    assert len(solves) == 2 * int(json.loads(str(g["params"]))["max_iter"]) + 2
    assert all(s["fused"] and s["entry"] == "efgp_cg_solve" for s in solves)


def test_seeded_learnt_fits_are_bit_identical():
    g, a = seeded(GOLDEN[IDS.index("pgnb_se1d_learn_n500")])
    b = fit_golden(g)
    for attr in ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        assert np.array_equal(getattr(a, attr), getattr(b, attr)), attr
    assert a.history_ == b.history_ and a.total_count_ == b.total_count_
    assert np.array_equal(a.predict(g["X_test"]), b.predict(g["X_test"]))


@pytest.mark.parametrize("form", ["probe_pointer", "device_hash"])
def test_nb_estep_update_kernel_against_torch(form):
    from efgp_hip.ops import pg_nb_estep_update, rademacher_fill
    dev = torch.device("cuda", 0)
    N, J, seed = 10 ** 6, 10, 4242
    g = torch.Generator(device=dev).manual_seed(3)
    S = torch.randn((J + 1, N), dtype=torch.float64, device=dev, generator=g)
    y = torch.floor(torch.rand(N, dtype=torch.float64, device=dev, generator=g) ** 3 * 200.0)
    delta0 = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 5.0
    probes = rademacher_fill(dev, seed, J, N)
    rho = 0.7 / (1.0 + 1e-3 * 2)
    for r in R_VALUES:
        delta = delta0.clone()
        mean, sd, sc = pg_nb_estep_update(S, delta, y, r, rho, probes=probes if form == "probe_pointer" else None, seed=seed)
        resid, abs_err = sc.tolist()
        m_ref, sd_ref, d_ref, r_ref, a_ref = nb_estep_restated(S, delta0, y, r, rho, probes)
        e_sd = float((sd - sd_ref).abs().max() / sd_ref.abs().max())
        e_d = float((delta - d_ref).abs().max() / d_ref.abs().max())
        e_a = abs(abs_err - a_ref) / a_ref
        print(f"\n{form} r={r}: mean exact={torch.equal(mean, m_ref)} sigma_diag {e_sd:.1e} delta {e_d:.1e} "
              f"residual {resid:.17g} vs {r_ref:.17g} mae sum {abs_err:.17g} vs {a_ref:.17g} ({e_a:.1e})")
        assert torch.equal(mean, m_ref)
        assert e_sd <= 1e-14 and e_d <= 1e-14
        assert abs(resid - r_ref) <= 4 * np.finfo(np.float64).eps * abs(r_ref)
        assert e_a <= 1e-14
        if form == "device_hash":
            # the hash form regenerates exactly the probes efgp_rademacher_fill writes
            delta_p = delta0.clone()
            _, sd_p, sc_p = pg_nb_estep_update(S, delta_p, y, r, rho, probes=probes)
            assert torch.equal(sd, sd_p) and torch.equal(delta, delta_p) and torch.equal(sc, sc_p)


def test_total_count_grad_kernel_against_torch():
    from efgp_hip.ops import pg_nb_total_count_grad
    dev = torch.device("cuda", 0)
    N = 10 ** 6
    g = torch.Generator(device=dev).manual_seed(5)
    y = torch.floor(torch.rand(N, dtype=torch.float64, device=dev, generator=g) ** 4 * 10001.0)
    y[:3] = torch.tensor([0.0, 1.0, 1e4], dtype=torch.float64)
    mean = torch.randn(N, dtype=torch.float64, device=dev, generator=g) * 2.0
    var = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 3.0 - 0.3           # some negative variances
    for q in (1, 12, 64):
        x, w = gauss_hermite(q, dev)
        for r in R_VALUES:
            terms = total_count_grad_terms(y, mean, var, r, x, w)
            ref, scale = float(terms.sum()), float(terms.abs().sum())
            got = pg_nb_total_count_grad(y, mean, var, r, x, w)
            again = pg_nb_total_count_grad(y, mean, var, r, x, w)
            err = abs(float(got) - ref)
            print(f"\nQ={q} r={r}: grad {float(got):.17g} vs {ref:.17g}, |err| / sum|terms| = {err / scale:.1e}")
            assert err <= 1e-12 * scale
            assert torch.equal(got, again)


def test_device_digamma():
    """npts = 1, sigma_diag = 0, Q = 1, mean = -800: the log-sigmoid term is exactly 0, each call is digamma(y + r) - digamma(r)."""
    from efgp_hip.ops import pg_nb_total_count_grad
    dev = torch.device("cuda", 0)
    x, w = gauss_hermite(1, dev)
    mean = torch.full((1,), -800.0, dtype=torch.float64, device=dev)
    sd = torch.zeros(1, dtype=torch.float64, device=dev)
    worst = 0.0
    for r in (1e-3, 0.01, 0.05, 0.3, 1.0, 1.4616321449683622, 2.5, 9.99, 10.0, 37.5, 1e3, 1e4):
        for yv in (0.0, 1.0, 2.0, 7.0, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6):
            y = torch.full((1,), yv, dtype=torch.float64, device=dev)
            got = float(pg_nb_total_count_grad(y, mean, sd, r, x, w))
            a = torch.special.digamma(torch.tensor(yv + r, dtype=torch.float64))
            b = torch.special.digamma(torch.tensor(r, dtype=torch.float64))
            bound = 1e-14 * (abs(float(a)) + abs(float(b)))
            err = abs(got - float(a - b))
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (yv, r, got, float(a - b))
    print(f"\ndigamma: worst |err| / (1e-14 (|psi(y+r)| + |psi(r)|)) = {worst:.2f}")


def test_unseeded_device_probe_fit_on_2d_golden():
    """Device-hash probes (no reference stream): the fit lands near the seeded reference.  The bands (MAE within 5 %, held-out
    mean counts within 10 %) were set before any measurement; the first MI355X run gave 0.04 % and 0.05 %
    (profiles/pgnb_gpu_tests.txt), so they are loose but they hold."""
    g = np.load(GOLDEN[IDS.index("pgnb_se2d_fixed_n1000")])
    torch.manual_seed(0)
    reg = fit_golden(g, random_state=None)
    mae, mae_ref = reg.training_mean_absolute_error_, float(g["training_mean_absolute_error_"])
    held = rel(reg.predict(g["X_test"]), g["predict"])
    print(f"\nunseeded: mae {mae:.4f} (golden {mae_ref:.4f}, {abs(mae - mae_ref) / mae_ref:.2%}), held-out mean counts "
          f"{held:.2%} from the golden's")
    assert abs(mae - mae_ref) <= 0.05 * mae_ref
    assert held <= 0.10
    assert np.isfinite(reg.delta_).all() and np.isfinite(reg.beta_mean_).all()


def test_learnt_fit_at_one_million_points():
    from polyagamma_classification import PolyagammaGPNegativeBinomialRegressor
    from torch.distributions import NegativeBinomial
    gen = torch.Generator().manual_seed(6)
    N, r_true, r0 = 10 ** 6, 4.0, 1.0
    x = torch.rand(N, 2, dtype=torch.float64, generator=gen) * 2 - 1
    f = 1.2 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.5 * x[:, 1]) + 0.5 * x[:, 1]
    torch.manual_seed(6)
    y = NegativeBinomial(total_count=torch.tensor(r_true, dtype=torch.float64), logits=f).sample().numpy()
    reg = PolyagammaGPNegativeBinomialRegressor(total_count=r0, learn_total_count=True, total_count_update_frequency=1,
                                                total_count_lr=0.1, max_iter=10, device="cuda", store_history=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg.fit(x.numpy(), y)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    e_cg = [int(r["e_cg_iters"]) for r in reg.history_]
    m_cg = [int(r["m_cg_iters"]) for r in reg.history_]
    print(f"\nN = 1e6 NB fit (10 outer iterations, device probes, r learnt every iteration): {wall:.2f} s, r {r0} -> "
          f"{reg.total_count_:.4f} (true {r_true}), mae {reg.training_mean_absolute_error_:.4f}, lengthscale "
          f"{reg.lengthscale_:.4f} variance {reg.variance_:.4f}, E-step CG {e_cg}, M-step / mean CG {m_cg}")
    for attr in ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        assert np.isfinite(getattr(reg, attr)).all(), attr
    assert all(np.isfinite(v) for r in reg.history_ for v in r.values())
    assert abs(reg.total_count_ - r_true) < abs(r0 - r_true)
