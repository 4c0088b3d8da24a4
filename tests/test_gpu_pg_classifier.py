"""Polya-Gamma GP classifier on the MI355X: seeded fits against the reference's own classifier (tests/golden/pg_*.npz, made by
tools/gen_golden_pg.py with the exact-NUDFT stand-in), reproducibility, the new kernels against torch restatements, an
unseeded device-probe fit and one fit at N = 1e6."""
import glob
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from _pg_edges import estep_restated as _estep_restated

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pg_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in GOLDEN]

# Tolerances against the reference: the goldens are exact NUDFTs, the fits run at nufft_eps = 1e-7 and cg_tol = 1e-6.
REL = 1e-5


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _dtype(name):
    return {"torch.float32": torch.float32, "torch.float64": torch.float64}[name]


def fit_golden(g, **over):
    from polyagamma_classification import PolyagammaGPClassifier
    params = json.loads(str(g["params"]))
    params.update(device="cuda", store_history=True)
    params.update(over)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(_dtype(str(g["torch_default_dtype"])))      # the dtype the reference's hyper-parameters lived in
    try:
        return PolyagammaGPClassifier(**params).fit(g["X"], g["y"])
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
    g, clf = seeded(path)
    hist = {k: np.array([r[k] for r in clf.history_]) for k in clf.history_[0]}
    dev = {
        "lengthscale": rel(hist["lengthscale"], g["history_lengthscale"]),
        "variance": rel(hist["variance"], g["history_variance"]),
        "grad_lengthscale": rel(hist["grad_lengthscale"], g["history_grad_lengthscale"]),
        "grad_variance": rel(hist["grad_variance"], g["history_grad_variance"]),
        "delta_": rel(clf.delta_, g["delta_"]),
        "posterior_mean_": rel(clf.posterior_mean_, g["posterior_mean_"]),
        "posterior_var_diag_": rel(clf.posterior_var_diag_, g["posterior_var_diag_"]),
        "beta_mean_": rel(clf.beta_mean_, g["beta_mean_"]),
        "m_step_gradient_": rel(clf.m_step_gradient_, g["m_step_gradient_"]),
        "decision_function": rel(clf.decision_function(g["X_test"]), g["decision_function"]),
        "predictive_variance": rel(clf.predictive_variance(g["X_test"]), g["predictive_variance"]),
    }
    proba = clf.predict_proba(g["X_test"])
    dp = float(np.abs(proba - g["predict_proba"]).max())
    de = np.abs(hist["e_cg_iters"] - g["history_e_cg_iters"]).max()
    dm = np.abs(hist["m_cg_iters"] - g["history_m_cg_iters"]).max()
    print(f"\n{os.path.basename(path)}: " + " ".join(f"{k}={v:.1e}" for k, v in dev.items()) +
          f" proba={dp:.1e} d_e_cg={de} d_m_cg={dm} acc={clf.training_accuracy_} ref={float(g['training_accuracy_'])}")
    assert len(clf.history_) == len(g["history_iter"])
    for k, v in dev.items():
        assert v <= REL, (k, v)
    assert de <= 1 and dm <= 1
    assert clf.training_accuracy_ == float(g["training_accuracy_"])
    assert dp <= 1e-6
    np.testing.assert_array_equal(clf.predict(g["X_test"]), g["predict"])
    assert abs(clf.lengthscale_ - float(g["lengthscale_"])) <= REL * float(g["lengthscale_"])
    assert abs(clf.variance_ - float(g["variance_"])) <= REL * float(g["variance_"])
    # every solve of the fit went through the fused device solver
    solves = clf.last_fit_stats["solves"]
    P = json.loads(str(g["params"]))["max_iter"]
    assert len(solves) == 2 * P + 2
    assert all(s["fused"] and s["entry"] == "efgp_cg_solve" for s in solves)
    assert [s["cg_iters"] for s in solves if s["step"] == "estep"] == list(hist["e_cg_iters"].astype(int))


def test_seeded_fits_are_bit_identical():
    g, a = seeded(GOLDEN[IDS.index("pg_se2d_n1000")])
    b = fit_golden(g)
    for attr in ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        assert np.array_equal(getattr(a, attr), getattr(b, attr)), attr
    assert a.history_ == b.history_
    assert np.array_equal(a.predict_proba(g["X_test"]), b.predict_proba(g["X_test"]))


@pytest.mark.parametrize("form", ["probe_pointer", "device_hash"])
def test_estep_update_kernel_against_torch(form):
    from efgp_hip.ops import pg_estep_update, rademacher_fill
    dev = torch.device("cuda", 0)
    N, J, seed = 10 ** 6, 10, 12345
    g = torch.Generator(device=dev).manual_seed(1)
    S = torch.randn((J + 1, N), dtype=torch.float64, device=dev, generator=g)
    S[0] *= 2.0
    y = (torch.rand(N, dtype=torch.float64, device=dev, generator=g) > 0.5).to(torch.float64)
    delta0 = torch.rand(N, dtype=torch.float64, device=dev, generator=g) * 0.3
    pg_b = torch.rand(N, dtype=torch.float64, device=dev, generator=g) + 0.5 if form == "probe_pointer" else None
    probes = rademacher_fill(dev, seed, J, N)
    rho = 0.7 / (1.0 + 1e-3 * 2)
    delta = delta0.clone()
    if form == "probe_pointer":
        mean, sd, r, c = pg_estep_update(S, delta, y, rho, probes=probes, pg_b=pg_b)
    else:
        mean, sd, r, c = pg_estep_update(S, delta, y, rho, probes=None, seed=seed)
        # the hash form regenerates exactly the probes efgp_rademacher_fill writes
        delta_p = delta0.clone()
        mean_p, sd_p, r_p, c_p = pg_estep_update(S, delta_p, y, rho, probes=probes)
        assert torch.equal(sd, sd_p) and torch.equal(delta, delta_p) and torch.equal(r, r_p) and torch.equal(c, c_p)
    m_ref, sd_ref, d_ref, r_ref, c_ref = _estep_restated(S, delta0, y, rho, probes, pg_b)
    e_sd = float((sd - sd_ref).abs().max() / sd_ref.abs().max())
    e_d = float((delta - d_ref).abs().max() / d_ref.abs().max())
    print(f"\n{form}: mean exact={torch.equal(mean, m_ref)} sigma_diag {e_sd:.1e} delta {e_d:.1e} "
          f"residual {float(r):.17g} vs {r_ref:.17g} count {int(c)} vs {c_ref}")
    assert torch.equal(mean, m_ref)
    assert e_sd <= 1e-14 and e_d <= 1e-14
    # The per-point values of the kernel and of torch's elementwise ops (tanh, the damped update) differ by an ulp now and then
    # (measured: delta 2.1e-16 to 3.2e-16 relative, max residual 0.075347095535661351 vs ...379), so the max over 1e6 points
    # agrees to a few ulp, not always bit for bit; the integer count is exact.
    assert abs(float(r) - r_ref) <= 1.6e-15 * abs(r_ref)
    assert int(c) == c_ref


def test_mstep_terms_kernel_against_einsum():
    from efgp_hip.ops import pg_mstep_terms
    dev = torch.device("cuda", 0)
    M, J = 31 * 31, 10
    g = torch.Generator(device=dev).manual_seed(2)

    def crandn(*shape):
        return torch.complex(torch.randn(shape, dtype=torch.float64, device=dev, generator=g),
                             torch.randn(shape, dtype=torch.float64, device=dev, generator=g))
    bx, bj, R = crandn(M), crandn(J, M), crandn(J, M)
    dpr = torch.rand((M, 2), dtype=torch.float64, device=dev, generator=g)
    t1 = torch.einsum("kp,k->p", dpr, (bx.conj() * bx).real)
    t2 = torch.einsum("jk,kp->jp", (R.conj() * bj).real, dpr).mean(dim=0)
    for dp in (dpr.contiguous(), dpr.to(torch.complex128).contiguous()):
        out = pg_mstep_terms(bx, bj, R, dp)
        assert float((out[:2] - t1).abs().max() / t1.abs().max()) <= 1e-12
        assert float((out[2:4] - t2).abs().max() / t2.abs().max()) <= 1e-12
        assert float((out[4:6] - 0.5 * (t1 - t2)).abs().max() / (0.5 * (t1 - t2)).abs().max()) <= 1e-12
    assert torch.equal(pg_mstep_terms(bx, bj, R, dpr.contiguous()), pg_mstep_terms(bx, bj, R, dpr.contiguous()))


def test_weight_rows_kernel():
    from efgp_hip.ops import pg_weight_rows, rademacher_fill
    dev = torch.device("cuda", 0)
    N, J = 100003, 3
    omega = torch.rand(N, dtype=torch.float64, device=dev)
    z = rademacher_fill(dev, 77, J, N)
    assert torch.equal(pg_weight_rows(omega, J, seed=77), omega * z)
    assert torch.equal(pg_weight_rows(omega, J, probes=z), omega * z)


def test_unseeded_device_probe_fit_on_2d_golden():
    g = np.load(GOLDEN[IDS.index("pg_se2d_n1000")])
    torch.manual_seed(0)
    clf = fit_golden(g, random_state=None)
    agree = float(np.mean(clf.predict(g["X_test"]) == g["predict"]))
    print(f"\nunseeded: accuracy {clf.training_accuracy_:.4f} (golden {float(g['training_accuracy_']):.4f}), "
          f"held-out label agreement {agree:.3f}")
    assert abs(clf.training_accuracy_ - float(g["training_accuracy_"])) <= 0.03
    assert agree >= 0.95
    assert np.isfinite(clf.delta_).all() and np.isfinite(clf.beta_mean_).all()


def test_fit_at_one_million_points():
    from polyagamma_classification import PolyagammaGPClassifier
    gen = torch.Generator().manual_seed(4)
    N = 10 ** 6
    x = torch.rand(N, 2, dtype=torch.float64, generator=gen) * 2 - 1
    f = 2.0 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.5 * x[:, 1]) + 0.8 * x[:, 1]
    y = (torch.rand(N, dtype=torch.float64, generator=gen) < torch.sigmoid(2.0 * f)).to(torch.int64).numpy()
    bayes = float(((torch.sigmoid(2.0 * f) > 0.5).to(torch.int64).numpy() == y).mean())
    clf = PolyagammaGPClassifier(max_iter=10, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    clf.fit(x.numpy(), y)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"\nN = 1e6 fit (10 outer iterations, device probes): {wall:.2f} s, accuracy {clf.training_accuracy_:.4f} "
          f"(Bayes {bayes:.4f}), lengthscale {clf.lengthscale_:.4f} variance {clf.variance_:.4f}")
    assert wall < 120.0
    for attr in ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        assert np.isfinite(getattr(clf, attr)).all(), attr
    assert clf.training_accuracy_ > 0.70 and clf.training_accuracy_ > bayes - 0.05
