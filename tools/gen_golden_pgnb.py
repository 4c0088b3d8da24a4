#!/usr/bin/env python3
"""Goldens of the Polya-Gamma negative-binomial GP regressor, produced by running the REFERENCE's own
`PolyagammaGPNegativeBinomialRegressor` (polyagamma_classification/pg_classifier.py) on the CPU of the build container:

    python tools/gen_golden_pgnb.py            -> tests/golden/pgnb_<case>.npz

Set-up as tools/gen_golden_pg.py: the reference directory on sys.path with `oracle/standin` as `pytorch_finufft` (exact
NUDFT), device="cpu", random_state fixed, store_history=True, and `pg_classifier.vmap` replaced by a loop that stacks the
per-row results.  Counts are drawn from torch.distributions.NegativeBinomial(total_count=r_true, logits=f(x)) under a fixed
torch seed.  The files are named pgnb_*, apart from the classifier's pg_*.

Each file holds the inputs (X, y, held-out X_test), the constructor settings, the reference's default get_params() as JSON,
the per-outer history (one array per record key, and the keys in the reference's order), the fitted attributes,
decision_function / predictive_variance / predict on X_test, and reference values of negative_binomial_gaussian_mean,
_gauss_hermite_normal_rule (Q = 12, 16, 64), _expected_log_sigmoid_negative_gaussian and
_negative_binomial_total_count_gradient on fixed inputs.  Nothing on the GPU machine reads the reference.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("GP_QUADRATURE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "oracle", "standin"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "polyagamma_classification"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.distributions import NegativeBinomial  # noqa: E402

import pg_classifier as P  # noqa: E402  (the reference)

GOLD = os.path.join(ROOT, "tests", "golden")


def _stacking_vmap(fn, in_dims=0, out_dims=0):
    assert in_dims == 0 and out_dims == 0
    return lambda t: torch.stack([fn(row) for row in t], dim=0)


P.vmap = _stacking_vmap


def latent(x):
    d = x.shape[1]
    f = 1.2 * torch.sin(3.0 * x[:, 0])
    if d >= 2:
        f = f * torch.cos(2.5 * x[:, 1]) + 0.5 * x[:, 1]
    if d >= 3:
        f = f + 0.6 * torch.sin(2.0 * x[:, 2])
    return f


def make_data(N, n_test, d, seed, r_true):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N + n_test, d, dtype=torch.float64, generator=g) * 2 - 1
    torch.manual_seed(seed)
    y = NegativeBinomial(total_count=torch.tensor(r_true, dtype=torch.float64), logits=latent(x)).sample().to(torch.int64)
    return x[:N].numpy(), y[:N].numpy(), x[N:].numpy()


CASES = {
    "se2d_fixed_n1000": dict(N=1000, n_test=200, d=2, seed=21, r_true=3.0,
                             params=dict(total_count=3.0, lengthscale_init=0.3, variance_init=1.0, max_iter=8, random_state=7)),
    "se1d_learn_n500": dict(N=500, n_test=150, d=1, seed=22, r_true=4.0,
                            params=dict(total_count=1.5, learn_total_count=True, total_count_lr=0.08, total_count_update_frequency=2,
                                        total_count_quadrature_nodes=16, lengthscale_init=0.2, variance_init=1.0, max_iter=8,
                                        random_state=3)),
    "se3d_learn_n500": dict(N=500, n_test=100, d=3, seed=23, r_true=5.0,
                            params=dict(total_count=2.0, learn_total_count=True, total_count_update_frequency=1,
                                        lengthscale_init=0.6, variance_init=1.0, max_iter=6, spectral_eps=1e-3, trunc_eps=1e-3,
                                        random_state=5)),
}


def helper_values():
    g = torch.Generator().manual_seed(98)
    out = {}
    mean = torch.randn(64, dtype=torch.float64, generator=g) * 1.5
    var = torch.rand(64, dtype=torch.float64, generator=g) * 4 - 0.5
    out.update(helper_nb_mean_in=mean.numpy(), helper_nb_var_in=var.numpy(), helper_nb_total_count=np.float64(2.7),
               helper_nb_mean=P.negative_binomial_gaussian_mean(mean, var, total_count=2.7).numpy())
    for q in (12, 16, 64):
        nodes, weights = P._gauss_hermite_normal_rule(q)
        out[f"helper_gh{q}_nodes"], out[f"helper_gh{q}_weights"] = np.array(nodes), np.array(weights)
    mean = torch.randn(64, dtype=torch.float64, generator=g) * 3
    var = torch.rand(64, dtype=torch.float64, generator=g) * 4 - 0.5
    out.update(helper_els_mean=mean.numpy(), helper_els_var=var.numpy())
    for q in (12, 64):
        out[f"helper_els_q{q}"] = P._expected_log_sigmoid_negative_gaussian(mean, var, quadrature_nodes=q).numpy()
    # the r gradient: counts 0 .. 1e4, some negative variances, r in {0.05, 1, 37.5}
    y = torch.cat([torch.tensor([0, 1, 2, 3, 5, 10, 100, 1000, 10000], dtype=torch.float64),
                   torch.randint(0, 10001, (55,), generator=g).to(torch.float64)])
    mean = torch.randn(64, dtype=torch.float64, generator=g) * 2
    var = torch.rand(64, dtype=torch.float64, generator=g) * 3 - 0.3
    rs = np.array([0.05, 1.0, 37.5])
    out.update(helper_tcg_y=y.numpy(), helper_tcg_mean=mean.numpy(), helper_tcg_var=var.numpy(), helper_tcg_r=rs)
    for q in (12, 16):
        out[f"helper_tcg_q{q}"] = np.array([float(P._negative_binomial_total_count_gradient(
            y, mean, var, total_count=float(r), quadrature_nodes=q)) for r in rs])
    return out


def run_case(name, spec):
    X, y, Xt = make_data(spec["N"], spec["n_test"], spec["d"], spec["seed"], spec["r_true"])
    params = dict(spec["params"], device="cpu", store_history=True)
    t0 = time.time()
    reg = P.PolyagammaGPNegativeBinomialRegressor(**params).fit(X, y)
    fit_s = time.time() - t0
    out = {"X": X, "y": y, "X_test": Xt, "params": json.dumps(params), "r_true": np.float64(spec["r_true"]),
           "torch_default_dtype": str(torch.get_default_dtype()),
           "default_params": json.dumps(P.PolyagammaGPNegativeBinomialRegressor().get_params())}
    keys = list(reg.history_[0].keys())
    out["history_keys"] = np.array(keys)
    for k in keys:
        out["history_" + k] = np.array([float(r[k]) for r in reg.history_])
    for attr in ("delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        out[attr] = np.asarray(getattr(reg, attr))
    for attr in ("lengthscale_", "variance_", "training_metric_", "training_mean_absolute_error_", "total_count_",
                 "shape_parameter_", "n_iter_"):
        out[attr] = np.float64(getattr(reg, attr))
    out["decision_function"] = reg.decision_function(Xt)
    out["predictive_variance"] = reg.predictive_variance(Xt)
    out["predict"] = reg.predict(Xt)
    out["mtot"] = np.int64(reg._spectral_state_.mtot)
    out["h"] = np.float64(reg._spectral_state_.h)
    out.update(helper_values())
    path = os.path.join(GOLD, f"pgnb_{name}.npz")
    np.savez_compressed(path, **out)
    upd = int(out["history_total_count_updated"].sum())
    print(f"{name}: fit {fit_s:.1f} s, mtot {out['mtot']}, counts {y.min()}..{y.max()}, mae {reg.training_mean_absolute_error_:.4f}, "
          f"r {out['history_total_count'][0]:.4f} -> {reg.total_count_:.4f} ({upd} updates), "
          f"cg {out['history_e_cg_iters'].min():.0f}..{out['history_e_cg_iters'].max():.0f}, lengthscale {reg.lengthscale_:.6f}, "
          f"variance {reg.variance_:.6f} -> {path} ({os.path.getsize(path)} bytes)")


def main():
    torch.set_num_threads(8)
    names = sys.argv[1:] or list(CASES)
    for name in names:
        run_case(name, CASES[name])


if __name__ == "__main__":
    main()
