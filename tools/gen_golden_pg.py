#!/usr/bin/env python3
"""Goldens of the Polya-Gamma GP classifier, produced by running the REFERENCE's own `PolyagammaGPClassifier`
(polyagamma_classification/pg_classifier.py) on the CPU of the build container:

    python tools/gen_golden_pg.py            -> tests/golden/pg_<case>.npz

The reference directory is put on sys.path with `oracle/standin` as `pytorch_finufft` (exact NUDFT), device="cpu",
random_state fixed, store_history=True.  The stand-in accumulates its chunks in place, which `torch.vmap` cannot trace, so
`pg_classifier.vmap` is replaced by a loop that stacks the per-row results -- the same numbers, row by row.

Each file holds the inputs (X, y, held-out X_test), the constructor settings, the per-outer history (one array per
record key), the fitted attributes, decision_function / predictive_variance / predict_proba / predict on X_test, and
reference values of approximate_logistic_gaussian_prob and _pg_omega_expectation on a fixed grid of inputs.
Nothing on the GPU machine reads the reference: these files are all the GPU tests need.
"""
import json
import math
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

import pg_classifier as P  # noqa: E402  (the reference)

GOLD = os.path.join(ROOT, "tests", "golden")


def _stacking_vmap(fn, in_dims=0, out_dims=0):
    assert in_dims == 0 and out_dims == 0
    return lambda t: torch.stack([fn(row) for row in t], dim=0)


P.vmap = _stacking_vmap


def latent(x):
    d = x.shape[1]
    f = 2.0 * torch.sin(3.0 * x[:, 0])
    if d >= 2:
        f = f * torch.cos(2.5 * x[:, 1]) + 0.8 * x[:, 1]
    if d >= 3:
        f = f + torch.sin(2.0 * x[:, 2])
    return f


def make_data(N, n_test, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N + n_test, d, dtype=torch.float64, generator=g) * 2 - 1
    p = torch.sigmoid(2.0 * latent(x))
    y = (torch.rand(N + n_test, dtype=torch.float64, generator=g) < p).to(torch.int64)
    return x[:N].numpy(), y[:N].numpy(), x[N:].numpy()


CASES = {
    "se2d_n1000": dict(N=1000, n_test=200, d=2, seed=11,
                       params=dict(lengthscale_init=0.3, variance_init=1.0, max_iter=8, random_state=7)),
    "se1d_n500": dict(N=500, n_test=150, d=1, seed=12,
                      params=dict(lengthscale_init=0.2, variance_init=1.5, max_iter=8, random_state=3)),
    "se3d_n500": dict(N=500, n_test=100, d=3, seed=13,
                      params=dict(lengthscale_init=0.6, variance_init=1.0, max_iter=6, spectral_eps=1e-3, trunc_eps=1e-3,
                                  random_state=5)),
}


def helper_values():
    g = torch.Generator().manual_seed(99)
    mean = torch.randn(64, dtype=torch.float64, generator=g) * 3
    var = torch.rand(64, dtype=torch.float64, generator=g) * 4 - 0.5
    c = torch.cat([torch.tensor([0.0, 1e-13, 1e-9, 1e-8, 2e-8, 1e-6], dtype=torch.float64),
                   torch.rand(58, dtype=torch.float64, generator=g) * 20])
    b = torch.rand(64, dtype=torch.float64, generator=g) * 3 + 0.5
    return {"helper_mean": mean.numpy(), "helper_var": var.numpy(),
            "helper_prob": P.approximate_logistic_gaussian_prob(mean, var).numpy(),
            "helper_prob_novar": P.approximate_logistic_gaussian_prob(mean).numpy(),
            "helper_c": c.numpy(), "helper_b": b.numpy(), "helper_omega": P._pg_omega_expectation(c, b).numpy()}


def run_case(name, spec):
    X, y, Xt = make_data(spec["N"], spec["n_test"], spec["d"], spec["seed"])
    params = dict(spec["params"], device="cpu", store_history=True)
    t0 = time.time()
    clf = P.PolyagammaGPClassifier(**params).fit(X, y)
    fit_s = time.time() - t0
    out = {"X": X, "y": y, "X_test": Xt, "params": json.dumps(params), "torch_default_dtype": str(torch.get_default_dtype())}
    keys = sorted(clf.history_[0].keys())
    out["history_keys"] = np.array(keys)
    for k in keys:
        out["history_" + k] = np.array([float(r[k]) for r in clf.history_])
    for attr in ("classes_", "delta_", "posterior_mean_", "posterior_var_diag_", "beta_mean_", "m_step_gradient_"):
        out[attr] = np.asarray(getattr(clf, attr))
    for attr in ("lengthscale_", "variance_", "training_accuracy_", "n_iter_"):
        out[attr] = np.float64(getattr(clf, attr))
    out["decision_function"] = clf.decision_function(Xt)
    out["predictive_variance"] = clf.predictive_variance(Xt)
    out["predict_proba"] = clf.predict_proba(Xt)
    out["predict"] = clf.predict(Xt)
    out["mtot"] = np.int64(clf._spectral_state_.mtot)
    out["h"] = np.float64(clf._spectral_state_.h)
    out.update(helper_values())
    path = os.path.join(GOLD, f"pg_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: fit {fit_s:.1f} s, mtot {out['mtot']}, accuracy {clf.training_accuracy_:.4f}, "
          f"lengthscale {clf.lengthscale_:.6f}, variance {clf.variance_:.6f} -> {path} ({os.path.getsize(path)} bytes)")


def main():
    torch.set_num_threads(8)
    names = sys.argv[1:] or list(CASES)
    for name in names:
        run_case(name, CASES[name])


if __name__ == "__main__":
    main()
