#!/usr/bin/env python3
"""Goldens of the approximate predictive variances of the Polya-Gamma GP classifier, produced by the REFERENCE's own
`PolyagammaGPClassifier` on the CPU of the build container (never on a GPU machine):

    python tools/gen_golden_pg_variance.py            -> tests/golden/variance_pg_<case>.npz

The set-up is that of tools/gen_golden_pg.py, imported from it: the reference directory on sys.path with `oracle/standin` as
`pytorch_finufft` (exact NUDFT), the stacking stand-in for `torch.vmap`, device="cpu".  For each case the reference is refitted on the X, y and
constructor settings stored in tests/golden/pg_<case>.npz, and its `delta_` must agree with that file's to 1e-12 relative: both
files then describe one fit.  `predictive_variance_method` is then set on the fitted object and, at that file's X_test,

    variance_stochastic / proba_stochastic    "stochastic", the reference's default 16 probes (seed random_state + 2_000_000),
    variance_chebyshev  / proba_chebyshev     "chebyshev", 7 nodes per axis (5 for the 3-D case: 125 node solves)

are recorded.  Neither X, y nor the lag box is stored: each file is a few KB.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden_pg as G  # noqa: E402  (puts the reference and the stand-ins in place; G.P is the reference's module)

P = G.P
GOLD = G.GOLD
CASES = {"se2d_n1000": 7, "se1d_n500": 7, "se3d_n500": 5}          # Chebyshev nodes per axis


def run_case(name, n_cheb):
    fit = np.load(os.path.join(GOLD, f"pg_{name}.npz"), allow_pickle=False)
    params = json.loads(str(fit["params"]))
    clf = P.PolyagammaGPClassifier(**params).fit(fit["X"], fit["y"])
    rel = float(np.linalg.norm(clf.delta_ - fit["delta_"]) / np.linalg.norm(fit["delta_"]))
    assert rel <= 1e-12, f"{name}: refit delta_ differs from pg_{name}.npz by {rel:.3e} relative"
    Xt = fit["X_test"]
    out = {"case": np.array(name), "delta_rel_to_fit_golden": np.float64(rel), "n_test": np.int64(Xt.shape[0]),
           "random_state": np.int64(params["random_state"])}

    clf.predictive_variance_method = "stochastic"
    out["n_probes"] = np.int64(clf.predictive_variance_probes)
    out["variance_stochastic"] = np.asarray(clf.predictive_variance(Xt), dtype=np.float64)
    out["proba_stochastic"] = np.asarray(clf.predict_proba(Xt), dtype=np.float64)
    out["stochastic_cg_iters"] = np.int64(clf._stochastic_predictive_variance_info_["cg_iters"])

    clf.predictive_variance_method = "chebyshev"
    clf.predictive_variance_chebyshev_nodes = n_cheb
    out["chebyshev_nodes"] = np.int64(n_cheb)
    out["variance_chebyshev"] = np.asarray(clf.predictive_variance(Xt), dtype=np.float64)
    out["proba_chebyshev"] = np.asarray(clf.predict_proba(Xt), dtype=np.float64)

    path = os.path.join(GOLD, f"variance_pg_{name}.npz")
    np.savez_compressed(path, **out)
    exact = fit["predictive_variance"]
    print(f"{name}: delta rel {rel:.2e}; stochastic vs exact {np.linalg.norm(out['variance_stochastic'] - exact) / np.linalg.norm(exact):.3e}, "
          f"chebyshev vs exact {np.linalg.norm(out['variance_chebyshev'] - exact) / np.linalg.norm(exact):.3e} -> {path} "
          f"({os.path.getsize(path)} bytes)")


def main():
    torch.set_num_threads(8)
    for name in sys.argv[1:] or list(CASES):
        run_case(name, CASES[name])


if __name__ == "__main__":
    main()
