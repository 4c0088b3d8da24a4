#!/usr/bin/env python3
"""Timings of the PG classifier's per-call predictive variances on one GPU (record only, nothing asserted):

    python tools/pg_variance_bench.py [--out FILE] [--train 100000] [--sizes 10000,100000,1000000]

The d = 2, J = 10 model of tools/pg_bench.py (default 50-iteration fit, device probes, mtot 17) at N = `--train`.  For each
n_test, wall clock of `predict_proba` closed by a device synchronisation, after one unrecorded call of the same shape:
  * variance_method="stochastic", cold (the lag-sum cache cleared: probes, one batched solve, efgp_lag_sums, then the type 2)
    and cached (median of 3);
  * variance_method="chebyshev", 7 nodes per axis (49 exact node solves + efgp_cheb_interp; median of 3);
  * the exact variance at n_test = 1e4 only: the figure the project had before, and the only baseline;
  * the cached stochastic call split into upload / latent mean / variance / response map and download.
Plus efgp_cheb_interp alone at 1e6 points for (d, n) = (2, 7), (3, 7), (3, 16): HIP events around 20 back-to-back launches on
the same inputs -- upper bounds on the rate, since the 8 d + 8 MB of a call stay in the 256-MB MALL between launches.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pg_bench import data, sync  # noqa: E402


def timed(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = sync()
        fn()
        out.append(sync() - t0)
    return statistics.median(out)


def kernel_alone(d, n, npts=10 ** 6, reps=20):
    from efgp_hip.lib import check, lib
    dev = torch.device("cuda", 0)
    k = np.arange(n, dtype=np.float64)
    nodes = np.sort(np.cos(np.pi * k / (n - 1)))
    w = (-1.0) ** k
    w[0] *= 0.5
    w[-1] *= 0.5
    nd = torch.as_tensor(np.tile(nodes, d)).to(dev)
    wt = torch.as_tensor(np.tile(w, d)).to(dev)
    vals = torch.rand(n ** d, dtype=torch.float64, device=dev)
    x = torch.rand(npts, d, dtype=torch.float64, device=dev) * 2 - 1
    out = torch.empty(npts, dtype=torch.float64, device=dev)
    counts = (C.c_int64 * d)(*([n] * d))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        check(lib().efgp_cheb_interp(0, d, counts, C.c_void_p(nd.data_ptr()), C.c_void_p(wt.data_ptr()), C.c_void_p(vals.data_ptr()),
                                     C.c_void_p(x.data_ptr()), npts, 1, C.c_void_p(out.data_ptr()), stream), "efgp_cheb_interp")

    for _ in range(3):
        launch()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        launch()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    nbytes = npts * 8 * (d + 1)                               # the point's coordinates read, one double written
    # per point: sum_a n_a divisions for the normalisers, then one division and one multiply-add per node of the box
    # (the innermost raw weight is recomputed) and one division per partial sum
    div = npts * (d * n + sum(n ** (a + 1) for a in range(d)) + sum(n ** a for a in range(d)))
    fma = npts * sum(n ** (a + 1) for a in range(d))
    return {"d": d, "n": n, "npts": npts, "ms": ms, "bytes": nbytes, "GB_per_s": nbytes / (ms * 1e-3) / 1e9,
            "divisions": div, "Gdiv_per_s": div / (ms * 1e-3) / 1e9, "multiply_adds": fma}


def split_cached_stochastic(clf, xt):
    """Where a cached stochastic predict_proba spends its time: the calls of predict_response_mean, each closed by a sync."""
    t0 = sync()
    xn = clf._device_points(xt)
    t1 = sync()
    mean = clf._latent_mean(xn)
    t2 = sync()
    var = clf._predictive_variance_at(xn, "stochastic")
    t3 = sync()
    p1 = np.clip(clf._response_mean(mean, var).cpu().numpy(), 1e-8, 1.0 - 1e-8)
    np.column_stack([1.0 - p1, p1])
    t4 = sync()
    return {"upload_s": t1 - t0, "latent_mean_s": t2 - t1, "variance_s": t3 - t2, "response_download_s": t4 - t3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", type=int, default=10 ** 5)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    args = ap.parse_args()
    from polyagamma_classification import PolyagammaGPClassifier
    res = {"device": torch.cuda.get_device_name(0), "d": 2, "J": 10, "N": args.train, "rows": [], "kernel": []}
    X, y = data(args.train)
    clf = PolyagammaGPClassifier(random_state=None, device="cuda")
    t0 = sync()
    clf.fit(X, y)
    res["fit50_s"] = sync() - t0
    res["mtot"] = int(clf._spec.mtot)
    res["predictive_variance_probes"] = int(clf.predictive_variance_probes)
    res["predictive_variance_chebyshev_nodes"] = int(clf.predictive_variance_chebyshev_nodes)
    gen = torch.Generator().manual_seed(9)
    for n_test in [int(s) for s in args.sizes.split(",")]:
        xt = (torch.rand(n_test, 2, dtype=torch.float64, generator=gen) * 2 - 1).numpy()
        row = {"n_test": n_test}
        clf.predict_proba(xt, variance_method="stochastic")                      # unrecorded: plans and FFT lengths of this shape
        clf._variance_sums_cache = None
        row["stochastic_cold_s"] = timed(lambda: clf.predict_proba(xt, variance_method="stochastic"), reps=1)
        row["stochastic_probe_solve_cg_iters"] = clf.last_variance_stats["cg_iters"]
        row["stochastic_cached_s"] = timed(lambda: clf.predict_proba(xt, variance_method="stochastic"))
        assert clf.last_variance_stats["cached"]
        row["stochastic_cached_split"] = split_cached_stochastic(clf, xt)
        clf.predict_proba(xt, variance_method="chebyshev")
        row["chebyshev_s"] = timed(lambda: clf.predict_proba(xt, variance_method="chebyshev"))
        if n_test <= 10 ** 4:
            clf.predict_proba(xt[:64])
            row["exact_s"] = timed(lambda: clf.predict_proba(xt))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    for d, n in ((2, 7), (3, 7), (3, 16)):
        res["kernel"].append(kernel_alone(d, n))
        print(json.dumps(res["kernel"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
