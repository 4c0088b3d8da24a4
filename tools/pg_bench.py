#!/usr/bin/env python3
"""Timings of the Polya-Gamma classifier on one GPU (record only, nothing asserted):

    python tools/pg_bench.py [--out FILE] [--sizes 100000,1000000] [--skip-full-fit]

For d = 2 and each N (J = 10 probes), in both probe modes (seeded: the reference's host-generated probes, uploaded;
device: counter-hash probes generated in the kernels):
  * one outer iteration split into spectral rebuild / E-step / M-step / host (Adam step, scalar reads), median of 5,
    each phase closed by a device synchronisation;
  * a default 50-iteration fit (wall clock);
  * predict_proba on 1e4 held-out points (exact variance).
Plus efgp_pg_estep_update alone at N = 1e6, J = 10 (HIP events) and its bandwidth against its byte count.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def data(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 2, dtype=torch.float64, generator=g) * 2 - 1
    f = 2.0 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.5 * x[:, 1]) + 0.8 * x[:, 1]
    y = (torch.rand(N, dtype=torch.float64, generator=g) < torch.sigmoid(2.0 * f)).to(torch.int64)
    return x.numpy(), y.numpy()


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def outer_split(clf, reps=5):
    """Times the body of one outer iteration of fit() on a fitted classifier (same calls, same order)."""
    from polyagamma_classification.pg_classifier import _Spectral
    kernel = clf.kernel_
    raw = kernel._gp_params_ref.raw
    opt = torch.optim.Adam(kernel._gp_params_ref.parameters(), lr=clf.lr, maximize=True)
    lo, hi = clf._points.bounds()
    L = max(h - l for l, h in zip(lo, hi))
    rows = []
    for r in range(reps):
        seed = None if clf.random_state is None else int(clf.random_state) + 1000 * r
        t0 = sync()
        spec = _Spectral(kernel, clf._points, clf._xd, L, clf.spectral_eps, clf.trunc_eps, clf.nufft_eps)
        t1 = sync()
        clf._estep(spec, clf.e_step_iters, seed, r)
        t2 = sync()
        ms = clf._mstep(spec, seed, r)
        t3 = sync()
        g = [float(v) for v in ms["grad"].tolist()]
        raw.grad = torch.stack([torch.tensor(g[0], dtype=torch.float64).to(raw.dtype) * kernel.lengthscale,
                                torch.tensor(g[1], dtype=torch.float64).to(raw.dtype) * kernel.variance,
                                torch.tensor(0.0, dtype=raw.dtype)])
        opt.step()
        opt.zero_grad(set_to_none=True)
        t4 = sync()
        rows.append({"spectral_ms": 1e3 * (t1 - t0), "estep_ms": 1e3 * (t2 - t1), "mstep_ms": 1e3 * (t3 - t2),
                     "host_ms": 1e3 * (t4 - t3), "total_ms": 1e3 * (t4 - t0), "mtot": spec.mtot})
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}


def update_kernel_bandwidth(N=10 ** 6, J=10, reps=20):
    from efgp_hip.ops import pg_estep_update, rademacher_fill
    dev = torch.device("cuda", 0)
    S = torch.randn((J + 1, N), dtype=torch.float64, device=dev)
    y = (torch.rand(N, device=dev) > 0.5).to(torch.float64)
    delta = torch.full((N,), 0.25, dtype=torch.float64, device=dev)
    probes = rademacher_fill(dev, 5, J, N)
    out = {}
    for form, pr in (("probe_pointer", probes), ("device_hash", None)):
        for _ in range(3):
            pg_estep_update(S, delta, y, 0.5, probes=pr, seed=5)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            pg_estep_update(S, delta, y, 0.5, probes=pr, seed=5)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        # S rows, y, delta read + write, mean and sigma_diag written; the probe rows when they come from memory
        nbytes = N * 8 * ((J + 1) + 1 + 2 + 2 + (J if pr is not None else 0))
        out[form] = {"ms": ms, "bytes": nbytes, "GB_per_s": nbytes / (ms * 1e-3) / 1e9}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--skip-full-fit", action="store_true")
    args = ap.parse_args()
    from polyagamma_classification import PolyagammaGPClassifier
    res = {"device": torch.cuda.get_device_name(0), "J": 10, "d": 2, "cases": []}
    res["update_kernel"] = update_kernel_bandwidth()
    print(json.dumps(res["update_kernel"]), flush=True)
    gen = torch.Generator().manual_seed(9)
    xt = (torch.rand(10 ** 4, 2, dtype=torch.float64, generator=gen) * 2 - 1).numpy()
    for N in [int(s) for s in args.sizes.split(",")]:
        X, y = data(N)
        for mode, rs in (("seeded", 0), ("device", None)):
            clf = PolyagammaGPClassifier(max_iter=1, random_state=rs, device="cuda")
            clf.fit(X, y)                                     # warm-up: plans, FFT lengths, pools
            case = {"N": N, "mode": mode, "outer": outer_split(clf)}
            if not args.skip_full_fit:
                clf50 = PolyagammaGPClassifier(random_state=rs, device="cuda")
                t0 = sync()
                clf50.fit(X, y)
                case["fit50_s"] = sync() - t0
                case["fit50_accuracy"] = clf50.training_accuracy_
                clf50.predict_proba(xt[:64])
                t0 = sync()
                clf50.predict_proba(xt)
                case["predict_proba_1e4_s"] = sync() - t0
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
