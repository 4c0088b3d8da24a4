#!/usr/bin/env python3
"""Timings of the Polya-Gamma classifier on one GPU (record only, nothing asserted):

    python tools/pg_bench.py [--out FILE] [--sizes 100000,1000000] [--skip-full-fit] [--likelihood {bernoulli,nb}]

For d = 2 and each N (J = 10 probes), in both probe modes (seeded: the reference's host-generated probes, uploaded;
device: counter-hash probes generated in the kernels):
  * one outer iteration split into spectral rebuild / E-step / M-step / host (Adam step, scalar reads), median of 5,
    each phase closed by a device synchronisation;
  * a default 50-iteration fit (wall clock);
  * predict_proba on 1e4 held-out points (exact variance).
Plus efgp_pg_estep_update alone at N = 1e6, J = 10 (HIP events) and its bandwidth against its byte count.

--likelihood nb measures the negative-binomial regressor instead (NB counts, r learnt every iteration so that each outer
iteration also pays the kappa refresh): the same phases plus `nb_ms` (the r gradient kernel, its read-back, the Adam step of
log r and the kappa refresh), the CG counts of the measured iterations, the classifier's outer iteration on the same points in
the same run, and efgp_pg_nb_estep_update / efgp_pg_nb_total_count_grad alone (HIP events) against their byte and operation
counts at each N.
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


def nb_data(N, r_true=4.0, seed=0):
    from torch.distributions import NegativeBinomial
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 2, dtype=torch.float64, generator=g) * 2 - 1
    f = 1.2 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.5 * x[:, 1]) + 0.5 * x[:, 1]
    torch.manual_seed(seed)
    y = NegativeBinomial(total_count=torch.tensor(r_true, dtype=torch.float64), logits=f).sample()
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
    nb = hasattr(clf, "_step_auxiliary") and getattr(clf, "learn_total_count", False)
    for r in range(reps):
        seed = None if clf.random_state is None else int(clf.random_state) + 1000 * r
        t0 = sync()
        if nb:
            clf._refresh_likelihood()                   # r moved in the previous repetition: the kappa refresh of the loop
        ta = sync()
        spec = _Spectral(kernel, clf._points, clf._xd, L, clf.spectral_eps, clf.trunc_eps, clf.nufft_eps)
        t1 = sync()
        est = clf._estep(spec, clf.e_step_iters, seed, r)
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
        row = {"spectral_ms": 1e3 * (t1 - ta), "estep_ms": 1e3 * (t2 - t1), "mstep_ms": 1e3 * (t3 - t2),
               "host_ms": 1e3 * (t4 - t3), "total_ms": 1e3 * (t4 - t0), "mtot": spec.mtot,
               "e_cg_iters": est["cg_iters"], "m_cg_iters": ms["cg_iters"]}
        if nb:
            clf._step_auxiliary(0)                      # r gradient + read-back + Adam step of log r (update_frequency 1)
            t5 = sync()
            row["nb_ms"] = 1e3 * ((t5 - t4) + (ta - t0))
            row["total_ms"] = 1e3 * (t5 - t0)
        rows.append(row)
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


def nb_kernel_timings(N, J=10, Q=12, r=4.0, reps=20):
    """efgp_pg_nb_estep_update (both probe forms) and efgp_pg_nb_total_count_grad alone under HIP events, with their byte
    and operation counts."""
    from efgp_hip.ops import pg_nb_estep_update, pg_nb_total_count_grad, rademacher_fill
    from polyagamma_classification import _gauss_hermite_normal_rule
    dev = torch.device("cuda", 0)
    S = torch.randn((J + 1, N), dtype=torch.float64, device=dev)
    y = torch.floor(torch.rand(N, dtype=torch.float64, device=dev) * 20.0)
    delta = torch.full((N,), 1.0, dtype=torch.float64, device=dev)
    sd = torch.rand(N, dtype=torch.float64, device=dev)
    probes = rademacher_fill(dev, 5, J, N)
    x, w = (torch.from_numpy(a.copy()).to(dev) for a in _gauss_hermite_normal_rule(Q))
    out = torch.empty(2, dtype=torch.float64, device=dev)
    g = torch.empty(1, dtype=torch.float64, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    res = {}
    for form, pr in (("probe_pointer", probes), ("device_hash", None)):
        ms = timed(lambda: pg_nb_estep_update(S, delta, y, r, 0.5, probes=pr, seed=5, out=out))
        # S rows, y, delta read + write, mean and sigma_diag written; the probe rows when they come from memory
        nbytes = N * 8 * ((J + 1) + 1 + 2 + 2 + (J if pr is not None else 0))
        res["nb_estep_update_" + form] = {"ms": ms, "bytes": nbytes, "GB_per_s": nbytes / (ms * 1e-3) / 1e9}
    ms = timed(lambda: pg_nb_total_count_grad(y, S[0], sd, r, x, w, out=g))
    nbytes = N * 8 * 3                                  # y, mean, sigma_diag
    # per point: Q (exp + log1p) pairs and one digamma(y + r) (one log, up to 10 reciprocals)
    res["nb_total_count_grad"] = {"ms": ms, "bytes": nbytes, "GB_per_s": nbytes / (ms * 1e-3) / 1e9, "Q": Q,
                                  "transcendentals": N * (2 * Q + 1),
                                  "Gtranscendentals_per_s": N * (2 * Q + 1) / (ms * 1e-3) / 1e9}
    return res


def main_nb(args):
    from polyagamma_classification import PolyagammaGPClassifier, PolyagammaGPNegativeBinomialRegressor
    res = {"device": torch.cuda.get_device_name(0), "likelihood": "nb", "J": 10, "d": 2, "r_true": 4.0, "cases": [],
           "kernels": {}}
    gen = torch.Generator().manual_seed(9)
    xt = (torch.rand(10 ** 4, 2, dtype=torch.float64, generator=gen) * 2 - 1).numpy()
    for N in [int(s) for s in args.sizes.split(",")]:
        res["kernels"][str(N)] = nb_kernel_timings(N)
        print(json.dumps({"N": N, "kernels": res["kernels"][str(N)]}), flush=True)
        X, y = nb_data(N)
        yb = (y > np.median(y)).astype(np.int64)            # the classifier on the same points, in the same run
        for mode, rs in (("seeded", 0), ("device", None)):
            reg = PolyagammaGPNegativeBinomialRegressor(max_iter=1, random_state=rs, device="cuda", learn_total_count=True,
                                                        total_count_update_frequency=1)
            reg.fit(X, y)                                     # warm-up: plans, FFT lengths, pools
            case = {"N": N, "mode": mode, "outer": outer_split(reg)}
            clf = PolyagammaGPClassifier(max_iter=1, random_state=rs, device="cuda")
            clf.fit(X, yb)
            case["classifier_outer"] = outer_split(clf)
            if not args.skip_full_fit:
                reg50 = PolyagammaGPNegativeBinomialRegressor(random_state=rs, device="cuda", learn_total_count=True)
                t0 = sync()
                reg50.fit(X, y)
                case["fit50_s"] = sync() - t0
                case["fit50_mae"] = reg50.training_mean_absolute_error_
                case["fit50_total_count"] = reg50.total_count_
                reg50.predict(xt[:64])
                t0 = sync()
                reg50.predict(xt)
                case["predict_1e4_s"] = sync() - t0
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--skip-full-fit", action="store_true")
    ap.add_argument("--likelihood", choices=("bernoulli", "nb"), default="bernoulli")
    args = ap.parse_args()
    if args.likelihood == "nb":
        res = main_nb(args)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
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
