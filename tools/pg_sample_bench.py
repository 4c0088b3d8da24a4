#!/usr/bin/env python3
"""Timings of posterior function draws on the Polya-Gamma classifier, one GPU (record only, nothing asserted):

    python tools/pg_sample_bench.py [--out FILE] [--sizes 1000000,10000000] [--rows 8] [--reps 7] [--outer 1]

Per size N (2-D, points uniform on [-1, 1]^2, the classifier's defaults: NUFFT tolerance 1e-7, CG tolerance 1e-6, plan on the fit's
point layout), after a fit of --outer outer iterations with device probes:
  transform, T = --rows rows on the fit's plan and mode box
    (a) fused scaled:  NufftPlan.type1_normal_scaled(seed, T, shape, sqrt(delta))   -- the row sqrt(delta) .* e1 never exists
    (b) unscaled:      NufftPlan.type1_normal(seed, T, shape)                        -- what the per-point factor costs on top
    (c) composed:      normal_fill -> multiply by sqrt(delta) in place -> NufftPlan.type1 from memory; these entry points are what
                       the library offered before the scaled entry (unchanged by it), so (c) is what a user could do without it
  plus the spread launches of (a) and (b) alone and both entries on a plan without the layout (where the factor is read in point order)
  whole draw, T rows at 128 test points: `sample_latent` and its four stages on their own (transform, right-hand side, solve, type 2),
  with the CG iteration counts next to the bound sqrt(cond) ln(2 / tol) / 2, cond = 1 + max(ws^2) sum(delta).
Times are HIP events around the enqueued work (torch.cuda.Event), after two warm-up calls, median of --reps with the spread.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))

import torch  # noqa: E402


def timed(fn, reps, warmup=2):
    """(median, min, max) in ms of fn() between two HIP events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    rows = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        rows.append(t0.elapsed_time(t1))
    return statistics.median(rows), min(rows), max(rows)


def put(row, key, res, per=1):
    row[key + "_ms"] = res[0] / per
    row[key + "_ms_spread"] = [res[1] / per, res[2] / per]


def bench_size(N, T, reps, outer):
    import efgpnd
    from efgp_hip import NufftPlan, cg_solve, hermitian_normal_rows, kernel_timing, kernel_timing_read, normal_fill
    from polyagamma_classification import PolyagammaGPClassifier
    gen = torch.Generator().manual_seed(N % 97)
    x = torch.rand(N, 2, dtype=torch.float64, generator=gen) * 2 - 1
    f = 2.0 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.5 * x[:, 1]) + 0.8 * x[:, 1]
    y = (torch.rand(N, dtype=torch.float64, generator=gen) < torch.sigmoid(2.0 * f)).to(torch.int64).numpy()
    torch.manual_seed(0)
    clf = PolyagammaGPClassifier(max_iter=outer, device="cuda").fit(x.numpy(), y)
    spec, dev = clf._spec, clf._dev
    M, shape, ws, plan = spec.M, spec.shape, spec.ws, spec.plan
    root = torch.sqrt(clf._delta)
    seed = 12345
    s1, s2 = efgpnd._derive_seed(seed, 1), efgpnd._derive_seed(seed, 2)
    cond = 1.0 + float((ws.abs() ** 2).max()) * float(clf._delta.sum())
    row = {"N": N, "rows": T, "mtot": spec.mtot, "outer_iterations": outer, "lengthscale": clf.lengthscale_, "variance": clf.variance_,
           "cond_bound": cond, "cg_tol": clf.cg_tol, "cg_iteration_bound": 0.5 * math.sqrt(cond) * math.log(2.0 / clf.cg_tol)}

    # the transform
    put(row, "type1_normal_scaled", timed(lambda: plan.type1_normal_scaled(s1, T, shape, root), reps))
    put(row, "type1_normal", timed(lambda: plan.type1_normal(s1, T, shape), reps))

    def composed():
        Z = normal_fill(dev, s1, T, N)
        Z.mul_(root)
        return plan.type1(Z, shape)
    put(row, "composed_fill_multiply_type1", timed(composed, reps))
    put(row, "composed_fill_only", timed(lambda: normal_fill(dev, s1, T, N), reps))
    Z = normal_fill(dev, s1, T, N)
    put(row, "composed_multiply_only", timed(lambda: Z.mul_(1.0), reps))
    put(row, "composed_type1_only", timed(lambda: plan.type1(Z, shape), reps))
    del Z
    # where the difference between (a) and (b) goes: the spread launches alone (the library's own event timers around them; the
    # rest of (a) - (b) is the max pass over sqrt(delta)), and both entries on a plan WITHOUT the layout, whose LDS spreader reads
    # the factor in point order (coalesced) where the layout's MFMA spreader gathers it through its permutation
    for key, fn in (("type1_normal_scaled", lambda: plan.type1_normal_scaled(s1, T, shape, root)),
                    ("type1_normal", lambda: plan.type1_normal(s1, T, shape))):
        fn()
        torch.cuda.synchronize()
        kernel_timing(True, only="spread")
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms, launches = kernel_timing_read("spread")
        kernel_timing(False)
        row[key + "_spread_kernels_ms"] = ms / reps
        row[key + "_spread_launches"] = launches // reps
    plain = NufftPlan(clf._xd, spec.h, clf.nufft_eps)
    put(row, "plain_plan_type1_normal_scaled", timed(lambda: plain.type1_normal_scaled(s1, T, shape, root), reps))
    put(row, "plain_plan_type1_normal", timed(lambda: plain.type1_normal(s1, T, shape), reps))
    del plain
    row["scaled_over_unscaled"] = row["type1_normal_scaled_ms"] / row["type1_normal_ms"]
    row["scaled_over_composed"] = row["type1_normal_scaled_ms"] / row["composed_fill_multiply_type1_ms"]

    # the whole draw and its stages
    idx = torch.randint(0, N, (128,), generator=torch.Generator().manual_seed(5))
    xn_np = x[idx].numpy()
    xn = torch.as_tensor(xn_np).to(dev).contiguous()
    put(row, "sample_latent_per_draw", timed(lambda: clf.sample_latent(xn_np, T, seed=seed), reps), T)
    its = clf.last_sample_stats["cg_iters"]
    row["cg_iters"] = {"min": min(its), "median": statistics.median(its), "max": max(its)}
    plan_new = NufftPlan(xn, spec.h, clf.nufft_eps)
    keep = {}

    def st_type1():
        keep["fz"] = plan.type1_normal_scaled(s1, T, shape, root).reshape(T, M)

    def st_rhs():
        keep["rhs"] = hermitian_normal_rows(dev, s2, T, M, a=1.0, ws=ws, fz=keep["fz"], b=1.0)

    def st_cg():
        keep["u"], _, _ = cg_solve(clf._op_pred, ws, 1.0, 1, keep["rhs"], None, clf.cg_tol, max_iter=2000, early_stop=True, batched=True,
                                   hermitian=True)

    def st_type2():
        u = keep["u"].reshape(T, M)
        w = 0.5 * (u + u.flip(1).conj()) + (ws * clf._beta_mean).reshape(1, M)
        keep["f"] = plan_new.type2(w, shape, real_only=True, batched=True, mode_scale=ws)
    for name, fn in (("transform", st_type1), ("rhs", st_rhs), ("solve", st_cg), ("type2", st_type2)):
        put(row, f"stage_{name}_per_draw", timed(fn, reps), T)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pg_sample_bench_mi355x.json"))
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--outer", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pg_sample_bench.py needs a GPU: a CPU run says nothing about these timings")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dimension": 2, "nufft_eps": 1e-7, "layout": True,
           "timer": "HIP events, 2 warm-up calls, median of %d" % args.reps, "sizes": []}
    for N in [int(float(s)) for s in args.sizes.split(",") if s]:
        res["sizes"].append(bench_size(N, args.rows, args.reps, args.outer))
        print(json.dumps(res["sizes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
