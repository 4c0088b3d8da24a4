#!/usr/bin/env python3
"""B outputs at shared points: EFGPNDMulti against a loop of B single-output EFGPND models (record only, nothing asserted).

    python tools/multi_output_bench.py [--out FILE] [--sizes 100000,1000000] [--outputs 1,8,64,256] [--reps 5] [--timeout 240]

d = 2, the SE kernel on the headline grid (l = 0.2, eps = 1e-4: 23 x 23 modes; nufft_eps 1e-7, CG tolerance 1e-4).  Per (N, B):
  fit + predict   EFGPNDMulti.fit() and predict at the N training points (mean only: the variance does not depend on Y and costs
                  both variants the same) against B x (EFGPND.fit() + predict) -- the single-output code path, untouched;
  gradient        one EFGPNDMulti.compute_gradients(trace_samples=10) against B single-output compute_gradients.
Every (N, B) runs in a child process of its own under its own time limit (a child that fails or runs out of time ends the sweep:
nothing further is started on the device).  In a child both variants are warmed up on the shapes they are timed on, then timed
alternately, --reps times each; a time is a host clock around work that ends in a device synchronisation; median, min and max
are kept.  Both variants see the same data and hyper-parameters, and the child also records the largest difference of their means
relative to max|mean|, separately for the rows whose solve stopped at the same iteration as the single-output model's and for the
others.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))


def one(N, B, reps):
    import torch
    from efgpnd import EFGPND
    from efgpnd_multi import EFGPNDMulti
    from kernels.squared_exponential import SquaredExponential

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    g = torch.Generator(device="cuda").manual_seed(N % 97 + B)
    x = torch.rand(N, 2, generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    phase = torch.arange(B, dtype=torch.float64, device="cuda")[None, :]
    Y = torch.sin(3 * x[:, :1] + 0.3 * phase) * torch.cos(4 * x[:, 1:] - 0.2 * phase) \
        + math.sqrt(0.2) * torch.randn(N, B, generator=g, dtype=torch.float64, device="cuda")
    # no warm start: a refit with unchanged hyper-parameters would otherwise find its solution in the start vector
    opts = {"cg_tolerance": 1e-4, "point_layout": True, "mean_cg_warm_start": False}
    kw = dict(sigmasq=0.2, eps=1e-4, nufft_eps=1e-7, estimate_params=False, opts=opts)
    kern = lambda: SquaredExponential(dimension=2, init_lengthscale=0.2, init_variance=2.0)
    multi = EFGPNDMulti(x, Y, kern(), **kw)
    singles = [EFGPND(x, Y[:, b].contiguous(), kern(), **kw) for b in range(B)]
    keep = {}

    def multi_fit():
        multi.fit()
        keep["multi"] = multi.predict(x, return_variance=False)[0]

    def loop_fit():
        keep["loop"] = [m.fit().predict(x, return_variance=False)[0] for m in singles]

    def multi_grad():
        keep["g_multi"] = multi.compute_gradients(trace_samples=10, apply_gradients=False)

    def loop_grad():
        keep["g_loop"] = [m.compute_gradients(trace_samples=10, apply_gradients=False) for m in singles]

    def pair(fa, fb):
        for _ in range(2):                   # warm-up on the timed shapes: code objects, plans, layouts, pinned buffers
            fa()
            fb()
        ta, tb = [], []
        for _ in range(reps):                # alternating: both variants see the same neighbours on the machine
            t0 = sync()
            fa()
            t1 = sync()
            fb()
            t2 = sync()
            ta.append(1e3 * (t1 - t0))
            tb.append(1e3 * (t2 - t1))
        return [dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for t in (ta, tb)]

    row = {"N": N, "B": B, "reps": reps}
    row["fit_predict_multi"], row["fit_predict_loop"] = pair(multi_fit, loop_fit)
    loop_mean = torch.stack(keep["loop"], dim=1)
    st = multi.last_fit_stats
    its_multi = list(st["mean_cg_iters"])
    its_loop = [int(m.last_fit_stats["mean_cg_iters"]) for m in singles]
    # At this tolerance two stops one iteration apart are both valid fits and differ visibly: rows whose solve stopped at another
    # iteration than the single-output model's (a residual next to the threshold, rounding apart) are reported on their own
    same = torch.tensor([a == b for a, b in zip(its_multi, its_loop)], device=loop_mean.device)
    col = (keep["multi"] - loop_mean).abs().amax(dim=0) / loop_mean.abs().max()
    row["mean_difference_rel"] = float(col[same].max()) if bool(same.any()) else None
    row["rows_with_other_iteration_count"] = int((~same).sum())
    row["mean_difference_rel_of_those"] = float(col[~same].max()) if bool((~same).any()) else None
    row["shape"] = list(st["shape"])
    row["multi_cg_iters_max"] = max(its_multi)
    row["loop_cg_iters_max"] = max(its_loop)
    keep.clear()
    row["gradient_multi"], row["gradient_loop"] = pair(multi_grad, loop_grad)
    row["fit_predict_speedup"] = row["fit_predict_loop"]["median_ms"] / row["fit_predict_multi"]["median_ms"]
    row["gradient_speedup"] = row["gradient_loop"]["median_ms"] / row["gradient_multi"]["median_ms"]
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_output_mi355x.json"))
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--outputs", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a single (N, B) may take")
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "B"), help="measure one (N, B) in this process")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multi_output_bench.py needs a GPU: a CPU run says nothing about these timings")
    if args.one:
        return one(args.one[0], args.one[1], args.reps)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernel": "SE l=0.2 var=2 sigmasq=0.2 eps=1e-4",
           "nufft_eps": 1e-7, "cg_tolerance": 1e-4, "trace_samples": 10, "rows": []}
    for N in [int(float(s)) for s in args.sizes.split(",") if s]:
        for B in [int(s) for s in args.outputs.split(",") if s]:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", str(N), str(B),
                   "--reps", str(args.reps)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            rows = [ln[4:] for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not rows:
                print(out.stdout[-2000:], out.stderr[-4000:], sep="\n")
                raise SystemExit(f"N = {N}, B = {B} ended with status {out.returncode}: the sweep stops here")
            res["rows"].append(json.loads(rows[-1]))
            print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
