#!/usr/bin/env python3
"""Timings of the isotropic and the ARD model on a 2.3 : 1 box on one GPU (record only: nothing here is a requirement):

    python tools/ard_bench.py [--out FILE] [--n 1000000] [--new 100000] [--reps 7]

SE kernel, N points uniform in [0, 2.3] x [0, 1], fixed hyper-parameters, eps = 1e-4, NUFFT tolerance 1e-7, CG tolerance 1e-4,
point layout on, no warm start.  Three models:
  isotropic   SquaredExponential(l): one spacing and one mode count, sized for the long side of the box;
  ard_equal   SquaredExponentialARD(l, l): the same kernel on the per-axis grid -- the short axis gets its own, smaller block;
  ard         SquaredExponentialARD(l, 2.5 l): a longer lengthscale on the short axis.
Per model: the mode block, the CG route (tests/_cg_routes.py restates the library's dispatch) and iteration count, and the time of
fit + posterior mean at --new points: host clock around work that ends in a device synchronisation, two warm-up calls, the median
of --reps and the spread, the models taken in turn within every repetition.  The fit of every repetition is forced.

Every model is also held to a dense restatement at this N (--no-check skips it): F*y and the Toeplitz vector as exact sums over all
N points (tests/_nudft.py, float64 on the CPU), the M x M system solved by LAPACK, the mean at 2000 of the new points by exact
sums; the model is refitted with CG tolerance 1e-10 for that comparison, and the timed model (CG tolerance 1e-4) is compared with
the same restatement.  At this N the plans run the point-layout (MFMA) spreader and the large-N gathers, with a spacing per axis for
the two ARD models.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--new", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lengthscale", type=float, default=0.1)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ard_bench.py measures on a GPU; none is visible")
    import _cg_routes as R
    from efgpnd import EFGPND
    from kernels import SquaredExponential, SquaredExponentialARD

    N, ell = args.n, args.lengthscale
    g = torch.Generator(device="cuda").manual_seed(3)
    box = torch.tensor([2.3, 1.0], dtype=torch.float64, device="cuda")
    x = torch.rand(N, 2, generator=g, dtype=torch.float64, device="cuda") * box
    y = torch.sin(5 * x[:, 0]) * torch.cos(3 * x[:, 1]) + 0.3 * torch.randn(N, generator=g, dtype=torch.float64, device="cuda")
    xn = torch.rand(args.new, 2, generator=g, dtype=torch.float64, device="cuda") * box
    kernels = {
        "isotropic": SquaredExponential(dimension=2, init_lengthscale=ell, init_variance=1.0),
        "ard_equal": SquaredExponentialARD(dimension=2, init_lengthscale=(ell, ell), init_variance=1.0),
        "ard": SquaredExponentialARD(dimension=2, init_lengthscale=(ell, 2.5 * ell), init_variance=1.0),
    }
    models = {name: EFGPND(x, y, k, sigmasq=0.09, eps=1e-4, nufft_eps=1e-7, estimate_params=False,
                           opts={"cg_tolerance": 1e-4, "mean_cg_warm_start": False, "point_layout": True})
              for name, k in kernels.items()}

    def step(m):
        m.fit(force_recompute=True)
        return m.predict(xn, return_variance=False)[0]

    means = {}
    for name, m in models.items():                       # warm-up: code objects, the sorted layout, the plans' window tables
        for _ in range(2):
            means[name] = step(m)
    times = {name: [] for name in models}
    for _ in range(args.reps):
        for name, m in models.items():
            t0 = sync()
            step(m)
            times[name].append(1e3 * (sync() - t0))
    rows = []
    for name, m in models.items():
        st = m._fit_state
        shape = tuple(st["shape"])
        kern, grid = R.route(shape, True)
        rows.append({"model": name, "lengthscales": [float(v) for v in (m.kernel.lengthscales if st["ard"] else (ell,))],
                     "block": list(shape), "modes": int(st["ws"].numel()), "hs": [float(v) for v in st["hs"]],
                     "cg_route": kern, "cg_grid": list(grid), "cg_iters": int(m.last_fit_stats["mean_cg_iters"]),
                     "fit_plus_mean_ms_median": statistics.median(times[name]), "fit_plus_mean_ms_min": min(times[name]),
                     "fit_plus_mean_ms_max": max(times[name])})
    if not args.no_check:
        import _nudft as E
        xc, yc, xs = x.cpu(), y.cpu(), xn[:2000].cpu()
        for r, (name, m) in zip(rows, models.items()):
            st = m._fit_state
            shape, hs = tuple(st["shape"]), torch.tensor(st["hs"], dtype=torch.float64)
            ws = st["ws"].real.cpu()
            Fy = E.type1(xc * hs, 1.0, yc, shape).reshape(-1)
            v = E.type1(xc * hs, 1.0, torch.ones(N, dtype=torch.float64), tuple(2 * n - 1 for n in shape))
            k0 = torch.cartesian_prod(*[torch.arange(n) for n in shape]).reshape(-1, 2)
            lag = k0[:, None, :] - k0[None, :, :] + torch.tensor([n - 1 for n in shape])
            T = v[lag[..., 0], lag[..., 1]]                                   # T[k, l] = v[k - l]
            A = ws[:, None] * T * ws[None, :] + st["sig"] * torch.eye(ws.numel(), dtype=torch.complex128)
            beta = torch.linalg.solve(A, (ws * Fy).to(torch.complex128))
            ref = E.type2(xs * hs, 1.0, ws * beta, shape).real
            timed = means[name][:2000].cpu()
            tight = EFGPND(x, y, kernels[name], sigmasq=0.09, eps=1e-4, nufft_eps=1e-7, estimate_params=False,
                           opts={"cg_tolerance": 1e-10, "mean_cg_warm_start": False, "point_layout": True})
            for _ in range(2):                                                # the second pass runs on the sorted layout
                tight.fit(force_recompute=True)
            got = tight.predict(xn[:2000], return_variance=False)[0].cpu()
            r["mean_vs_restatement_cg1e-10"] = float((got - ref).abs().max() / ref.abs().max())
            r["mean_vs_restatement_cg1e-4"] = float((timed - ref).abs().max() / ref.abs().max())
            r["tight_cg_iters"] = int(tight.last_fit_stats["mean_cg_iters"])
            r["restatement_cond"] = float(torch.linalg.cond(A))
    # same kernel, two grids: the means differ by the two quadratures' errors (amplified by N / sigma^2) and the CG truncation
    dm = float((means["ard_equal"] - means["isotropic"]).abs().max() / means["isotropic"].abs().max())
    out = {"N": N, "new_points": args.new, "box": [2.3, 1.0], "eps": 1e-4, "reps": args.reps, "rows": rows,
           "ard_equal_vs_isotropic_mean_rel": dm, "device": torch.cuda.get_device_name(0)}
    print(f"{'model':10} {'block':>10} {'modes':>6} {'route':>10} {'iters':>5} {'fit+mean ms (median, min..max)':>34}")
    for r in rows:
        print(f"{r['model']:10} {str(tuple(r['block'])):>10} {r['modes']:6d} {r['cg_route']:>10} {r['cg_iters']:5d} "
              f"{r['fit_plus_mean_ms_median']:12.3f} {r['fit_plus_mean_ms_min']:9.3f}..{r['fit_plus_mean_ms_max']:.3f}")
    if not args.no_check:
        for r in rows:
            print(f"{r['model']:10} mean against the dense restatement at N = {N}: {r['mean_vs_restatement_cg1e-10']:.2e} with CG tolerance "
                  f"1e-10 ({r['tight_cg_iters']} iterations), {r['mean_vs_restatement_cg1e-4']:.2e} as timed (1e-4); cond {r['restatement_cond']:.2e}")
    print(f"ard_equal against isotropic, posterior mean at the new points: {dm:.2e} (two grids for one kernel, eps 1e-4, CG 1e-4)")
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
