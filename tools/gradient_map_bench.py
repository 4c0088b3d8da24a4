"""What the posterior gradient costs next to the mean: the 2-D squared-exponential model of bench.py at N = 1e6.

    python tools/gradient_map_bench.py [--out profiles/gradient_map_bench.txt] [--reps 15] [--points 1000000] [--raster 1024]

Two pairs, each at the model's own tolerances, in ONE process:
  points   m.predict_gradient(x, return_variance=False, return_mean=True)  against  m.predict(x, return_variance=False)
           at the training points (the plan over them is cached by both: the pass over the points is what is timed)
  raster   m.predict_gradient_grid(axes, return_variance=False)            against  m.predict_grid(axes, return_variance=False)
           on a raster x raster map
After three warm-up rounds of every route the two routes of a pair alternate inside the repetition loop; a repetition is --calls
back-to-back calls between two device events on the current stream, the device idle before the first, divided by the calls;
median, minimum and maximum over the repetitions are reported, and the ratio of the medians.  What the pairing of real-only rows
predicts for the points: 1 + d rows ride ceil((1 + d) / 2) complex fine grids where the mean rides one, plus one elementwise launch
(efgp_mode_jet_rows); 1 + d separate predict calls would cost 1 + d.  Nothing is asserted.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gp-quadrature_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def spread(ts):
    return f"median {statistics.median(ts):9.3f} ms  (min {min(ts):9.3f}, max {max(ts):9.3f}, n = {len(ts)})"


def timed(fn, dev, calls):
    """Milliseconds per call of `calls` back-to-back calls between two device events."""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    del out
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradient_map_bench.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--raster", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gradient_map_bench needs a GPU: times are not taken on a CPU")
    import bench
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential
    dev = torch.device("cuda", 0)
    x, y = bench.synth(args.points, bench.DIM, 0, dev)
    m = EFGPND(x, y, SquaredExponential(dimension=bench.DIM, init_lengthscale=bench.LS, init_variance=bench.VAR), sigmasq=bench.SIG2,
               eps=bench.EPS, nufft_eps=bench.NUFFT_TOL, estimate_params=False, opts={"cg_tolerance": bench.CG_TOL})
    m.fit()
    d, shape = bench.DIM, tuple(m._fit_state["shape"])
    axes = [torch.linspace(-1.0, 1.0, args.raster, dtype=torch.float64, device=dev) for _ in range(d)]
    pairs = [
        ("points", f"N = {args.points:,} training points",
         lambda: m.predict(x, return_variance=False), lambda: m.predict_gradient(x, return_variance=False, return_mean=True)),
        ("raster", f"{args.raster} x {args.raster} map",
         lambda: m.predict_grid(axes, return_variance=False), lambda: m.predict_gradient_grid(axes, return_variance=False)),
    ]
    lines = [f"# tools/gradient_map_bench.py --reps {args.reps} --calls {args.calls} --points {args.points} --raster {args.raster}; "
             f"{torch.cuda.get_device_name(0)}; float64; modes {shape}; nufft_eps {bench.NUFFT_TOL:g}",
             "# ms per call: device events around --calls back-to-back calls, device idle before; 3 warm-up rounds; the routes of a pair alternate"]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for name, what, value, jet in pairs:
        for _ in range(3):
            value(), jet()
        t_value, t_jet = [], []
        for _ in range(args.reps):
            t_value.append(timed(value, dev, args.calls))
            t_jet.append(timed(jet, dev, args.calls))
        ratio = statistics.median(t_jet) / statistics.median(t_value)
        say()
        say(f"{name}: {what}")
        say(f"  value               {spread(t_value)}")
        say(f"  value and gradient  {spread(t_jet)}")
        say(f"  ratio of the medians {ratio:.2f}  (pairing: at most ceil((1 + d) / 2) = {math.ceil((1 + d) / 2)} fine grids plus one "
            f"elementwise launch; {1 + d} separate calls: {1 + d})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
