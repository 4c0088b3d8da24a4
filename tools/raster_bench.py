"""Maps on rectilinear grids: EFGPND.predict_grid against predict on the materialised meshgrid, and the raster transform alone.

    python tools/raster_bench.py [--out profiles/raster_bench.txt] [--reps 7] [--points 200000] [--only NAME]

One seeded synthetic model per size (no data files).  Per size, in ONE process, after two warm-up rounds of every route:
  grid      m.predict_grid(axes, return_variance=False)
  points    building the (prod n, d) coordinate tensor on the device (meshgrid + stack), the plan over it and
            m.predict(points, return_variance=False) -- what a map costs without predict_grid (unchanged code)
  transform efgp_hip.raster_type2 alone (tables, contractions and the GEMM), between two device events
The two routes alternate inside the repetition loop, each between device synchronisations under a host clock; median, minimum
and maximum over the repetitions are reported.  The operation counts come from the shapes (below), not from counters:
FMA/s is the transform's FMA count over its event time, set against 1024 SIMDs x 1024 FMA per 29.4 ns of v_mfma_f64_16x16x4_f64
(tools/mfma_f64_bench.hip); bytes/s is the output alone (8 B per cell) over the same time.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gp-quadrature_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

MFMA_PEAK_FMA_PER_S = 1024 * 1024 / 29.4e-9       # 1024 SIMDs, one 16x16x4 f64 instruction (1024 FMA) per 29.4 ns each


def counts(shape, n_axis, nbatch=1):
    """Per kernel of the transform: (name, real FMAs, bytes written), from the shapes alone."""
    d = len(shape)
    kpad = [-(-m // 4) * 4 for m in shape]
    rows = [("tables", 0, sum(16 * n * k for n, k in zip(n_axis, kpad)))]
    if d == 1:
        rows.append(("pack", 4 * nbatch * shape[0], 16 * nbatch * kpad[0]))
        rows.append(("gemm", 2 * kpad[0] * nbatch * n_axis[0], 8 * nbatch * n_axis[0]))
    elif d == 2:
        rows.append(("contract axis 0", 4 * nbatch * n_axis[0] * shape[0] * shape[1], 16 * nbatch * n_axis[0] * kpad[1]))
        rows.append(("gemm", 2 * kpad[1] * nbatch * n_axis[0] * n_axis[1], 8 * nbatch * n_axis[0] * n_axis[1]))
    else:
        rows.append(("contract axis 0", 4 * nbatch * n_axis[0] * math.prod(shape), 16 * nbatch * n_axis[0] * shape[1] * shape[2]))
        rows.append(("contract axis 1", 4 * nbatch * n_axis[0] * n_axis[1] * shape[1] * shape[2], 16 * nbatch * n_axis[0] * n_axis[1] * kpad[2]))
        rows.append(("gemm", 2 * kpad[2] * nbatch * math.prod(n_axis), 8 * nbatch * math.prod(n_axis)))
    return rows


def synth(N, d, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, d, dtype=torch.float64, generator=g) * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, -1]) + math.sqrt(0.2) * torch.randn(N, dtype=torch.float64, generator=g)
    return x.to(dev), y.to(dev)


def models():
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    return {
        "headline-2d": (lambda: SquaredExponential(dimension=2, init_lengthscale=0.2, init_variance=2.0), 2, 1e-4, 1e-7, [(1024, 1024), (4096, 4096)]),
        "fine-2d": (lambda: SquaredExponential(dimension=2, init_lengthscale=0.02, init_variance=2.0), 2, 1e-4, 1e-7, [(2048, 2048)]),
        "matern-3d": (lambda: Matern(dimension=3, nu=1.5, init_lengthscale=0.2, init_variance=1.5), 3, 1e-3, 1e-6, [(256, 256, 256)]),
    }


def spread(ts):
    return f"median {1e3 * statistics.median(ts):9.3f} ms  (min {1e3 * min(ts):9.3f}, max {1e3 * max(ts):9.3f}, n = {len(ts)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raster_bench needs a GPU: times are not taken on a CPU")
    from efgp_hip import ops
    from efgpnd import EFGPND
    dev = torch.device("cuda", 0)
    lines = [f"# tools/raster_bench.py --reps {args.reps} --points {args.points}; {torch.cuda.get_device_name(0)}; float64",
             "# grid: predict_grid(axes); points: meshgrid tensor + plan + predict; transform: raster_type2 alone (device events)"]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for name, (kern, d, eps, nufft_eps, rasters) in models().items():
        if args.only and args.only != name:
            continue
        x, y = synth(args.points, d, 11, dev)
        m = EFGPND(x, y, kern(), sigmasq=0.2, eps=eps, nufft_eps=nufft_eps, estimate_params=False, opts={"cg_tolerance": 1e-4})
        m.fit()
        st = m._fit_state
        shape = tuple(st["shape"])
        for n_axis in rasters:
            axes = [torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=dev) for n in n_axis]

            def route_grid():
                return m.predict_grid(axes, return_variance=False)[0]

            def route_points():
                m._predict_plan = None               # a new map is a new point set: its plan is part of the cost
                pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, d)
                return m.predict(pts, return_variance=False)[0]

            def route_transform():
                return ops.raster_type2(axes, st["plan_h"], shape, st["beta"], mode_scale=st["ws"])

            for _ in range(2):
                a, b, _c = route_grid(), route_points(), route_transform()
            torch.cuda.synchronize(dev)
            mag = float((st["ws"] * st["beta"]).abs().sum())
            diff = float((a.reshape(-1) - b).abs().max()) / mag
            del a, b, _c
            t_grid, t_pts, t_tr = [], [], []
            for _ in range(args.reps):
                for fn, acc in ((route_grid, t_grid), (route_points, t_pts)):
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize(dev)
                    acc.append(time.perf_counter() - t0)
                    del out
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = route_transform()
                e1.record()
                torch.cuda.synchronize(dev)
                t_tr.append(1e-3 * e0.elapsed_time(e1))
                del out
            rows = counts(shape, n_axis)
            fma, out_bytes = sum(r[1] for r in rows), 8 * math.prod(n_axis)
            tt = statistics.median(t_tr)
            say()
            say(f"{name}: modes {shape}, raster {n_axis} = {math.prod(n_axis):,} cells, model of N = {args.points}, nufft_eps {nufft_eps:g}")
            say(f"  grid      {spread(t_grid)}")
            say(f"  points    {spread(t_pts)}   coordinate tensor {8 * d * math.prod(n_axis) / 1e6:.0f} MB")
            say(f"  transform {spread(t_tr)}")
            say(f"  points / grid = {statistics.median(t_pts) / statistics.median(t_grid):.2f}x at the medians; max |grid - points| = {diff:.2e} sum |ws beta|")
            for kname, f, wbytes in rows:
                say(f"    {kname:16s} {f:>16,} FMA  {wbytes:>14,} B written")
            say(f"  transform: {fma / tt:.3e} FMA/s = {100 * fma / tt / MFMA_PEAK_FMA_PER_S:.1f} % of {MFMA_PEAK_FMA_PER_S:.3e} (f64 MFMA); "
                f"output {out_bytes / tt / 1e9:.1f} GB/s")
        del m, x, y
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
