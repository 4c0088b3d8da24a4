"""Fitting from gridded observations: EFGPND.from_grid(...).fit() against EFGPND(meshgrid points, ...).fit(), and the raster
type-1 transform alone.

    python tools/raster_fit_bench.py [--out profiles/raster_fit_bench.txt] [--reps 7] [--only NAME]

One seeded synthetic raster per size (no data files).  Per size, in ONE process, after two warm-up rounds of every route:
  grid, refit     m.fit() of a gridded model that exists (axes, values and mask on the device)
  points, refit   m.fit() of a point model over the materialised observed cells whose sorted layout is cached
  grid, first     EFGPND.from_grid(axes, Y, mask=...).fit() from scratch
  points, first   building the (N, d) coordinate tensor of the observed cells on the device, EFGPND(points, y).fit() from scratch
  transform       efgp_hip.raster_type1 of the values onto the model's mode box alone, between two device events
The routes alternate inside the repetition loop, each between device synchronisations under a host clock; median, minimum and
maximum over the repetitions are reported.  No threshold is set: sizes where the point route wins stand as measured.  The GEMM's
bound comes from the shapes, not from counters: the raster read once at 6 TB/s, and its FMA count (2 Kpad_last per cell: a cos
and a sin column per padded mode) against 1024 SIMDs x 1024 FMA per 29.4 ns of v_mfma_f64_16x16x4_f64 (tools/mfma_f64_bench.hip).
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

MFMA_PEAK_FMA_PER_S = 1024 * 1024 / 29.4e-9
HBM_BYTES_PER_S = 6e12


def cases():
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    se = lambda: SquaredExponential(dimension=2, init_lengthscale=0.2, init_variance=2.0)
    return [
        ("se-2d-1024", se, (1024, 1024), 1e-4, 1e-7, 0.0),
        ("se-2d-4096", se, (4096, 4096), 1e-4, 1e-7, 0.0),
        ("matern-3d-256", lambda: Matern(dimension=3, nu=1.5, init_lengthscale=0.2, init_variance=1.5), (256, 256, 256), 1e-3, 1e-6, 0.0),
        ("se-2d-2048-masked", se, (2048, 2048), 1e-4, 1e-7, 0.3),
    ]


def synth(n_axis, masked, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    axes = [torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=dev) for n in n_axis]
    view = lambda a, i: a.reshape([-1 if j == i else 1 for j in range(len(n_axis))])
    Y = torch.sin(3 * view(axes[0], 0)) * torch.cos(4 * view(axes[-1], len(n_axis) - 1)) * torch.ones(n_axis, dtype=torch.float64, device=dev)
    Y = Y + math.sqrt(0.2) * torch.randn(n_axis, dtype=torch.float64, device=dev, generator=g)
    mask = None
    if masked > 0:
        mask = torch.rand(n_axis, device=dev, generator=g) >= masked
        mask.reshape(-1)[0] = mask.reshape(-1)[-1] = True            # the corners stay: one bounding box for both routes
    return axes, Y, mask


def spread(ts):
    return f"median {1e3 * statistics.median(ts):9.3f} ms  (min {1e3 * min(ts):9.3f}, max {1e3 * max(ts):9.3f}, n = {len(ts)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_fit_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raster_fit_bench needs a GPU: times are not taken on a CPU")
    from efgp_hip import ops
    from efgpnd import EFGPND
    dev = torch.device("cuda", 0)
    lines = [f"# tools/raster_fit_bench.py --reps {args.reps}; {torch.cuda.get_device_name(0)}; float64",
             "# grid: EFGPND.from_grid(...).fit(); points: EFGPND(observed meshgrid cells).fit(); transform: raster_type1 alone (device events)"]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    for name, kern, n_axis, eps, nufft_eps, masked in cases():
        if args.only and args.only != name:
            continue
        d = len(n_axis)
        axes, Y, mask = synth(n_axis, masked, dev)
        opts = {"cg_tolerance": 1e-4, "mean_cg_warm_start": False}
        common = dict(sigmasq=0.2, eps=eps, nufft_eps=nufft_eps, estimate_params=False, opts=opts)

        def points_of():
            pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, d)
            if mask is None:
                return pts, Y.reshape(-1)
            keep = mask.reshape(-1)
            return pts[keep], Y.reshape(-1)[keep]

        def grid_first():
            return EFGPND.from_grid(axes, Y, kern(), mask=mask, **common).fit()

        def points_first():
            x, y = points_of()
            return EFGPND(x, y, kern(), **common).fit()

        mg, mp = grid_first(), points_first()
        mp.fit()                                        # the second pass over the points builds the sorted layout
        st = mg._fit_state
        shape = tuple(st["shape"])
        assert tuple(mp._fit_state["shape"]) == shape
        scale = None if mask is None else mask.to(torch.float64)

        def transform():
            return ops.raster_type1(axes, st["plan_h"], shape, Y, cell_scale=scale)

        routes = [("grid, refit", mg.fit), ("points, refit", mp.fit), ("grid, first", grid_first), ("points, first", points_first)]
        for _ in range(2):
            for _, fn in routes:
                fn()
            transform()
        torch.cuda.synchronize(dev)
        N = mg._devdata["N"]
        e_fy = float((mg._fit_state["Fy"] - mp._fit_state["Fy"]).abs().max()) / float(Y.abs().sum() if mask is None else Y[mask].abs().sum())
        e_beta = float((mg._fit_state["beta"] - mp._fit_state["beta"]).abs().max() / mp._fit_state["beta"].abs().max())
        times = {label: [] for label, _ in routes}
        t_tr = []
        for _ in range(args.reps):
            for label, fn in routes:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize(dev)
                times[label].append(time.perf_counter() - t0)
                del out
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = transform()
            e1.record()
            torch.cuda.synchronize(dev)
            t_tr.append(1e-3 * e0.elapsed_time(e1))
            del out
        cells = math.prod(n_axis)
        kpad = -(-shape[-1] // 4) * 4
        gemm_fma, gemm_bytes = 2 * kpad * cells, 8 * cells * (1 if mask is None else 2)
        say()
        say(f"{name}: raster {n_axis} = {cells:,} cells, {N:,} observed, modes {shape}, nufft_eps {nufft_eps:g} (point route)")
        for label, _ in routes:
            say(f"  {label:14s} {spread(times[label])}")
        say(f"  transform      {spread(t_tr)}")
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"  points / grid = {med['points, refit'] / med['grid, refit']:.2f}x refit, {med['points, first'] / med['grid, first']:.2f}x first fit, at the medians; "
            f"coordinate tensor {8 * d * N / 1e6:.0f} MB")
        say(f"  max |Fy grid - Fy points| = {e_fy:.2e} sum|y|; max |beta grid - beta points| = {e_beta:.2e} max|beta|")
        say(f"  GEMM from the shapes: {gemm_bytes / 1e6:.0f} MB read = {1e6 * gemm_bytes / HBM_BYTES_PER_S:.1f} us at 6 TB/s; "
            f"{gemm_fma:.2e} FMA = {1e6 * gemm_fma / MFMA_PEAK_FMA_PER_S:.1f} us at {MFMA_PEAK_FMA_PER_S:.3e} FMA/s (f64 MFMA); "
            f"transform at {gemm_bytes / statistics.median(t_tr) / 1e9:.0f} GB/s, {gemm_fma / statistics.median(t_tr):.3e} FMA/s")
        del mg, mp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
