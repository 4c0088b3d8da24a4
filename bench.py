#!/usr/bin/env python3
"""Benchmark of the EFGP solve path on MI355X: GP-fits/s and CG-iter/s.

    python bench.py --gpus N --steps K --warmup W          (N > 1: one rank per GPU -- under torch.distributed.run as the
                                                            driver starts it, or started by bench.py itself when WORLD_SIZE is unset;
                                                            every rank checks WORLD_SIZE == N and exits non-zero otherwise)
    python bench.py ... --dump-outputs DIR                 (also writes the last timed step's posterior mean as DIR/mean.npy)
    python bench.py ... --full                             (the headline, then every other measurement of the record below)

A plain run sets up, warms up, times K steps and prints the headline keys (metric, value, unit, ms_per_step, dtype, config,
...).  Everything below beyond the headline -- the extra keys, `roofline` and the per-kernel timers, `cpu_baseline` -- is
measured with --full only.

Workload (BASELINE.json metric "GP-fits/sec + CG-iter/sec, N=1e6 d=2 SE kernel"; inputs as in the
reference's timing driver test_timing_profiling.py:18-44): x ~ U[-1,1]^2 (float64, seeded),
y = f(x) + N(0, 0.2); SE kernel l=0.2, sigma_f^2=2, sigma^2=0.2, eps=1e-4 (-> mtot=23, M=529,
Toeplitz FFT 64^2), NUFFT tol 1e-7, CG tol 1e-4 (the reference's default).

One step = one GP fit + posterior mean at the training points:
  grid construction (host) -> ONE fused spread pass over the points for (F*y, Toeplitz vector) ->
  accumulator -> modes (pruned transforms, no run-time compilation) -> Toeplitz setup -> Jacobi-PCG to tolerance -> type-2 interpolation at x.
Inputs are resident in HBM before the timed region.  With N GPUs the metric's GLOBAL problem (N = 1e6 points)
is sharded over the ranks (strong scaling: every rank holds N / n_gpus points, the gridded partial sums are
all-reduced over RCCL, CG is replicated) and `value` is the true fits/s of that global problem.  Extra keys:
`weak_scaling` (1e6 points PER rank, fits/s of the n_gpus x 1e6 problem) and `north_star_n1e7` (the
north_star's N = 1e7, d = 2 configuration: spread / gather / ordering microseconds per launch and their
fractions of the HBM peak; global N = 1e7 sharded over the ranks = BASELINE configs[3]), and -- N = 1 only --
`other_configs`: BASELINE configs[4] (3-D Matern-3/2, N = 5e6: first fit, refit, gradient step) and the hard case of
configs[3] (2-D, 256^2 circulant grid: fit, mean), configs[0] (1-D, N = 5000: fit, mean, stochastic variance) and configs[2]
(usa_temp Matern-5/2: fit, mean, stochastic J = 500 and regular variance) on data of their shape; `train_loop`: the metric's own
shape, test_timing_profiling.py:83-111 -- 50 Adam steps with MOVING hyper-parameters at N = 1e6; `scaling_model`: the replicated
share of the step from this run's timers and the speed-up ceiling it implies at 2 / 4 / 8 ranks.

The JSON line also carries `roofline` for the dominant N-scale kernel (the fused spread launch,
timed with HIP events on its launch stream inside the library) and `cpu_baseline` (the CPU oracle
of oracle/efgp_oracle.py timed on this box's host cores on a bounded sample, with 1 thread and with
all threads of the box's share; rank 0, N=1 only).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak (MI355X_MICROARCH.md)
N_PER_GPU = 1_000_000
DIM = 2
LS, VAR, SIG2, EPS = 0.2, 2.0, 0.2, 1e-4
NUFFT_TOL, CG_TOL = 1e-7, 1e-4
WARMUP_DEFAULT = 20            # + a floor of 0.5 s of warm-up steps when left at this value (see main)


def synth(N, d, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(N, d, dtype=torch.float64, generator=g) * 2 - 1
    f = (torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, 1])
         + 0.5 * torch.exp(-((x[:, 0] - 0.3) ** 2 + (x[:, 1] + 0.3) ** 2) / 0.3)
         + 0.7 * torch.sin(2 * math.pi * (x[:, 0] ** 2 + x[:, 1] ** 2)))
    y = f + torch.randn(N, dtype=torch.float64, generator=g) * math.sqrt(0.2)
    return x.to(device), y.to(device)


def cpu_baseline(seed):
    """CPU oracle (port of the reference algorithm, exact NUDFT) on a bounded sample: the full step with all threads
    of this box's share, and a 1-thread leg on a tenth of the points (SURVEY 8d asks for k in {1, all})."""
    from oracle import efgp_oracle as O
    # a one-GPU box owns a 16-core share of the host; more threads only oversubscribe it
    ncores = min(16, os.cpu_count() or 1)
    kern = O.KernelSpec("se", DIM, LS, VAR)

    def one(Ns, threads):
        torch.set_num_threads(threads)
        x, y = synth(Ns, DIM, seed, "cpu")
        t0 = time.perf_counter()
        fit = O.fit(x, y, kern, SIG2, EPS, cg_tol=CG_TOL)
        t1 = time.perf_counter()
        O.predict_mean(fit, x)
        t2 = time.perf_counter()
        A = O.make_A_mean(fit.ws, fit.T, SIG2)
        diag = O.jacobi_diag(fit.ws, SIG2, float(Ns))
        t3 = time.perf_counter()
        _, its = O.cg_single(A, fit.rhs, torch.zeros_like(fit.rhs), 1e-30, max_iter=200, diag=diag)
        t4 = time.perf_counter()
        return dict(fit_s=t1 - t0, mean_s=t2 - t1, iters=fit.iters, cg_iters_per_s=its / (t4 - t3))

    Ns = N_PER_GPU                  # the whole workload: the separable exact NUDFT takes a few seconds at N = 1e6
    full = one(Ns, ncores)
    n1 = Ns // 10
    single = one(n1, 1)
    torch.set_num_threads(ncores)
    return {
        "value": 1.0 / (full["fit_s"] + full["mean_s"]), "unit": "GP-fits/s (fit + mean at the N points, N=1e6)", "cores": ncores,
        "kind": "port",
        "sample": f"the full N={Ns} workload, same kernel/eps, one step: fit {full['fit_s']:.2f}s ({full['iters']} CG iterations) + mean "
                  f"at N points {full['mean_s']:.2f}s (exact-NUDFT oracle, torch CPU, {ncores} threads)",
        "cg_iters_per_s": full["cg_iters_per_s"],
        "one_thread": {"cores": 1, "sample": f"N={n1} (a tenth of the points), one step: fit {single['fit_s']:.2f}s + mean "
                                             f"{single['mean_s']:.2f}s",
                       "fits_per_s_scaled_to_n1e6": (n1 / Ns) / (single["fit_s"] + single["mean_s"]),
                       "cg_iters_per_s": single["cg_iters_per_s"]},
    }


def model_costs(dev, x, y):
    """What a model costs beyond the steady step (N = the headline's points, warm process): `one_shot_fit_ms` -- a NEW EFGPND +
    fit + posterior mean at the N points, the unit of the legacy efgp_nd() call (efgpnd_variance_shootout.py:129-137), which
    never builds the sorted point layout; `one_shot_fit_with_layout_ms` -- the same with the layout forced from the first fit;
    `layout_once_ms` -- their difference: bounding box, band keys, radix sort, two gathers, max|y|, paid once by a model at its
    second pass over the points."""
    from efgpnd import EFGPND
    from kernels.squared_exponential import SquaredExponential

    def one(layout):
        ts = []
        for _ in range(7):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            kern = SquaredExponential(dimension=DIM, init_lengthscale=LS, init_variance=VAR)
            m = EFGPND(x, y, kern, sigmasq=SIG2, eps=EPS, nufft_eps=NUFFT_TOL, estimate_params=False,
                       opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False, "point_layout": layout})
            m._compute_common_parameters()
            m.predict(x, return_variance=False)
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
            del m
        return 1e3 * sorted(ts)[len(ts) // 2]
    plain, forced = one("auto"), one(True)
    return {"one_shot_fit_ms": plain, "one_shot_fit_with_layout_ms": forced, "layout_once_ms": forced - plain}


def other_configs(dev):
    """BASELINE configs beyond the headline, one GPU, synthetic data of their shape (extras of the N=1 run, ~3 s):
    `configs4_3d_n5e6` -- configs[4]: 3-D Matern-3/2 (l = 0.2, eps 1e-3 -> mtot 57, 128^3 circulant grid), N = 5e6: first fit of
    the process for this model, forced refit (123 CG iterations), hyper-gradient step (Hutchinson trace, T = 2);
    `configs3_hard_2d_256sq` -- the hard case of configs[3]: 2-D SE l = 0.05 (mtot 71, 256^2 circulant grid), N = 1e6: fit and
    posterior mean at the N points."""
    from efgpnd import EFGPND
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(1e3 * (time.perf_counter() - t0))
        return sorted(ts)[len(ts) // 2]

    out = {}
    g = torch.Generator(device=dev).manual_seed(21)
    N3 = 5_000_000
    x = torch.rand(N3, 3, generator=g, dtype=torch.float64, device=dev) * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, 1]) * torch.cos(2 * x[:, 2]) + 0.3 * torch.randn(N3, generator=g, dtype=torch.float64, device=dev)
    m = EFGPND(x, y, Matern(dimension=3, nu=1.5, init_lengthscale=0.2, init_variance=1.5), sigmasq=0.2, eps=1e-3, nufft_eps=1e-6,
               estimate_params=False, opts={"cg_tolerance": 1e-5, "mean_cg_warm_start": False})
    first = timed(m.fit, 1)
    timed(m.fit, 1)
    refit = timed(m.fit, 3)
    M = m.last_fit_stats["feature_count"]
    V = torch.ones(2, M, dtype=torch.float64)
    V[1, ::2] = -1
    step = lambda: m.compute_gradients(trace_samples=2, cg_tol=1e-3, probe_seed=99, probes_V=V)    # noqa: E731
    timed(step, 1)
    grad = timed(step, 3)
    out["configs4_3d_n5e6"] = {"first_fit_ms": first, "refit_ms": refit, "gradient_step_ms_T2": grad, "mtot": int(m.last_fit_stats["mtot"]),
                               "mean_cg_iters": int(m.last_fit_stats["mean_cg_iters"])}
    del m, x, y
    x, y = synth(1_000_000, 2, 1000, dev)
    m = EFGPND(x, y, SquaredExponential(dimension=2, init_lengthscale=0.05, init_variance=2.0), sigmasq=0.2, eps=1e-4, nufft_eps=1e-7,
               estimate_params=False, opts={"cg_tolerance": 1e-4, "mean_cg_warm_start": False})
    fit = lambda: m._compute_common_parameters(force_recompute=True)      # noqa: E731
    mean = lambda: m.predict(x, return_variance=False)                     # noqa: E731
    for _ in range(3):
        fit()
        mean()
    out["configs3_hard_2d_256sq"] = {"fit_ms": timed(fit, 5), "mean_ms": timed(mean, 5), "mtot": int(m.last_fit_stats["mtot"]),
                                     "mean_cg_iters": int(m.last_fit_stats["mean_cg_iters"])}
    del m, x, y

    # configs[0]: 1-D SE, N = 5000 (the shape of data/gp_samples_5000_0.1_2_0.1.pt: l = 0.1, sigma_f^2 = 2, sigma^2 = 0.1), eps 1e-4:
    # fit, posterior mean at the N points, stochastic variance with J = 100 probes (efgpnd_basic_ex.ipynb:319-381)
    g1 = torch.Generator(device="cpu").manual_seed(5)
    x1 = (torch.rand(5000, 1, dtype=torch.float64, generator=g1) * 2 - 1)
    y1 = (torch.sin(3 * x1[:, 0]) + 0.5 * torch.exp(-((x1[:, 0] - 0.3) ** 2) / 0.3) + 0.7 * torch.sin(2 * math.pi * x1[:, 0] ** 2)
          + math.sqrt(0.1) * torch.randn(5000, dtype=torch.float64, generator=g1))
    x1, y1 = x1.to(dev), y1.to(dev)
    m = EFGPND(x1, y1, SquaredExponential(dimension=1, init_lengthscale=0.1, init_variance=2.0), sigmasq=0.1, eps=1e-4, nufft_eps=1e-7,
               estimate_params=False, opts={"cg_tolerance": 1e-4, "mean_cg_warm_start": False})
    fit = lambda: m._compute_common_parameters(force_recompute=True)      # noqa: E731
    mean = lambda: m.predict(x1, return_variance=False)                    # noqa: E731
    svar = lambda: m.predict(x1, variance_method="stochastic", hutchinson_probes=100)   # noqa: E731
    for _ in range(3):
        fit()
        mean()
    svar()
    out["configs0_1d_n5000"] = {"fit_ms": timed(fit, 7), "mean_ms": timed(mean, 7), "mean_plus_stochastic_variance_J100_ms": timed(svar, 5),
                                "mtot": int(m.last_fit_stats["mtot"]), "mean_cg_iters": int(m.last_fit_stats["mean_cg_iters"])}
    del m, x1, y1

    # configs[2]: 2-D Matern-5/2 on PRISM usa_temp (N = 4766), posterior mean + variance -- the shapes the reference publishes
    # timings for (efgpnd_ex.ipynb:662-663, 694: 500 Hutchinson probes 11.63 s, 'regular' variance 180.9 s on its CPU path).
    # Inputs: the normalised usa_temp points held by the parity fixture tests/golden/c3_matern52_usatemp.npz when it is there
    # (it travels with the repo), synthetic points of the same count otherwise.
    import numpy as np
    fx = os.path.join(ROOT, "tests", "golden", "c3_matern52_usatemp.npz")
    if os.path.exists(fx):
        gz = np.load(fx)
        x2, y2, src = torch.from_numpy(gz["x"]).to(dev), torch.from_numpy(gz["y"]).to(dev), "PRISM usa_temp (tests/golden/c3_matern52_usatemp.npz)"
    else:
        g2 = torch.Generator(device="cpu").manual_seed(6)
        x2 = torch.rand(4766, 2, dtype=torch.float64, generator=g2)
        y2 = (torch.sin(6 * x2[:, 0]) * torch.cos(5 * x2[:, 1]) + 0.2 * torch.randn(4766, dtype=torch.float64, generator=g2))
        x2, y2, src = x2.to(dev), y2.to(dev), "synthetic, N = 4766 in [0,1]^2"
    c2 = {"inputs": src}
    for eps2 in (1e-3, 1e-4):
        m = EFGPND(x2, y2, Matern(dimension=2, nu=2.5, init_lengthscale=0.1, init_variance=1.0), sigmasq=0.05, eps=eps2, nufft_eps=1e-7,
                   estimate_params=False, opts={"cg_tolerance": 1e-4, "mean_cg_warm_start": False})
        fit = lambda: m._compute_common_parameters(force_recompute=True)      # noqa: E731
        mean = lambda: m.predict(x2, return_variance=False)                    # noqa: E731
        svar = lambda: m.predict(x2, variance_method="stochastic", hutchinson_probes=500)   # noqa: E731
        rvar = lambda: m.predict(x2[:256], variance_method="regular")         # noqa: E731
        fit()
        mean()
        svar()
        rvar()
        c2[f"eps{eps2:g}"] = {"fit_ms": timed(fit, 5), "mean_ms": timed(mean, 5), "mean_plus_stochastic_variance_J500_ms": timed(svar, 3),
                              "mean_plus_regular_variance_256pts_ms": timed(rvar, 3), "mtot": int(m.last_fit_stats["mtot"]),
                              "mean_cg_iters": int(m.last_fit_stats["mean_cg_iters"]),
                              "circulant_grid": list(m._toeplitz.fft_shape)}
        del m
    out["configs2_usatemp_m52"] = c2
    return out


def train_loop(dev, x, y):
    """The loop the BASELINE metric is named after (test_timing_profiling.py:83-111): EFGPND(x, y, kernel='SquaredExponential',
    eps=1e-4) with the data heuristic for the initial hyper-parameters, Adam(lr=0.1), 50 steps; steps 0..40 with
    trace_samples=5, cg_tol=1e-3, the last 20 % with trace_samples=J=10 at the default tolerance; warm-started mean solves (the
    default).  The hyper-parameters MOVE: every step has a new grid spacing h, every few steps a new mode count mtot (new window
    polynomials, correction factors, circulant grid).  Every step is synchronised (optimizer.step() reads the gradient)."""
    from efgpnd import EFGPND
    from torch.optim import Adam
    builds = []
    for _ in range(2):                           # the first construction of a process loads torch's kernels for the heuristic
        torch.manual_seed(1234)                  # the heuristic draws a random subset (squared_exponential.py:192-195)
        torch.cuda.synchronize(dev)
        t_build = time.perf_counter()
        model = EFGPND(x, y, kernel="SquaredExponential", eps=1e-4)
        opt = Adam(model.parameters(), lr=0.1)
        torch.cuda.synchronize(dev)
        builds.append(1e3 * (time.perf_counter() - t_build))
    build_ms = builds[1]
    max_iters, J = 50, 10
    ms, mtots, iters = [], [], []
    t0 = time.perf_counter()
    for it in range(max_iters):
        t1 = time.perf_counter()
        opt.zero_grad()
        if it > max_iters * 0.8:
            model.compute_gradients(trace_samples=J)
        else:
            model.compute_gradients(trace_samples=5, cg_tol=1e-3)
        opt.step()
        torch.cuda.synchronize(dev)
        ms.append(1e3 * (time.perf_counter() - t1))
        st = model.last_gradient_stats
        mtots.append(int(st["mtot"]))
        iters.append(int(st["mean_cg_iters"]))
    total = time.perf_counter() - t0
    new_mtot = [i for i in range(1, max_iters) if mtots[i] != mtots[i - 1]]
    same = [ms[i] for i in range(1, 41) if mtots[i] == mtots[i - 1]]
    changed = [ms[i] for i in new_mtot]
    srt = sorted(ms)
    return {"steps": max_iters, "total_s": total, "steps_per_s": max_iters / total, "model_build_ms": build_ms,
            "model_build_first_in_process_ms": builds[0],
            "median_step_ms": srt[len(srt) // 2], "slowest_step_ms": srt[-1], "slowest_step_index": ms.index(srt[-1]),
            "first_step_ms": ms[0], "median_step_ms_T5_same_mtot": sorted(same)[len(same) // 2] if same else None,
            "median_step_ms_new_mtot": sorted(changed)[len(changed) // 2] if changed else None,
            "steps_with_new_mtot": len(new_mtot), "distinct_mtot": sorted(set(mtots)), "mtot_path": mtots,
            "mean_cg_iters_first_last": [iters[0], iters[-1]],
            "final_hypers": {"lengthscale": float(model.kernel.get_hyper("lengthscale")), "variance": float(model.kernel.get_hyper("variance")),
                             "sigmasq": float(model._gp_params.sig2.item())},
            "shape": "test_timing_profiling.py:83-111: N=1e6 d=2, kernel='SquaredExponential' eps=1e-4 estimated start, Adam lr=0.1, "
                     "50 steps: 41 x (T=5, cg_tol=1e-3) then 9 x (T=10, default tolerances), warm starts on, every step synchronised"}


def north_star(dev, rank, world, distributed, barrier):
    """The north_star configuration (N = 1e7, d = 2, SE): microseconds per launch of the N-scale kernels of one
    fit + mean step, HIP events inside the library.  `ordering_us` = per-step ordering passes (none: the point layout
    is built once per model, its cost is reported as `layout_once_ms`)."""
    from efgpnd import EFGPND
    from efgp_hip import kernel_timing, kernel_timing_read
    from kernels.squared_exponential import SquaredExponential
    NG = 10_000_000
    n_loc = NG // world + (1 if rank < NG % world else 0)
    x, y = synth(n_loc, DIM, 2000 + rank, dev)
    kern = SquaredExponential(dimension=DIM, init_lengthscale=LS, init_variance=VAR)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    model = EFGPND(x, y, kern, sigmasq=SIG2, eps=EPS, nufft_eps=NUFFT_TOL, estimate_params=False,
                   opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False, "shard_points": distributed})
    model._compute_common_parameters(force_recompute=True)
    model.predict(x, return_variance=False)
    torch.cuda.synchronize(dev)
    first_ms = 1e3 * (time.perf_counter() - t0)      # a model's first fit + mean: no sorted layout yet (built at its second pass)

    def step():
        model._compute_common_parameters(force_recompute=True)
        return model.predict(x, return_variance=False)[0]
    early = []
    for _ in range(3):                               # step 1 of these builds the layout; the later ones are steady
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize(dev)
        early.append(1e3 * (time.perf_counter() - t0))
    barrier()
    kernel_timing(True)
    reps = 10
    t1 = time.perf_counter()
    for _ in range(reps):
        step()
    barrier()
    el = time.perf_counter() - t1
    sp_ms, sp_n = kernel_timing_read("spread")
    ip_ms, ip_n = kernel_timing_read("interp")
    od_ms, od_n = kernel_timing_read("order")
    kernel_timing(False)
    if distributed:
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    spread_us = 1e3 * sp_ms / max(sp_n, 1)
    gather_us = 1e3 * ip_ms / max(ip_n, 1)
    order_us = 1e3 * od_ms / reps
    total_us = spread_us + gather_us + order_us
    survey_bytes = 3 * n_loc * (8 * DIM + 16)        # N(8d+16) per transform, two in the fused spread + one gather
    actual_bytes = 2 * n_loc * (8 * DIM + 8)         # x + real y read / x read + real mean written
    del model
    return {"global_n": NG, "n_per_gpu": n_loc, "ms_per_step": 1e3 * el / reps, "fits_per_s": reps / el,
            "spread_us": spread_us, "gather_us": gather_us, "ordering_us": order_us, "sum_us": total_us,
            "first_fit_ms": first_ms, "layout_once_ms": early[0] - min(early[1:]),
            "frac_hbm_survey_bytes": survey_bytes / (total_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "frac_hbm_actual_bytes": actual_bytes / (total_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "survey_bytes": survey_bytes, "actual_bytes": actual_bytes}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, mean, rank, world):
    """What a caller of the timed step receives: the posterior mean at this rank's training points, float64, as
    out_dir/mean.npy (mean_rank<r>.npy with several ranks).  Beyond 64 MB for the whole job a fixed stride sample is written."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    cap = DUMP_MAX_BYTES // (8 * world)
    stride = -(-mean.numel() // cap)
    name = "mean" if world == 1 else f"mean_rank{rank}"
    np.save(os.path.join(out_dir, name + ".npy"), mean.detach()[::stride].to(torch.float64).cpu().numpy())


def launch_ranks(n, argv):
    """One child process per GPU via torch.distributed.run on 127.0.0.1 (a free port), started BEFORE anything in this process
    touches the GPU; returns the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 200 timed steps of 0.3 ms behind 20 warm-up steps (60 ms in all) -- 20 steps behind 3 left the figure at the mercy of
    # one slow launch (0.277-0.302 ms from run to run on the same code)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=WARMUP_DEFAULT)
    ap.add_argument("--global-n", type=int, default=N_PER_GPU, help="points of the GLOBAL problem, sharded over the ranks")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the posterior mean of the last timed step as DIR/mean.npy (float64)")
    ap.add_argument("--full", action="store_true", help="after the headline, every other measurement of the record: fit-only time, "
                                                         "CG rates, gradient step, roofline and per-kernel timers, other configs, "
                                                         "train loop, weak scaling, north star, scaling model, CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the weak-scaling, north-star, mid-grid CG, "
                                                              "model-cost, other-config and train-loop legs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--check-launch", action="store_true", help="print this rank's place in the job and exit (no GPU needed): "
                                                                "checks the launcher and the WORLD_SIZE == --gpus rule")
    ap.add_argument("--main-only", action="store_true",
                    help="timed steps only (no CG-rate / gradient / CPU-baseline extras): for rocprofv3 --pmc passes, so "
                         "that every profiled launch belongs to the fit step")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: this process has not touched the GPU yet -- start the N ranks as children through
        # torch.distributed.run (one process per GPU, RCCL over xGMI) and leave with their exit code
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # a line that claims n_gpus = world while the caller asked for another count would be a wrong measurement
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    if args.check_launch:
        print(f"bench.py rank {rank} of {world} (local {local})", flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X GPU (no CPU fallback in the product path)")
    # stdout carries ONE line, the record: whatever the measured code prints on the way (the variance routines mirror the
    # reference's "Time to compute diag sums" messages, efgpnd.py:1664) goes to stderr
    record_out = sys.stdout
    sys.stdout = sys.stderr
    if torch.cuda.device_count() <= local:
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local} but this node shows {torch.cuda.device_count()} device(s)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    distributed = world > 1
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)

    import efgp_hip
    from efgpnd import EFGPND
    from efgp_hip import cg_solve, kernel_timing, kernel_timing_read
    from kernels.squared_exponential import SquaredExponential

    NG = args.global_n
    N = NG // world + (1 if rank < NG % world else 0)          # strong scaling: this rank's block of the global problem
    x, y = synth(N, DIM, 1000 + rank, dev)
    kern = SquaredExponential(dimension=DIM, init_lengthscale=LS, init_variance=VAR)
    model = EFGPND(x, y, kern, sigmasq=SIG2, eps=EPS, nufft_eps=NUFFT_TOL, estimate_params=False,
                   opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False, "shard_points": distributed})

    def step():
        model._compute_common_parameters(force_recompute=True)
        mean, _ = model.predict(x, return_variance=False)
        return mean

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # Warm-up: W steps, and when W was left at its default also at least 0.5 s of them.  A fresh process stalls two or three times for
    # 35-60 ms of HOST time during its first ~0.25 s of stepping (tools/r4/first_process_steps.py, cpu_burn_probe.py: `import torch`
    # alone burns 4 CPU-seconds in 0.8 s and gets the cgroup throttled; one-off runtime pool growth follows) -- with the device-bound
    # step at 0.28 ms a single such stall inside a 56-ms timed region reads as 0.46-0.53 ms per step.
    t_w = time.perf_counter()
    warm_done = 0
    # (several ranks: every step holds a collective, so all ranks must take the SAME number of steps -- a fixed 1500 instead of a clock)
    warm_steps = 1500 if (distributed and args.warmup == WARMUP_DEFAULT) else args.warmup
    while warm_done < warm_steps or (not distributed and args.warmup == WARMUP_DEFAULT and time.perf_counter() - t_w < 0.5):
        step()
        warm_done += 1
        if warm_done % 64 == 0:
            torch.cuda.synchronize(dev)             # the time floor is wall time of EXECUTED steps, not of enqueued ones
    barrier()
    # --full: inside the timed region only the roofline's kernel (the fused spread) carries HIP events: every timed launch puts
    # two event records into the stream, and with all timers on they cost the 0.3-ms step ~10 % (measured: 0.331 vs 0.291 ms)
    if args.full:
        kernel_timing(True, only="spread")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        mean = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, mean, rank, world)
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = 1e3 * elapsed / args.steps
    fits_per_s = args.steps / elapsed
    mean_iters = model.last_fit_stats["mean_cg_iters"]
    mtot = model.last_fit_stats["mtot"]

    def finish(rec):
        if rank == 0:
            print(json.dumps(rec), file=record_out, flush=True)
        if distributed:
            dist.barrier()
            dist.destroy_process_group()

    if args.main_only:
        finish({"metric": "GP-fits/sec (main-only profiling run)", "value": fits_per_s,
                "ms_per_step": ms_per_step, "steps": args.steps, "warmup": warm_done, "n_gpus": world})
        return
    headline = {
        "metric": "GP-fits/sec (fit + posterior mean at the N training points), N=1e6 d=2 SE kernel",
        "value": fits_per_s,
        "unit": "GP fits/s of the global N=1e6 problem (whole job; the points are sharded over the GPUs)",
        "n_gpus": world, "rccl_ranks": world if distributed else 0, "steps": args.steps, "warmup": warm_done,
        "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong",
        "scaling_note": "strong scaling of the metric's global N = 1e6: only the two N-scale launches shard; the mean solve (one "
                        "M-sized system, ~70 % of the one-GPU step) is replicated, so the curve is capped near 1.2 x at 8 GPUs by "
                        "construction (scaling_model, from the one-GPU timers); weak_scaling and north_star_n1e7 carry the cases "
                        "that gain",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "2D squared-exponential l=0.2 var=2 sigma2=0.2, eps=1e-4, global N=1e6 synthetic "
                               "(BASELINE configs[1] at the metric's N=1e6), points sharded over the GPUs",
                   "n_per_gpu": N, "global_n": NG, "d": DIM, "mtot": mtot, "M": mtot ** DIM,
                   "nufft_tol": NUFFT_TOL, "cg_tol": CG_TOL, "mean_cg_iters": mean_iters,
                   "parallelism": f"points sharded over {world} GPU(s), CG replicated"},
        "points_per_s": NG * fits_per_s,
    }
    if not args.full:
        finish(headline)
        return

    spread_ms, spread_n = kernel_timing_read("spread")
    kernel_timing(False)
    # gather and solve durations for the extra blocks: a second, untimed pass with all timers on
    kernel_timing(True)
    for _ in range(min(args.steps, 10)):
        step()
    barrier()
    interp_ms, interp_n = kernel_timing_read("interp")
    cgs_ms, cgs_n = kernel_timing_read("cg_solve")
    kernel_timing(False)

    # fit-only time and CG iteration rate (forced 200 iterations, no early stop), untimed region
    barrier()
    t1 = time.perf_counter()
    for _ in range(5):
        model._compute_common_parameters(force_recompute=True)
    torch.cuda.synchronize(dev)
    fit_only_ms = 1e3 * (time.perf_counter() - t1) / 5
    st = model._fit_state
    rhs = st["ws"] * st["Fy"]
    diag = (float(NG) * st["ws"].abs().pow(2).real + SIG2)
    # the model's own systems: rhs = D F*y of the real y, i.e. coefficients of real functions (hermitian=True, as the fit uses)
    cg_solve(model._toeplitz._op, st["ws"], SIG2, 0, rhs, torch.zeros_like(rhs), 1e-30, max_iter=50, diag=diag, batched=False,
             hermitian=True)
    cg_iter_per_s = 0.0
    for _ in range(3):       # 400 forced iterations are ~1.2 ms: one host hiccup moved a single sample by 20 % (2.92 -> 3.46 us) -- best of 3
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        _, its, _ = cg_solve(model._toeplitz._op, st["ws"], SIG2, 0, rhs, torch.zeros_like(rhs), 1e-300, max_iter=400,
                             early_stop=False, diag=diag, batched=False, hermitian=True)
        torch.cuda.synchronize(dev)
        cg_iter_per_s = max(cg_iter_per_s, its / (time.perf_counter() - t2))
    # batched rate: 64 independent right-hand sides
    B = 64
    rb = rhs[None, :].repeat(B, 1) * torch.linspace(0.5, 1.5, B, device=dev, dtype=torch.float64)[:, None]
    torch.cuda.synchronize(dev)
    t3 = time.perf_counter()
    _, itb, _ = cg_solve(model._toeplitz._op, st["ws"], SIG2, 0, rb, torch.zeros_like(rb), 1e-300, max_iter=200,
                         early_stop=False, diag=diag, batched=True, hermitian=True)
    torch.cuda.synchronize(dev)
    cg_rhs_iter_per_s = B * itb / (time.perf_counter() - t3)

    # one hyper-gradient step (the reference's training-loop unit, test_timing_profiling.py:94-111), T = 5 probes
    for _ in range(100):     # warm start, allocator, and the host's own first-use costs settle (2 steps left the median 40 us high)
        model.compute_gradients(trace_samples=5, cg_tol=1e-3)
    barrier()
    gts = []
    for _ in range(100):     # median of synchronised iterations: a single 10-ms host hiccup used to move a 10-iteration mean by 1 ms
        t4 = time.perf_counter()
        model.compute_gradients(trace_samples=5, cg_tol=1e-3)
        torch.cuda.synchronize(dev)
        gts.append(time.perf_counter() - t4)
    barrier()
    grad_step_ms = 1e3 * sorted(gts)[len(gts) // 2]

    # CG iteration time on the circulant grids beyond one CU (BASELINE configs[2], [3] solve on 128^2..512^2): one cooperative
    # launch per solve; synthetic Hermitian Toeplitz vector, 160 forced iterations, rank 0's GPU only.  The systems are what a
    # model's are -- right-hand side conjugate-even (the transform of real data), ws real and even -- and go through the
    # Hermitian kernel (cg_coop2d_herm_kernel, round 3); `cg_mid_general_us_per_iter`: the same systems through the general
    # complex kernel (cg_coop2d_kernel), which arbitrary right-hand sides (feature-space probes) take.
    cg_mid = None
    cg_mid_general = None
    if rank == 0 and not args.no_extras:
        from efgp_hip import ToeplitzOp
        cg_mid, cg_mid_general = {}, {}
        gm = torch.Generator().manual_seed(0)
        for mt in (41, 71, 131):
            L = 2 * mt - 1
            vv = torch.complex(torch.randn(L, L, generator=gm, dtype=torch.float64), torch.randn(L, L, generator=gm, dtype=torch.float64))
            vv = ((vv + vv.flip(0, 1).conj()) / 2).to(dev)
            wr = torch.rand(mt, mt, generator=gm, dtype=torch.float64)
            wsm = ((wr + wr.flip(0, 1)) / 2).reshape(-1).to(torch.complex128).to(dev)
            br = torch.complex(torch.randn(mt, mt, generator=gm, dtype=torch.float64), torch.randn(mt, mt, generator=gm, dtype=torch.float64))
            bm = ((br + br.flip(0, 1).conj()) / 2).reshape(-1).to(dev)
            dgm = (wsm.abs() ** 2 + 0.1).real
            opm = ToeplitzOp(vv)
            for herm, dst in ((True, cg_mid), (False, cg_mid_general)):
                for _ in range(2):
                    torch.cuda.synchronize(dev)
                    tm = time.perf_counter()
                    _, itm, _ = cg_solve(opm, wsm, 0.1, 0, bm, torch.zeros_like(bm), 1e-300, max_iter=160, early_stop=False, diag=dgm,
                                         batched=False, hermitian=herm)
                    torch.cuda.synchronize(dev)
                    dtm = time.perf_counter() - tm
                dst[f"{opm.fft_shape[0]}x{opm.fft_shape[1]}"] = 1e6 * dtm / itm
            del opm

    costs = model_costs(dev, x, y) if (world == 1 and rank == 0 and not args.no_extras) else None
    others = other_configs(dev) if (world == 1 and rank == 0 and not args.no_extras) else None
    loop = train_loop(dev, x, y) if (world == 1 and rank == 0 and not args.no_extras) else None
    # extra legs (every rank takes part: they contain collectives)
    weak = None
    star = None
    if not args.no_extras:
        if distributed:      # weak scaling: 1e6 points PER rank, fits/s of the n_gpus x 1e6 problem (at one GPU = the headline run)
            del model
            xw, yw = synth(N_PER_GPU, DIM, 3000 + rank, dev)
            mw = EFGPND(xw, yw, SquaredExponential(dimension=DIM, init_lengthscale=LS, init_variance=VAR), sigmasq=SIG2, eps=EPS,
                        nufft_eps=NUFFT_TOL, estimate_params=False,
                        opts={"cg_tolerance": CG_TOL, "mean_cg_warm_start": False, "shard_points": True})
            for _ in range(3):
                mw._compute_common_parameters(force_recompute=True)
                mw.predict(xw, return_variance=False)
            barrier()
            tw = time.perf_counter()
            for _ in range(args.steps):
                mw._compute_common_parameters(force_recompute=True)
                mw.predict(xw, return_variance=False)
            barrier()
            elw = torch.tensor([time.perf_counter() - tw], dtype=torch.float64, device=dev)
            dist.all_reduce(elw, op=dist.ReduceOp.MAX)
            weak = {"n_per_gpu": N_PER_GPU, "global_n": N_PER_GPU * world, "fits_per_s": args.steps / float(elw.item()),
                    "ms_per_step": 1e3 * float(elw.item()) / args.steps}
            del mw, xw, yw
        star = north_star(dev, rank, world, distributed, barrier)

    rec = None
    if rank == 0:
        m = (mtot - 1) // 2
        out_bytes = 16 * (mtot ** DIM + (4 * m + 1) ** DIM)
        spread_bytes = N * (8 * DIM + 8) + out_bytes                  # x + real y read once, two mode boxes written
        unfused_bytes = 2 * N * (8 * DIM + 16) + out_bytes           # two complex-strength type-1 passes
        spread_avg_s = (spread_ms / max(spread_n, 1)) * 1e-3
        achieved = spread_bytes / spread_avg_s / 1e9 if spread_n else None
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "r4_pmc_hbm_n1000000.json")
        if os.path.exists(tpath):
            try:
                traffic = json.load(open(tpath)).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        interp_bytes = N * (8 * DIM + 8) + 16 * mtot ** DIM          # real-only output
        ftot = 1
        for _ in range(DIM):
            ftot *= 1 << (4 * m + 1 - 1).bit_length()
        cg_bytes = 16 * (ftot + 8 * mtot ** DIM) * mean_iters        # fused-ideal bytes per iteration
        rec = dict(headline)
        rec.update({
            "fit_only_ms": fit_only_ms,
            "cg_iter_per_s": cg_iter_per_s,
            "cg_us_per_iter": 1e6 / cg_iter_per_s,
            "cg_rhs_iter_per_s_batch64": cg_rhs_iter_per_s,
            "gradient_step_ms_T5": grad_step_ms,
            "roofline": {"bound": "hbm", "kernel": "spread_mfma_kernel (fused F*y + Toeplitz-vector pass over the per-model sorted "
                                             "point layout, MFMA register tiles)",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic,
                         "traffic_source": "profiles/" + os.path.basename(tpath) + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
                                           "bench.py --main-only, committed; not measured in this run)" if traffic is not None else None,
                         "bytes_per_launch": spread_bytes, "avg_launch_us": spread_avg_s * 1e6, "launches": spread_n,
                         "achieved_vs_unfused_survey_figure": unfused_bytes / spread_avg_s / 1e9 if spread_n else None},
            "interp": {"avg_launch_us": 1e3 * interp_ms / max(interp_n, 1),
                       "achieved_GBs": interp_bytes / (1e-3 * interp_ms / max(interp_n, 1)) / 1e9 if interp_n else None},
            # the mean solve is ONE persistent launch (one CU): largest share of the step, latency/VALU bound by design,
            # priced here against the survey's per-iteration bytes 16*(F_tot + 8M) x the iterations of the launch
            "cg_solve": {"kernel": "cg_herm48_kernel (whole mean solve, one launch; real transforms on the 48 x 48 circulant grid)",
                         "avg_launch_us": 1e3 * cgs_ms / max(cgs_n, 1), "iterations": mean_iters,
                         "bytes_per_launch": cg_bytes,
                         "achieved_GBs": cg_bytes / (1e-3 * cgs_ms / max(cgs_n, 1)) / 1e9 if cgs_n else None,
                         "frac_hbm": cg_bytes / (1e-3 * cgs_ms / max(cgs_n, 1)) / 1e9 / HBM_PEAK_GBS if cgs_n else None,
                         "share_of_step": (cgs_ms / max(cgs_n, 1)) / ms_per_step if cgs_n else None},
        })
        if weak is not None:
            rec["weak_scaling"] = weak
        if star is not None:
            rec["north_star_n1e7"] = star
        if cg_mid is not None:
            rec["cg_mid_us_per_iter"] = cg_mid
            rec["cg_mid_general_us_per_iter"] = cg_mid_general
        if world == 1 and not args.no_extras:
            rec["model_costs"] = costs
            rec["other_configs"] = others
            rec["train_loop"] = loop
        if world == 1:
            # What more GPUs can and cannot do for this step, from THIS run's one-GPU timers (no multi-GPU hardware needed): the
            # N-scale launches (fused spread, gather) shard over the points; everything else -- the mean solve (one system,
            # replicated on every rank), the M-scale launches, host time -- does not.  ceiling(R) = step / (replicated +
            # n_scale / R); the all-reduce of the gridded partial sums (bytes below, one fused in-place RCCL call per fit) comes
            # ON TOP and is not in the ceiling.
            def amdahl(step_us, n_scale_us):
                repl = max(step_us - n_scale_us, 0.0)
                return {"step_us": step_us, "n_scale_us": n_scale_us, "replicated_us": repl, "replicated_share": repl / step_us,
                        "speedup_ceiling": {str(r): step_us / (repl + n_scale_us / r) for r in (2, 4, 8)}}
            sm = {"n1e6_headline": amdahl(1e3 * ms_per_step, 1e6 * spread_avg_s + 1e3 * interp_ms / max(interp_n, 1)),
                  "allreduce_bytes_per_fit": out_bytes,
                  "mean_solve": "replicated (one M-sized system; no collective inside the CG loop)",
                  "batched_solves": {"rows_sharded_in_this_workload": False,
                                     "rule": "the 2T trace systems of a gradient / the J Hutchinson systems of a variance are split by "
                                             "rows over the ranks when every rank gets a row (grids beyond one workgroup) or when there "
                                             "are more systems than CUs (64 x 64 grid); gathered by ONE all-reduce of rows x M x 16 bytes",
                                     "gradient_T5_rows": 10, "gradient_T5_allreduce_bytes_if_sharded": 10 * mtot ** DIM * 16},
                  "note": "strong scaling of the metric's global N = 1e6: the replicated mean solve caps the speedup; the sharded "
                          "share grows with N (north_star N = 1e7 below) and with the batched solves of configs[2] / configs[4]"}
            if star is not None:
                sm["n1e7_north_star"] = amdahl(1e3 * star["ms_per_step"], star["spread_us"] + star["gather_us"])
            rec["scaling_model"] = sm
        if world == 1 and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(1000)
    finish(rec)


if __name__ == "__main__":
    main()
