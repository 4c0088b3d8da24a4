#!/usr/bin/env python3
"""Timings of GP path sampling on one GPU (record only, nothing asserted):

    python tools/sample_bench.py [--out FILE] [--sizes 1000000,10000000] [--draws 64] [--reps 5]

For d = 2, the SE kernel and the headline grid (l = 0.2, eps = 1e-4: 23 x 23 modes, NUFFT tolerance 1e-7, CG tolerance 1e-4)
and S draws at the N training points of each size:
  (a) fused:    EFGPND.sample_paths -- noise generated inside the spreader (NufftPlan.type1_normal), right-hand sides by
                efgp_hermitian_normal_rows, one batched Hermitian CG, one batched type 2;
  (b) composed: the same draws from what the library offered before: torch.randn(S, N) through NufftPlan.type1, right-hand sides
                in torch, cg_solve, type2.
Per variant: the whole call (host clock around work that ends in a device synchronisation, warmed up, median of --reps) and
every stage on its own (closed by a synchronisation), per draw; CG iterations; peak device memory of torch's allocator above the
resident model (the library's own scratch pool -- fine grids, accumulators -- is not in that figure: it is the same pool in both
variants, sized by S / 2 fine grids).  Plus the fused type 1 against type1_rademacher and against type1 on materialised rows of
the same count (the cost of the normals alone), at the headline's MFMA spreader and, on plans of their own, on the LDS and
tile-sorted spreaders in 2-D and 3-D (`other_spread_paths`).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gp-quadrature_amd"))

import torch  # noqa: E402


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed(fn, reps, warmup=2):
    """Median wall time in ms of fn() (its work ends in a synchronisation), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    sync()
    rows = []
    for _ in range(reps):
        t0 = sync()
        fn()
        rows.append(1e3 * (sync() - t0))
    return statistics.median(rows), min(rows), max(rows)


def peak_of(fn):
    sync()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    sync()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_size(N, S, reps):
    from efgp_hip import cg_solve, gradient_prepare, hermitian_normal_rows
    from efgpnd import EFGPND, _SAMPLE_BLOCK, _center_flat, _derive_seed
    from kernels.squared_exponential import SquaredExponential
    g = torch.Generator(device="cuda").manual_seed(N % 97)
    x = torch.rand(N, 2, generator=g, dtype=torch.float64, device="cuda") * 2 - 1
    y = torch.sin(3 * x[:, 0]) * torch.cos(4 * x[:, 1]) + math.sqrt(0.2) * torch.randn(N, generator=g, dtype=torch.float64, device="cuda")
    kern = SquaredExponential(dimension=2, init_lengthscale=0.2, init_variance=2.0)
    m = EFGPND(x, y, kern, sigmasq=0.2, eps=1e-4, nufft_eps=1e-7, estimate_params=False,
               opts={"cg_tolerance": 1e-4, "mean_cg_warm_start": False, "point_layout": True, "max_cg_iterations": 20000})
    m.fit()
    st = m._fit_state
    dev = x.device
    M, shape, sig, ws = st["ws"].numel(), (st["mtot"],) * 2, st["sig"], st["ws"]
    tol, max_iter = m.opts["cg_tolerance"], m.opts.get("max_cg_iterations", 1000)
    seed = 12345
    row = {"N": N, "draws": S, "mtot": st["mtot"], "block": _SAMPLE_BLOCK[2], "fit_cg_iters": int(m.last_fit_stats["mean_cg_iters"]),
           "cond_A": float(N * (ws.abs() ** 2).max() / sig + 1.0)}

    # (a) fused, the whole call
    med, lo, hi = timed(lambda: m.sample_paths(x, S, seed=seed), reps)
    row["fused_total_ms_per_draw"] = med / S
    row["fused_total_ms_spread"] = [lo / S, hi / S]
    its = m.last_sample_stats["cg_iters"]
    row["fused_cg_iters"] = {"min": min(its), "median": statistics.median(its), "max": max(its)}
    row["fused_peak_torch_mib"] = peak_of(lambda: m.sample_paths(x, S, seed=seed))
    row["output_mib"] = S * N * 8 / 2 ** 20

    # (a) by stage (one block of rows at a time, as sample_paths does)
    plan_x = m._sample_plan[1]
    plan_new = m._predict_plan[1]
    cidx = _center_flat(st["v"])
    diag, _ = gradient_prepare(ws, None, st["v"].reshape(-1)[cidx:cidx + 1], sig, want_diag=True, want_rhs=False)
    block = _SAMPLE_BLOCK[2]
    nb = min(block, S)
    nblocks = -(-S // block)
    s1, s2 = _derive_seed(seed, 1), _derive_seed(seed, 2)
    keep = {}

    def a_type1():
        keep["fz"] = plan_x.type1_normal(s1, nb, shape).reshape(nb, M)

    def a_rhs():
        keep["rhs"] = hermitian_normal_rows(dev, s2, nb, M, a=math.sqrt(sig), ws=ws, fz=keep["fz"], b=sig)

    def a_cg():
        keep["delta"], _, keep["rows"] = cg_solve(m._toeplitz._op, ws, sig, 0, keep["rhs"], None, tol, max_iter=max_iter, early_stop=True,
                                                  diag=diag, batched=True, hermitian=True)

    def a_type2():
        keep["f"] = plan_new.type2(keep["delta"].reshape(nb, M) + st["beta"].reshape(1, M), shape, real_only=True, batched=True,
                                   mode_scale=ws)
    for name, fn in (("type1_normal", a_type1), ("rhs_kernel", a_rhs), ("cg", a_cg), ("type2", a_type2)):
        row[f"fused_{name}_ms_per_draw"] = timed(fn, reps)[0] / nb

    # the normals alone: the fused type 1 against Rademacher rows and against materialised rows of the same count
    row["type1_rademacher_ms_per_draw"] = timed(lambda: plan_x.type1_rademacher(s1, nb, shape), reps)[0] / nb
    Z = torch.randn(nb, N, dtype=torch.float64, device=dev)
    row["type1_materialised_ms_per_draw"] = timed(lambda: plan_x.type1(Z, shape), reps)[0] / nb
    del Z

    # (b) composed from the earlier interface, block by block like (a)
    def b_randn():
        keep["e1"] = torch.randn(nb, N, dtype=torch.float64, device=dev)

    def b_type1():
        keep["fz"] = plan_x.type1(keep["e1"], shape).reshape(nb, M)

    def b_rhs():
        p, q = torch.randn(nb, M, dtype=torch.float64, device=dev), torch.randn(nb, M, dtype=torch.float64, device=dev)
        e = torch.complex(p, q) / math.sqrt(2.0)
        e = 0.5 * (e + e.flip(1).conj()) * math.sqrt(2.0)
        c = (M - 1) // 2
        e[:, c] = torch.complex(p[:, c], torch.zeros_like(p[:, c]))
        keep["rhs"] = math.sqrt(sig) * ws.reshape(1, M) * keep["fz"] + sig * e

    def b_all():
        outs, its = [], []
        for r0 in range(0, S, block):
            b_randn()
            b_type1()
            b_rhs()
            a_cg()
            a_type2()
            its += list(keep["rows"])
            outs.append(keep["f"])
        keep["b_iters"] = its
        return outs[0] if len(outs) == 1 else torch.cat(outs)
    if S % block == 0 or S < block:
        med, lo, hi = timed(b_all, reps)
        row["composed_total_ms_per_draw"] = med / S
        row["composed_total_ms_spread"] = [lo / S, hi / S]
        its = [int(v) for v in keep["b_iters"]]
        row["composed_cg_iters"] = {"min": min(its), "median": statistics.median(its), "max": max(its)}
        keep.clear()
        row["composed_peak_torch_mib"] = peak_of(b_all)
        b_all()                                  # the stage timings below reuse what a pass leaves in `keep`
    for name, fn in (("randn", b_randn), ("type1", b_type1), ("rhs_torch", b_rhs), ("cg", a_cg), ("type2", a_type2)):
        row[f"composed_{name}_ms_per_draw"] = timed(fn, reps)[0] / nb
    row["blocks"] = nblocks
    return row


def bench_other_paths(reps, T=8):
    """Type 1 of T generated normal rows against T Rademacher rows and T rows read from memory on the spread paths the headline
    does not take: plans without a layout (padded LDS spreader), a 2-D window wide enough for the generator to spill there, and
    the 3-D LDS and tile-sorted spreaders.  ms per row."""
    from efgp_hip import NufftPlan, lib
    rows = []
    for name, d, N, h, nm, tol in (("2-D plain plan, LDS padded rows", 2, 1_000_000, 0.346, 23, 1e-7),
                                   ("2-D plain plan, LDS padded rows, wide window", 2, 1_000_000, 0.346, 23, 1e-11),
                                   ("3-D, fine grid in LDS", 3, 1_000_000, 0.3, 9, 1e-6),
                                   ("3-D, tile-sorted spreader", 3, 5_000_000, 0.2, 57, 1e-6)):
        g = torch.Generator(device="cuda").manual_seed(d + nm)
        x = torch.rand(N, d, generator=g, dtype=torch.float64, device="cuda") * 2 - 1
        plan = NufftPlan(x, h, tol)
        shape = (nm,) * d
        Z = torch.randn(T, N, dtype=torch.float64, device="cuda")
        row = {"path": name, "d": d, "N": N, "modes": nm, "tol": tol, "rows": T, "window_width_at_ratio_2": int(lib().efgp_window_width(tol, 2.0))}
        row["type1_normal_ms_per_row"] = timed(lambda: plan.type1_normal(7, T, shape), reps)[0] / T
        row["type1_rademacher_ms_per_row"] = timed(lambda: plan.type1_rademacher(7, T, shape), reps)[0] / T
        row["type1_materialised_ms_per_row"] = timed(lambda: plan.type1(Z, shape), reps)[0] / T
        rows.append(row)
        del Z, x, plan
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_paths_mi355x.json"))
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py needs a GPU: a CPU run says nothing about these timings")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "kernel": "SE l=0.2 var=2 sigmasq=0.2 eps=1e-4",
           "nufft_eps": 1e-7, "cg_tolerance": 1e-4, "sizes": []}
    for N in [int(float(s)) for s in args.sizes.split(",") if s]:
        res["sizes"].append(bench_size(N, args.draws, args.reps))
        print(json.dumps(res["sizes"][-1]), flush=True)
    res["other_spread_paths"] = bench_other_paths(args.reps)
    for r in res["other_spread_paths"]:
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
