"""The host dispatch of the CG solves (csrc/toeplitz_cg.hip: efgp_toeplitz_create_ex, cg_solve_sync; csrc/cg_multi.hip: setup_apply; csrc/cg_coop2d.hip: coop_enqueue;
csrc/cg_persistent.hip: persistent_cg_launch; csrc/cg_plan_host.cpp: the planners both call) restated in Python, and the named cases of
tests/test_gpu_cg_routes.py.

`route(ns, hermitian, env)` says which kernel a solve of the block `ns` runs on, from the block shape, the Hermitian promise and
the EFGP_NO_* hooks that are set; tests/test_dense_toeplitz_host.py::test_cases_take_their_routes asserts on a machine without a
GPU that every case lands where it is listed, and the GPU tests assert that the operator reports the same grids.
"""
import math

K_THREADS, K_SLOTS, K_MAX_GRID = 512, 4, 4608          # cg_plan_host.hpp: pcg::kThreads, kSlots, kMaxGrid
LINE1D_MAX_N = 64 * 4 - 1                              # 64 * l1d::KS - 1
COOP_LADDER = (96, 128, 192, 256, 384, 512)


def next_pow2(L):
    return 1 << (L - 1).bit_length()


def fft_shape(ns):
    """The reference's circulant grid: next power of two of 2 n - 1 per axis (force_pow2, efgpnd.py:1269)."""
    return tuple(next_pow2(2 * n - 1) for n in ns)


def padded_cells(F):
    """Cells of one ping-pong buffer of the generic kernel: the fastest axis is padded by one element when d > 1."""
    return math.prod(F[:-1]) * (F[-1] + 1 if len(F) > 1 else F[-1])


def persistent_cg_eligible(ns, F):
    if any(f & (f - 1) or f > 4096 for f in F):
        return False
    return padded_cells(F) <= K_MAX_GRID and math.prod(ns) <= K_SLOTS * K_THREADS


def radices_for(F):
    """Stockham radices of one axis of the generic kernel (radices_for): 8s, with 16 = 4 x 4, then 4 or 2."""
    k = (F - 1).bit_length()
    out = []
    while k >= 3 and k != 4:
        out.append(8)
        k -= 3
    if k == 4:
        out += [4, 4]
        k = 0
    if k == 2:
        out.append(4)
    if k == 1:
        out.append(2)
    return out


def operator(ns, env=()):
    """What efgp_toeplitz_create_ex decides for a block: dict(F, persistent_ok, cg64, h48, lines_ok, lines3_ok, coop_grid)."""
    ns = tuple(ns)
    d = len(ns)
    F = fft_shape(ns)
    Ls = tuple(2 * n - 1 for n in ns)
    eligible = persistent_cg_eligible(ns, F)
    square = d == 2 and ns[0] == ns[1] and F[0] == F[1]
    want48 = (square and ns[0] % 2 == 1 and ns[0] <= 23 and F[0] <= 64 and eligible
              and not {"EFGP_NO_CG48", "EFGP_NO_CG64", "EFGP_NO_CG_HERM"} & set(env))
    cg64 = (square and eligible and F[0] < 64 and Ls[0] <= 63 and not {"EFGP_NO_CG64_EMBED", "EFGP_NO_CG64"} & set(env))
    vhat_fused = d == 2 and F == (64, 64) and "EFGP_NO_VHAT64" not in env
    h48 = want48 and (vhat_fused or cg64)              # the 48 x 48 spectrum rides in a launch that makes a 64 x 64 one
    lines_ok = d == 2 and all(128 <= f <= 512 for f in F)
    lines3_ok = d == 3 and all(64 <= f <= 256 for f in F)
    coop_grid = None
    if lines_ok:
        small = tuple(next(c for c in COOP_LADDER if c >= L) for L in Ls)
        coop_grid = small if small != F and "EFGP_NO_COOP_SMALL" not in env else F
    # a grid of one cell has no transform stage: left to the multi-launch solver unless the 64 x 64 embedding takes it
    persistent_ok = eligible and not (math.prod(F) == 1 and not cg64)
    return dict(ns=ns, F=F, persistent_ok=persistent_ok, cg64=cg64, h48=h48, lines_ok=lines_ok, lines3_ok=lines3_ok, coop_grid=coop_grid)


def route(ns, hermitian=False, env=(), lanczos=False):
    """-> (kernel, grid the solve runs on).  kernel: herm48 | herm64 | line1d | 2d64 | generic (one launch, one workgroup per system),
    coop | coop_herm (cooperative launches), multi_lines2 | multi_lines3 | multi_lines3h | multi_fft (the multi-launch solver)."""
    op = operator(ns, env)
    ns, F, d = op["ns"], op["F"], len(op["ns"])
    if op["persistent_ok"] and "EFGP_NO_PERSISTENT_CG" not in env:
        G = (64, 64) if op["cg64"] else F
        fast64 = d == 2 and G == (64, 64) and ns[0] == ns[1] and ns[0] <= 32 and "EFGP_NO_CG64" not in env
        herm64 = fast64 and hermitian and not lanczos and ns[0] % 2 == 1 and ns[0] <= 31 and "EFGP_NO_CG_HERM" not in env
        if herm64 and op["h48"] and ns[0] <= 23 and "EFGP_NO_CG48" not in env:
            return "herm48", (48, 48)
        if herm64:
            return "herm64", G
        if d == 1 and not lanczos and ns[0] <= LINE1D_MAX_N and 8 <= G[0] <= 512 and "EFGP_NO_CG_LINE1D" not in env:
            return "line1d", G
        if fast64:
            return "2d64", G
        return "generic", tuple(f for f in G if f > 1)          # unit axes are dropped from the generic kernel's geometry
    if op["lines_ok"] and not {"EFGP_NO_CG_COOP", "EFGP_NO_CG_LINES"} & set(env):
        herm = hermitian and ns[0] % 2 == 1 and ns[1] % 2 == 1 and ns[0] >= 3 and "EFGP_NO_CG_COOP_HERM" not in env
        return ("coop_herm" if herm else "coop"), op["coop_grid"]
    if "EFGP_NO_CG_LINES" in env:
        return "multi_fft", F
    if op["lines_ok"]:
        return "multi_lines2", F
    if op["lines3_ok"]:
        herm = hermitian and all(n % 2 == 1 for n in ns) and ns[0] >= 3 and "EFGP_NO_CG_HERM3" not in env
        return ("multi_lines3h" if herm else "multi_lines3"), F
    return "multi_fft", F


def cg_shape(ns, hermitian=False, env=()):
    """efgp_toeplitz_cg_shape."""
    op = operator(ns, env)
    F = op["F"]
    if len(ns) == 2 and op["persistent_ok"]:
        if hermitian and op["h48"] and "EFGP_NO_CG48" not in env:
            return (48, 48)
        return (64, 64) if op["cg64"] else F
    if op["coop_grid"] is not None and op["coop_grid"] != F and not {"EFGP_NO_COOP_SMALL", "EFGP_NO_CG_COOP"} & set(env):
        return op["coop_grid"]
    return F


def single_launch_solves(ns, env=()):
    """efgp_toeplitz_single_launch_solves."""
    return operator(ns, env)["persistent_ok"] and "EFGP_NO_PERSISTENT_CG" not in env


def one_workgroup_per_system(ns):
    """ToeplitzOp.one_workgroup_per_system: at most 4096 cells on the reference's grid."""
    return math.prod(fft_shape(ns)) <= 4096


# ---- the named cases ----------------------------------------------------------------------------------------------------------
# name -> (block, hermitian, kernel).  DENSE: M <= 2048, held to the dense matrix.  ORACLE: the oracle's FFT Toeplitz.
DENSE = {
    # 1-D
    "1d_2": ((2,), False, "generic"),                   # F = 4: one radix-4 stage, the crop inside the fused middle stage
    "1d_3": ((3,), False, "line1d"),                    # F = 8: the smallest line1d, odd
    "1d_4": ((4,), False, "line1d"),                    # ... and even
    "1d_255": ((255,), False, "line1d"),                # the largest line1d
    "1d_256": ((256,), False, "generic"),               # F = 512: radices 8, 8, 8
    "1d_700": ((700,), False, "generic"),               # F = 2048: radices 8, 8, 8, 4
    "1d_2048": ((2048,), False, "generic"),             # F = 4096, M = kSlots * kThreads exactly
    "1d_1": ((1,), False, "multi_fft"),                 # one cell: no transform stage
    # 2-D generic
    "2d_2x3": ((2, 3), False, "generic"),
    "2d_8x64": ((8, 64), False, "generic"),             # the two stride orders
    "2d_64x16": ((64, 16), False, "generic"),
    "2d_4x256": ((4, 256), False, "generic"),           # F = (8, 512), padded 4104
    "2d_16x17": ((16, 17), False, "generic"),           # F = (32, 64)
    "2d_20x30": ((20, 30), False, "generic"),           # F = (64, 64), not square: must not take 2d64
    "2d_1x37": ((1, 37), False, "generic"),             # unit axis 0: it would own the fused middle stage
    "2d_37x1": ((37, 1), False, "generic"),
    # 2-D square
    "sq_2": ((2, 2), False, "2d64"),                    # even, embedded in 64 x 64
    "sq_8": ((8, 8), False, "2d64"),
    "sq_16": ((16, 16), False, "2d64"),
    "sq_24": ((24, 24), False, "2d64"),                 # even, on the grid itself
    "sq_32": ((32, 32), False, "2d64"),                 # L = 63
    "sq_2_herm": ((2, 2), True, "2d64"),                # a Hermitian promise on an even block: the general kernel
    "sq_8_herm": ((8, 8), True, "2d64"),
    "sq_16_herm": ((16, 16), True, "2d64"),
    "sq_24_herm": ((24, 24), True, "2d64"),
    "sq_32_herm": ((32, 32), True, "2d64"),
    "sq_23_herm": ((23, 23), True, "herm48"),           # 23 | 25: 48 x 48 against 64 x 64 Hermitian
    "sq_25_herm": ((25, 25), True, "herm64"),
    "sq_31_herm": ((31, 31), True, "herm64"),           # 31 | 32: Hermitian against complex
    # 3-D generic
    "3d_2x3x5": ((2, 3, 5), False, "generic"),
    "3d_4x8x16": ((4, 8, 16), False, "generic"),
    "3d_16x4x8": ((16, 4, 8), False, "generic"),
    "3d_8x16x4": ((8, 16, 4), False, "generic"),        # F = (16, 32, 8), padded 4608 = kMaxGrid exactly
    "3d_8x8x8": ((8, 8, 8), False, "generic"),
    "3d_3x7x9_herm": ((3, 7, 9), True, "generic"),      # no Hermitian kernel here: the general answer
    "3d_1x7x7": ((1, 7, 7), False, "generic"),
    "3d_7x1x7": ((7, 1, 7), False, "generic"),
    "3d_1x20x20": ((1, 20, 20), False, "generic"),      # what is left is a 64 x 64 square: still generic, 2d64 is picked by the caller's d
    "3d_1x1x9": ((1, 1, 9), False, "generic"),          # what is left is a 1-D F = 32 line: still generic, not line1d
    # no fused path: the multi-launch solver with no hook set
    "2d_30x50": ((30, 50), False, "multi_fft"),         # F = (64, 128)
    "3d_5x7x12": ((5, 7, 12), False, "multi_fft"),      # F = (16, 16, 32), padded 8448 > 4608
}
ORACLE = {
    "1d_2049": ((2049,), False, "multi_fft"),           # M above the persistent limit
    "3d_17x19x33": ((17, 19, 33), False, "multi_lines3"),       # F = (64, 64, 128)
    "3d_17x19x33_herm": ((17, 19, 33), True, "multi_lines3h"),
    "3d_17x18x33_herm": ((17, 18, 33), True, "multi_lines3"),   # an even axis: the Hermitian request falls back to general
    "2d_33x40": ((33, 40), False, "coop"),              # an even axis on the cooperative grid (96, 96)
}
CASES = {**DENSE, **ORACLE}
# one long solve per route on the ill-conditioned systems (sigma^2 = 4): judged on residual and direct solve only, not on counts
LONG = ("2d_8x64", "1d_255", "sq_24", "sq_25_herm", "sq_23_herm", "2d_30x50", "2d_33x40", "3d_17x19x33", "3d_17x19x33_herm")


def geometry_table():
    """One line per case: block, route, grid of the solve, padded cells of the generic kernel, radices per axis."""
    lines = [f"{'case':18} {'block':14} {'herm':5} {'route':14} {'F':16} {'solve grid':14} {'padded':>6}  radices per axis"]
    for name, (ns, herm, _) in CASES.items():
        kern, grid = route(ns, herm)
        F = fft_shape(ns)
        pad = padded_cells(grid) if kern == "generic" else ""
        rad = " | ".join(",".join(str(r) for r in radices_for(f)) for f in grid) if kern == "generic" else ""
        lines.append(f"{name:18} {str(ns):14} {str(herm):5} {kern:14} {str(F):16} {str(grid):14} {str(pad):>6}  {rad}")
    return "\n".join(lines)
