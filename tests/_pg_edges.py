"""Case builders and references of tests/test_pg_edges_host.py and tests/test_gpu_pg_kernel_edges.py: the five entries of
csrc/pg_ops.hip at the sizes where their grids end or wrap, with the points at which the per-point formulas change arm planted at
fixed indices.  Host only (CPU tensors, float64); nothing here touches the GPU.

Launch rules restated from csrc/pg_ops.hip, so that a test can assert that its size really wraps:
  E-step, total-count gradient, M-step terms   min(ceil(n / 256), 1024) workgroups of 256 (four wave64) -- the grid-stride loop
                                               wraps from n = 262145
  weight rows                                  min(ceil(n / 256), 512) workgroups per row -- wraps from n = 131073
"""
import math

import numpy as np
import torch

import _helper_seams as H
import _pgnb

THREADS = 256
MAX_BLOCKS = 1024
WRAP = THREADS * MAX_BLOCKS                               # 262144: the first size whose every thread holds a point
ESTEP_SIZES = (1, 63, 64, 65, 255, 256, 257, WRAP, WRAP + 1, WRAP + 257)
WEIGHT_ROWS_BLOCKS = 512
NB_TOTAL_COUNTS = (1e-3, 1.0, 37.5)
U53 = 2.0 ** -53
_F = torch.float64

BELOW_1E12 = float(np.nextafter(1e-12, 0.0))
ABOVE_1E12 = float(np.nextafter(1e-12, 1.0))
TINY = 5e-324                                             # the smallest subnormal: sigmoid(+-TINY / den) is exactly 0.5

MAX_POSITIONS = ("index_0", "wave3_last_lane", "last_thread_of_last_workgroup", "wrapped_tail")


def blocks(n):
    return max(1, min((n + THREADS - 1) // THREADS, MAX_BLOCKS))


def max_index(position, N):
    """Index of the planted maximum of |delta - Lambda|: lane 63 of wave 3 of workgroup 0 is thread 255, the last thread of the
    last workgroup holds index blocks * 256 - 1 in its first trip, and N - 1 is in the second trip when N > 262144."""
    if position == "wrapped_tail":
        assert N > WRAP
    return {"index_0": 0, "wave3_last_lane": THREADS - 1, "last_thread_of_last_workgroup": blocks(N) * THREADS - 1,
            "wrapped_tail": N - 1}[position]


def estep_restated(S, delta, y, rho, probes, pg_b):
    """efgp_pg_estep_update in torch, with the probe sum in the kernel's order (sequential over j, no FMA)."""
    from polyagamma_classification import _pg_omega_expectation, approximate_logistic_gaussian_prob
    J = probes.shape[0]
    mean = S[0].clone()
    acc = torch.zeros_like(mean)
    for j in range(J):
        acc = acc + probes[j] * S[j + 1]
    sd = acc / torch.full_like(acc, J)                   # a true division (torch turns `/ J` into a product with 1/J)
    c = torch.sqrt((sd + mean.pow(2)).clamp_min(1e-12))
    lam = _pg_omega_expectation(c, pg_b if pg_b is not None else torch.ones_like(mean))
    dn = (delta * (1.0 - rho) + rho * lam).clamp(min=0.0)
    resid = float((dn - lam).abs().max())
    correct = int((approximate_logistic_gaussian_prob(mean, sd).gt(0.5) == y.bool()).sum())
    return mean, sd, dn, resid, correct


def estep_j0(S, delta, y, rho, pg_b, r=None):
    """The restatements at J = 0: sigma_diag is 0 (the kernel skips the probe mean; 0 / 0 in the torch line would be NaN)."""
    N = S.shape[1]
    z = torch.zeros((1, N), dtype=_F)
    S1 = torch.cat([S[:1], z])
    if r is None:
        return estep_restated(S1, delta, y, rho, z + 1.0, pg_b)
    return _pgnb.nb_estep_restated(S1, delta, y, r, rho, z + 1.0)


# ---- E-step cases -------------------------------------------------------------------------------------------------------------
# (kind, mean, sigma_diag, y, delta0, pg_b); None = leave the background value.  sigma_diag is planted exactly: S[j + 1] = z_j sd,
# so the probe mean is (sd + ... + sd) / J = sd for J <= 2.
_BERNOULLI = [
    ("clamp_m0_sd0", 0.0, 0.0, 1.0, None, None),
    ("sum_exactly_zero", 0.5, -0.25, 0.0, None, None),
    ("sum_negative", 0.5, -3.0, 1.0, None, None),
    ("c2_one_ulp_below_1e-12", 0.0, BELOW_1E12, 0.0, None, None),
    ("c2_one_ulp_above_1e-12", 0.0, ABOVE_1E12, 1.0, None, None),
    ("m_plus_40", 40.0, 0.3, 1.0, None, None),
    ("m_minus_40", -40.0, 0.3, 1.0, None, None),
    ("m_plus_800", 800.0, 0.3, 0.0, None, None),
    ("m_minus_800", -800.0, 0.3, 0.0, None, None),
    ("m_plus_tiny_y0", TINY, 0.3, 0.0, None, None),
    ("m_plus_tiny_y1", TINY, 0.3, 1.0, None, None),
    ("m_minus_tiny_y0", -TINY, 0.3, 0.0, None, None),
    ("m_minus_tiny_y1", -TINY, 0.3, 1.0, None, None),
    ("y_plus_zero", 1.5, 0.2, 0.0, None, None),
    ("y_minus_zero", 1.5, 0.2, -0.0, None, None),
    ("y_one", -1.5, 0.2, 1.0, None, None),
    ("y_two", -1.5, 0.2, 2.0, None, None),
    ("delta0_negative", 0.7, 0.2, 1.0, -1e7, None),
    ("b_zero", 0.7, 0.2, 0.0, None, 0.0),
    ("b_tiny", 0.7, 0.2, 1.0, None, 1e-300),
    ("b_one", 0.7, 0.2, 0.0, None, 1.0),
    ("b_1e6", 0.7, 0.2, 1.0, None, 1e6),
]
_NEGATIVE_BINOMIAL = [
    ("clamp_m0_sd0", 0.0, 0.0, 1.0, None, None),
    ("sum_exactly_zero", 0.5, -0.25, 0.0, None, None),
    ("sum_negative", 0.5, -3.0, 1.0, None, None),                        # also the max(sd, 0) of the metric
    ("c2_one_ulp_below_1e-12", 0.0, BELOW_1E12, 0.0, None, None),
    ("c2_one_ulp_above_1e-12", 0.0, ABOVE_1E12, 1.0, None, None),
    ("m_plus_40", 40.0, 0.3, 1.0, None, None),
    ("m_minus_40", -40.0, 0.3, 1.0, None, None),
    ("m_minus_800", -800.0, 0.3, 0.0, None, None),
    ("y_zero", 1.5, 0.2, 0.0, None, None),
    ("y_one", -1.5, 0.2, 1.0, None, None),
    ("y_1e4", -1.5, 0.2, 1e4, None, None),
    ("delta0_negative", 0.7, 0.2, 1.0, -1e10, None),
]
_NB_OVERFLOW = ("m_710_mean_count_inf", 710.0, 0.3, 1.0, None, None)
_NEEDS_SD = ("sum_exactly_zero", "sum_negative", "c2_one_ulp_below_1e-12", "c2_one_ulp_above_1e-12")
_NEEDS_B = ("b_zero", "b_tiny", "b_one", "b_1e6")
MAX_DELTA0 = 1e12                                         # the planted maximum: |dn - Lambda| ~ (1 - rho) 1e12 above every other point


def estep_kinds(likelihood, J=2, with_b=True, overflow=False):
    """Names of the special points a case of these options holds."""
    table = _BERNOULLI if likelihood == "bernoulli" else _NEGATIVE_BINOMIAL + ([_NB_OVERFLOW] if overflow else [])
    return [k[0] for k in table if (J > 0 or k[0] not in _NEEDS_SD) and (with_b or k[0] not in _NEEDS_B)]


def estep_case(N, J, likelihood="bernoulli", *, probes=None, with_b=True, overflow=False, max_at="index_0", start=0, seed=0,
               all_hits=None, tail_free=0):
    """-> dict(S (J+1, N), probes (J, N) of exact +-1, y, delta0, pg_b or None, kinds {name: index}, max_index, undecided).

    Background points: |mean| in [0.05, 3], S rows ~ 0.5 N(0, 1), y in {0, 1} (counts for the negative binomial), delta0 in
    [0, 0.3), pg_b in [0.5, 1.5).  The special points sit at indices N - 1, N - 2, ... (so index N - 1 always holds one, and in a
    size that wraps they are in the second trip of the grid-stride loop) except where the planted maximum needs the index; a size
    smaller than the table holds the N kinds from `start` on.  `probes` passes rows in (the counter-hash rows of a seed); J <= 2
    keeps the planted sigma_diag exact.  all_hits = True / False sets every y so that every point is a hit / a miss; tail_free
    keeps that many last indices as background points."""
    assert J <= 2 and likelihood in ("bernoulli", "negative_binomial")
    bern = likelihood == "bernoulli"
    g = torch.Generator().manual_seed(1000 + 7 * N + J + seed)
    S = torch.randn((J + 1, N), generator=g, dtype=_F) * 0.5
    sign = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(_F)
    S[0] = sign * (0.05 + 2.95 * torch.rand(N, generator=g, dtype=_F))
    if probes is None:
        probes = (torch.randint(0, 2, (J, N), generator=g) * 2 - 1).to(_F)
    assert probes.shape == (J, N) and bool((probes.abs() == 1.0).all())
    if bern:
        y = torch.randint(0, 2, (N,), generator=g).to(_F)
    else:
        y = torch.floor(torch.rand(N, generator=g, dtype=_F) ** 3 * 200.0)
    delta0 = torch.rand(N, generator=g, dtype=_F) * 0.3
    pg_b = torch.rand(N, generator=g, dtype=_F) + 0.5 if (bern and with_b) else None
    table = [k for k in (_BERNOULLI if bern else _NEGATIVE_BINOMIAL + ([_NB_OVERFLOW] if overflow else []))
             if k[0] in estep_kinds(likelihood, J, with_b, overflow)]
    start %= len(table)
    imax = max_index(max_at, N) if N > 1 else None
    free = [i for i in range(N - 1 - tail_free, -1, -1) if i != imax][:len(table)]
    kinds, exact_half = {}, []
    for (kind, m, sd, yv, d0, b), i in zip(table[start:] + table[:start], free):
        kinds[kind] = i
        S[0, i] = m
        for j in range(J):
            S[j + 1, i] = probes[j, i] * sd
        y[i] = yv
        if d0 is not None:
            delta0[i] = d0
        if b is not None:
            pg_b[i] = b
        if abs(m) <= TINY:
            exact_half.append(i)
    if imax is None and kinds and table[start][4] is None:
        imax = 0                                                     # N = 1: the special point carries the maximum as well
    if imax is not None:
        # |dn - Lambda| there is far above Lambda, so the residual is no cancelled difference: two correct Lambdas an ulp apart
        # move it by an ulp of Lambda, not by a share of the residual that no relative bound could hold
        delta0[imax] = MAX_DELTA0
    # the p > 0.5 decision: away from the points where p is exactly 0.5, |mean / den| >= 1e-3 (never one rounding from the boundary)
    acc = torch.zeros(N, dtype=_F)
    for j in range(J):
        acc = acc + probes[j] * S[j + 1]
    sd_all = acc / J if J else acc
    ratio = (S[0] / torch.sqrt(1.0 + (math.pi / 8.0) * sd_all.clamp_min(0.0))).abs()
    decided = ratio >= 1e-3
    decided[exact_half] = True
    undecided = int((~decided).sum())
    assert undecided == 0
    if all_hits is not None:
        assert bern
        predicted = S[0] > 0.0                                       # sigmoid(m / den) > 0.5 <=> m > 0 (TINY rounds to exactly 0.5)
        predicted[exact_half] = False
        y = (predicted == all_hits).to(_F)
    return dict(S=S, probes=probes, y=y, delta0=delta0, pg_b=pg_b, kinds=kinds, max_index=imax, undecided=undecided)


def estep_reference(case, rho, r=None):
    """The restatement on a case -> (mean, sigma_diag, delta, residual, metric) and, for the negative binomial, the per-point terms
    |r exp(mean + max(sd, 0) / 2) - y| of the metric."""
    S, J = case["S"], case["probes"].shape[0]
    if r is None:
        out = estep_restated(S, case["delta0"], case["y"], rho, case["probes"], case["pg_b"]) if J else \
            estep_j0(S, case["delta0"], case["y"], rho, case["pg_b"])
        return out, None
    from polyagamma_classification import negative_binomial_gaussian_mean
    out = _pgnb.nb_estep_restated(S, case["delta0"], case["y"], r, rho, case["probes"]) if J else \
        estep_j0(S, case["delta0"], case["y"], rho, None, r)
    terms = torch.abs(negative_binomial_gaussian_mean(out[0], out[1], total_count=r) - case["y"])
    return out, terms


def fsum_terms(terms):
    """(math.fsum of the terms, of their magnitudes); NaN / inf as IEEE addition gives them (fsum raises on inf - inf and NaN-free
    input only)."""
    t = terms.detach().cpu().reshape(-1)
    if not bool(torch.isfinite(t).all()):
        return float(t.sum()), float(t.abs().sum())
    v = t.tolist()
    return math.fsum(v), math.fsum(abs(x) for x in v)


def sum_depth(n):
    """Roundings on the longest path of a two-launch sum of n terms: the per-thread chain, six levels of the wave tree and the
    four waves, then the same over the workgroups' partials in the finish kernel."""
    b = blocks(n)
    return math.ceil(n / (THREADS * b)) + 6 + 4 + math.ceil(b / THREADS) + 6 + 4


# ---- non-finite cases ---------------------------------------------------------------------------------------------------------
NONFINITE_N = 257
NONFINITE_AT = 256                                        # the one point of the last workgroup
ESTEP_NONFINITE = ("nan_mean", "nan_probe_row", "nan_delta0", "inf_mean", "all")
NB_NONFINITE = ESTEP_NONFINITE + ("nb_nan_sigma_diag",)
GRAD_NONFINITE = ("nan_sigma_diag", "nan_mean", "nan_y", "all")


def plant_nonfinite(case, what):
    """One non-finite value in a copy of an N = 257, J >= 1 case; "all" plants them at four neighbouring points.  -> (case,
    [planted indices])."""
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in case.items()}
    nan = float("nan")
    at = {"nan_mean": NONFINITE_AT, "nan_probe_row": NONFINITE_AT, "nan_delta0": NONFINITE_AT, "inf_mean": NONFINITE_AT,
          "nb_nan_sigma_diag": NONFINITE_AT}
    if what == "all":
        at = {"nan_mean": 252, "nan_probe_row": 253, "nan_delta0": 254, "inf_mean": 255}
        todo = list(at)
    else:
        todo = [what]
    for w in todo:
        i = at[w]
        assert i not in c["kinds"].values() and i != c["max_index"]
        if w == "nan_mean":
            c["S"][0, i] = nan
            c["delta0"][i] = 0.0                                     # delta = rho Lambda: the reference's b / 4 arm shows undamped
        elif w in ("nan_probe_row", "nb_nan_sigma_diag"):
            c["S"][0, i] = 1.0                                       # a finite positive mean and y = 1: a hit if sigma_diag were dropped
            c["S"][1, i] = nan
            c["y"][i] = 1.0
        elif w == "nan_delta0":
            c["delta0"][i] = nan
        elif w == "inf_mean":
            c["S"][0, i] = float("inf")
    return c, sorted(at[w] for w in todo)


def nonfinite_base(likelihood):
    """The clean N = 257 case the non-finite values are planted in: the special points end below index 252."""
    return estep_case(NONFINITE_N, 2, likelihood, max_at="index_0", tail_free=5)


# ---- total-count gradient -----------------------------------------------------------------------------------------------------
def grad_case(N, seed=0):
    """(y, mean, sigma_diag) with y in {0, 1, 1e4} and counts, mean = +-800, negative sigma_diag planted at the end."""
    g = torch.Generator().manual_seed(2000 + N + seed)
    y = torch.floor(torch.rand(N, generator=g, dtype=_F) ** 4 * 10001.0)
    mean = torch.randn(N, generator=g, dtype=_F) * 2.0
    sd = torch.rand(N, generator=g, dtype=_F) * 3.0 - 0.3            # a tenth of them negative
    special = [(0.0, 800.0, 0.5), (1.0, -800.0, 0.5), (1e4, 0.3, -2.0), (3.0, -0.4, -1e-300), (0.0, 0.0, 0.0)]
    kinds = {}
    for k, (yv, m, s) in enumerate(special[:N]):
        i = N - 1 - k
        y[i], mean[i], sd[i] = yv, m, s
        kinds[("y0_m_plus_800", "y1_m_minus_800", "y1e4_sd_negative", "sd_tiny_negative", "all_zero")[k]] = i
    return y, mean, sd, kinds


def grad_reference(y, mean, sd, r, nodes, weights):
    """(fsum of the per-point terms, sum of the magnitudes of what each term adds: |psi(y + r)| + |psi(r)| + sum_q |w_q ls_q|)."""
    terms = _pgnb.total_count_grad_terms(y, mean, sd, r, nodes, weights)
    rt = torch.tensor(r, dtype=_F)
    s = torch.sqrt(sd.clamp_min(0.0))
    pts = mean[:, None] + s[:, None] * nodes[None, :]
    mag = (torch.special.digamma(y + rt).abs() + torch.special.digamma(rt).abs()
           + (torch.nn.functional.logsigmoid(-pts) * weights[None, :]).abs().sum(dim=1))
    total, _ = fsum_terms(terms)
    return total, fsum_terms(mag)[0]


def grad_depth(n, Q):
    """sum_depth plus what one term carries: 2 Q roundings of the quadrature's products and sums, and 72 for the two digammas
    (each up to ten recurrence steps of a quotient and a sum, a logarithm and the series: 16, as much again for the reference's
    own digamma) and the exp / log1p of the log-sigmoid (a few ulp in kernel and reference alike)."""
    return sum_depth(n) + 2 * Q + 72


# ---- M-step terms -------------------------------------------------------------------------------------------------------------
def mstep_case(M, J, seed=0):
    """bx (M,), bj and R (J, M) complex with magnitudes over 1e-3 .. 1e3 and both signs, dprime (M, 4) real of both signs."""
    g = torch.Generator().manual_seed(3000 + 11 * M + J + seed)
    bx = H.signed_wide(M, g, True)
    bj = H.signed_wide(J * M, g, True).reshape(J, M)
    R = H.signed_wide(J * M, g, True).reshape(J, M)
    dp = H.signed_wide(4 * M, g, False).reshape(M, 4)
    return bx, bj, R, dp


def _fsum_scaled(parts, d):
    """fsum of d_k * x_k over every exact part x of `parts`: each product split again into an exact pair."""
    out = []
    for x in parts:
        out += list(H.exact_products(x, d))
    return math.fsum(np.concatenate(out).tolist())


def mstep_reference(bx, bj, R, dp):
    """term1[p] = sum_k D'[k,p] |bx_k|^2 and term2[p] = (1/J) sum_k D'[k,p] sum_j Re(conj(R_jk) b_jk) (0 for J = 0) by math.fsum
    over exact products; grad = (term1 - term2) / 2.  -> (term1, term2, grad, mag1, mag2) as lists over p; mag = the sums of the
    magnitudes (term2's already divided by J)."""
    J, M = bj.shape
    P = dp.shape[1]
    d = dp.numpy()
    sq = list(H.exact_products(bx.real.numpy(), bx.real.numpy())) + list(H.exact_products(bx.imag.numpy(), bx.imag.numpy()))
    cross = []
    for j in range(J):
        cross += list(H.exact_products(R[j].real.numpy(), bj[j].real.numpy()))
        cross += list(H.exact_products(R[j].imag.numpy(), bj[j].imag.numpy()))
    a_mag = (bx.real ** 2 + bx.imag ** 2).numpy()
    s_mag = sum(((R[j].real * bj[j].real).abs() + (R[j].imag * bj[j].imag).abs()).numpy() for j in range(J)) if J else np.zeros(M)
    t1, t2, mag1, mag2 = [], [], [], []
    for p in range(P):
        col = np.ascontiguousarray(d[:, p])
        t1.append(_fsum_scaled(sq, col))
        t2.append(_fsum_scaled(cross, col) / J if J else 0.0)
        mag1.append(math.fsum((np.abs(col) * a_mag).tolist()))
        mag2.append(math.fsum((np.abs(col) * s_mag).tolist()) / J if J else 0.0)
    grad = [0.5 * (a - b) for a, b in zip(t1, t2)]
    return t1, t2, grad, mag1, mag2


def mstep_depth(M, J):
    """Roundings on the longest path of term1 / term2: the per-thread chain, the wave tree and the four waves, the partials added
    one after the other in the finish kernel, and what a term carries (|bx|^2: three, the product with D': one; term2: four per
    probe, the product, the division by J)."""
    b = blocks(M)
    base = math.ceil(M / (THREADS * b)) + 6 + 4 + b
    return base + 4, base + 4 * J + 2
