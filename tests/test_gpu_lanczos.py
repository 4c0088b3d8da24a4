"""GPU: the Lanczos mode of the single-launch CG kernels (EFGP_LANCZOS_BRANCH of cg_persistent_kernel and cg_persistent_2d64_kernel,
csrc/cg_persistent.hip) through efgp_hip.ops.lanczos, step by step against the dense recurrence of tests/_lanczos.py, and both
paths of efgpnd.logdet_slq against the dense value.

What is compared, and why the bounds are what they are, is settled on the CPU by tests/test_lanczos_host.py: three references of the
same recurrence (dense f64, dense 80-bit, the oracle's FFT product) agree per step to d_k; the steps with d_k <= 1e-10 are the
compared prefix; the kernel's alpha_k and beta_k must be within 100 max(d_k, 1e-15) |alpha_k| of the dense f64 recurrence there.
The factor 100 is a margin over the references' own distance: the kernel's product, FFT and block reductions round differently from
both (the forced-iteration CG tests hold 1e-12 where their references differ by 3e-15).  The Gauss-Lanczos quadrature of the
returned steps is held to z^H log(A) z from eigh of the dense matrix at 100 max(the references' own error, 1e-15).

Measured on an MI355X when this was written (33 blocks, both variants, two +-1 and two complex probes each), as the largest
(distance to the dense f64 recurrence) / (max(d_k, 1e-15) |alpha_k|) over the compared prefix, bound 100:
    steps        cg_persistent_kernel 10.4 (3d_1x1x9, variant 1, at a step where the references themselves differ by 1.7e-12: the
                 last before its Krylov space of nine is exhausted; below 3 everywhere else), cg_persistent_2d64_kernel 1.3
    quadrature   cg_persistent_kernel 2.8, cg_persistent_2d64_kernel 3.6 (the references' own error: at most 8e-15)
    2d64 against the generic kernel (EFGP_NO_CG64, and EFGP_NO_CG64_EMBED on (8, 8)): steps at most 1.4, quadrature at most 4.9
Breakdown, `taken` on all four probes, equal to the three references': ws = 0 on (8, 8): 1 (beta exactly 0 on the +-1 rows);
ws non-zero at one mode of (8, 8) and of (20, 30): 2; (2,): 2; (3,): 3; (1, 1, 3): 3; every last beta at most 1.6e-14.
logdet_slq: single launch, batched torch loop and dense value agree to all 15 printed digits on (8, 8), (16, 17), (30, 50) and on
(8, 8) with every probe stopping at step 2 of 25.

What these tests see: with alpha and beta swapped in the kernel's store, the store moved by one step, the - beta_prev q_prev term
dropped, sigma^2 u in the variant-1 arm of apply_A, or |z|^2 of every row written to row 0, between 76 and 147 of the 162 cases fail.
What they cannot see: `live[:, :-1]` in place of `live[:, 1:]` in logdet_slq.  The two differ only in whether the LAST recorded beta
of a probe that stopped early couples its last step to the padding, and the recurrence stops only where that beta is below 1e-12:
the eigenvalues move by its square.  The mask on the off-diagonal is a guard, not arithmetic.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _cg_routes as R
import _dense_toeplitz as D
import _lanczos as L

pytestmark = pytest.mark.gpu

MARGIN = 100.0
FLOOR = 1e-15
EPS = float(np.finfo(np.float64).eps)
PAIRS = [(name, variant) for name in L.CASES for variant in (0, 1)]          # case-major: the two-entry matrix caches hit
PAIR_IDS = [f"{name}-v{variant}" for name, variant in PAIRS]


@pytest.fixture(autouse=True)
def _serial_references():
    """One thread for the references, as tests/test_gpu_cg_routes.py."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _operator(ns):
    from efgp_hip import ToeplitzOp
    return ToeplitzOp(D.system(ns)["v"].cuda())


def _run(ns, variant, z, steps, ws=None, op=None):
    """ops.lanczos on the block -> (alpha (P, steps), beta (P, steps), norm2 (P,), taken (P,)) as numpy arrays, or None."""
    from efgp_hip.ops import lanczos
    s = D.system(ns)
    w = s["ws"] if ws is None else ws
    res = lanczos(op if op is not None else _operator(ns), w.cuda(), s["sigmasq"], variant, z.cuda(), steps)
    if res is None:
        return None
    return tuple(t.cpu().numpy() for t in res)


@functools.lru_cache(maxsize=None)
def _step_references(ns, variant, steps, ws_key="own"):
    """Per probe of L.probes(ns): the three references, d_k and the compared prefix."""
    A = L.matrix(ns, variant, ws_key)
    ws = None if ws_key == "own" else L.weights(ns, ws_key)
    return [L.references(A, D.system(ns), variant, z, steps, ws) for z in L.probes(ns)]


@functools.lru_cache(maxsize=None)
def _quad_references(ns, variant, ws_key="own", nreal=2, ncomplex=2, eigh_max=L.EIGH_MAX):
    """Per probe: (the value the quadrature is held to, the references' own relative error against it).  The value is the exact
    z^H log(A) z for M <= eigh_max and the dense recurrence's quadrature above."""
    s = D.system(ns)
    A = L.matrix(ns, variant, ws_key)
    ws = None if ws_key == "own" else L.weights(ns, ws_key)
    out = []
    for z in L.probes(ns, nreal, ncomplex):
        qd = L.quadrature(*L.lanczos_dense(A, z, L.QUAD_STEPS)[:3])
        qf = L.quadrature(*L.lanczos_fft(s, variant, z, L.QUAD_STEPS, ws)[:3])
        exact = L.exact_quadratic_form(L.eigen(ns, variant, ws_key), z) if math.prod(ns) <= eigh_max else qd
        out.append((exact, max(abs(qd - exact), abs(qf - exact)) / abs(exact)))
    return out


def _step_ratio(got_a, got_b, ref):
    """max over the compared prefix of (distance to the dense f64 recurrence) / (max(d_k, FLOOR) |alpha_k|); the prefix length."""
    p = ref["prefix"]
    a, b = ref["f64"][0][:p], ref["f64"][1][:p]
    dist = np.maximum(np.abs(got_a[:p] - a), np.abs(got_b[:p] - b))
    return float((dist / (np.maximum(ref["d"][:p], FLOOR) * np.abs(a))).max()), p


def _quad(alpha, beta, norm2, taken, row):
    k = int(taken[row])
    return L.quadrature(alpha[row, :k], beta[row, :k], norm2[row])


@pytest.mark.parametrize("name,variant", PAIRS, ids=PAIR_IDS)
def test_steps_equal_the_dense_recurrence(name, variant):
    ns, kernel = L.CASES[name]
    assert R.route(ns, lanczos=True)[0] == kernel
    M = math.prod(ns)
    K = min(L.STEPS, M)
    z = L.probes(ns)
    alpha, beta, norm2, taken = _run(ns, variant, z, K)
    refs = _step_references(ns, variant, K)
    assert alpha.shape == beta.shape == (4, K) and norm2.shape == taken.shape == (4,)
    assert np.isfinite(alpha).all() and np.isfinite(beta).all() and np.isfinite(norm2).all()
    ratios = []
    for r, ref in enumerate(refs):
        assert int(taken[r]) >= ref["prefix"] and 1 <= int(taken[r]) <= K
        ratios.append(_step_ratio(alpha[r], beta[r], ref)[0])
        exact2 = float(ref["ld"][2])
        if r < 2:
            assert float(norm2[r]) == float(M) == exact2               # +-1 rows: every partial sum is an integer
        else:
            assert abs(float(norm2[r]) - exact2) <= 4 * EPS * M * exact2
        assert (alpha[r, int(taken[r]):] == 0).all() and (beta[r, int(taken[r]):] == 0).all()
    worst = float(np.max(ratios))                                      # numpy's max: a NaN stays a NaN and fails the bound
    print(f"\n{name} ({kernel}) variant {variant}: K {K}, taken {taken.tolist()}, prefixes {[r['prefix'] for r in refs]}, "
          f"max d_k {max(float(r['d'][:r['prefix']].max()) for r in refs):.1e}, ratio {worst:.2f}")
    if M >= L.STEPS:
        assert taken.tolist() == [K] * 4
    assert worst <= MARGIN


@pytest.mark.parametrize("name,variant", PAIRS, ids=PAIR_IDS)
def test_quadrature_equals_the_exact_quadratic_form(name, variant):
    ns, kernel = L.CASES[name]
    res = _run(ns, variant, L.probes(ns), L.QUAD_STEPS)
    refs = _quad_references(ns, variant)
    worst = float(np.max([abs(_quad(*res, r) - exact) / abs(exact) / max(own, FLOOR) for r, (exact, own) in enumerate(refs)]))
    print(f"\n{name} ({kernel}) variant {variant}: taken {res[3].tolist()}, references' own error {max(o for _, o in refs):.1e}, ratio {worst:.2f}")
    assert np.isfinite(res[0]).all() and np.isfinite(res[1]).all()
    assert worst <= MARGIN


@pytest.mark.parametrize("name", list(L.BREAKDOWN))
def test_breakdown_stops_where_the_references_stop(name):
    """Variant 1 (the threshold is absolute).  The cases are those tests/test_lanczos_host.py shows to break at the same step in
    all three references with the last beta ten times under the threshold."""
    ns, ws_key, want = L.BREAKDOWN[name]
    ws = L.weights(ns, ws_key)
    z = L.probes(ns)
    alpha, beta, norm2, taken = _run(ns, 1, z, 10, ws=ws)
    refs = _step_references(ns, 1, 10, ws_key)
    print(f"\n{name}: taken {taken.tolist()} (references {[r['f64'][3] for r in refs]}), last beta {[float(beta[r, taken[r] - 1]) for r in range(4)]}")
    for r, ref in enumerate(refs):
        assert ref["f64"][3] == ref["fft"][3] == ref["ld"][3] == want
        assert int(taken[r]) == want
        assert _step_ratio(alpha[r], beta[r], ref)[0] <= MARGIN
        assert float(beta[r, want - 1]) < L.BREAK
        assert (alpha[r, want:] == 0).all() and (beta[r, want:] == 0).all()          # still the zeros ops.lanczos allocated
    if ws_key == "zero":
        assert (alpha[:2, 0] == 1.0).all() and (beta[:2, 0] == 0.0).all()             # A = I, q = z / 8: exact
    if ws_key != "own":                                                                # the same rows under the full ws run on
        assert _run(ns, 1, z, 10)[3].tolist() == [10] * 4


@pytest.mark.parametrize("variant", [0, 1])
def test_rows_are_independent(variant):
    """300 workgroups (more than CUs) in one launch: a row's outputs are those of the row run alone, bit for bit."""
    ns = (8, 8)
    z = L.probes(ns, 150, 150)
    assert len({tuple(r.tolist()) for r in torch.view_as_real(z).reshape(300, -1)}) == 300
    full = _run(ns, variant, z, L.STEPS)
    assert full[3].tolist() == [L.STEPS] * 300
    for r in (0, 149, 299):
        solo = _run(ns, variant, z[r:r + 1], L.STEPS)
        for got, want in zip(full, solo):
            assert np.array_equal(got[r], want[0]), r
    # an all-zero row in the middle: inv_nb = 0, so q = 0, alpha = beta = 0, one step recorded
    zz = z[[0, 150, 1, 151, 2]].clone()
    zz[2] = 0
    batch = _run(ns, variant, zz, L.STEPS)
    assert batch[2][2] == 0.0 and batch[3][2] == 1 and (batch[0][2] == 0).all() and (batch[1][2] == 0).all()
    for r in (1, 3):
        solo = _run(ns, variant, zz[r:r + 1], L.STEPS)
        for got, want in zip(batch, solo):
            assert np.array_equal(got[r], want[0]), r


@pytest.mark.parametrize("name,hook", [("sq_8", "EFGP_NO_CG64"), ("sq_23", "EFGP_NO_CG64"), ("sq_24", "EFGP_NO_CG64"), ("sq_32", "EFGP_NO_CG64"),
                                       ("sq_8", "EFGP_NO_CG64_EMBED")])
def test_the_two_kernels_agree(name, hook, monkeypatch):
    """The 64 x 64 kernel against the generic kernel on the same grid (EFGP_NO_CG64, read per call) and, for the embedded (8, 8),
    on the block's own 16 x 16 grid (EFGP_NO_CG64_EMBED, read when the operator is made)."""
    from efgp_hip import ToeplitzOp
    ns, kernel = L.CASES[name]
    assert kernel == "2d64" and R.route(ns, lanczos=True, env=(hook,))[0] == "generic"
    z = L.probes(ns)
    K = min(L.STEPS, math.prod(ns))
    for variant in (0, 1):
        fast = _run(ns, variant, z, K), _run(ns, variant, z, L.QUAD_STEPS)
        monkeypatch.setenv(hook, "1")
        op = ToeplitzOp(D.system(ns)["v"].cuda()) if hook == "EFGP_NO_CG64_EMBED" else None
        if op is not None:
            assert tuple(op.cg_shape()) == (16, 16)
        slow = _run(ns, variant, z, K, op=op), _run(ns, variant, z, L.QUAD_STEPS, op=op)
        monkeypatch.delenv(hook)
        refs, quads = _step_references(ns, variant, K), _quad_references(ns, variant)
        steps, quad = [], []
        for r, ref in enumerate(refs):
            p = ref["prefix"]
            dist = np.maximum(np.abs(fast[0][0][r, :p] - slow[0][0][r, :p]), np.abs(fast[0][1][r, :p] - slow[0][1][r, :p]))
            steps.append(float((dist / (np.maximum(ref["d"][:p], FLOOR) * np.abs(ref["f64"][0][:p]))).max()))
            qa, qb = _quad(*fast[1], r), _quad(*slow[1], r)
            quad.append(abs(qa - qb) / abs(quads[r][0]) / max(quads[r][1], FLOOR))
        worst, worst_q = float(np.max(steps)), float(np.max(quad))
        print(f"\n{name} variant {variant} under {hook}: steps ratio {worst:.2f}, quadrature ratio {worst_q:.2f}")
        assert fast[0][3].tolist() == slow[0][3].tolist() == [K] * 4 and np.array_equal(fast[0][2], slow[0][2])
        assert worst <= MARGIN and worst_q <= MARGIN


def test_one_step():
    for ns in ((8, 8), (16, 17)):
        z = L.probes(ns)
        for variant in (0, 1):
            alpha, beta, norm2, taken = _run(ns, variant, z, 1)
            assert alpha.shape == (4, 1) and taken.tolist() == [1] * 4
            for r, zr in enumerate(z):
                ref = L.lanczos_dense(L.matrix(ns, variant), zr, 1)
                assert abs(alpha[r, 0] - ref[0][0]) <= 1e-13 * abs(ref[0][0]) and abs(beta[r, 0] - ref[1][0]) <= 1e-13 * abs(ref[0][0])


@pytest.mark.parametrize("name", list(L.REFUSED))
def test_refused_blocks_return_none(name):
    ns = L.REFUSED[name]
    assert not R.single_launch_solves(ns)
    assert _run(ns, 1, L.probes(ns, 1, 0), 3) is None


@pytest.mark.parametrize("what,kw", [("steps", dict(steps=0)), ("nprobes", dict(nprobes=0)), ("variant", dict(variant=2)), ("sigmasq", dict(sigmasq=0.0))])
def test_bad_arguments_are_refused_before_anything_is_written(what, kw):
    from efgp_hip import lib
    from efgp_hip.lib import EFGP_EINVAL
    ns = (8, 8)
    s = D.system(ns)
    op = _operator(ns)
    arg = dict(steps=3, nprobes=2, variant=1, sigmasq=s["sigmasq"])
    arg.update(kw)
    z = L.probes(ns, 1, 1).cuda()
    ws = s["ws"].cuda()
    alpha = torch.full((2, 3), -7.0, dtype=torch.float64, device="cuda")
    beta, norm2 = alpha.clone(), torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    taken = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = lib().efgp_lanczos(op._h, ptr(ws), float(arg["sigmasq"]), arg["variant"], ptr(z), arg["nprobes"], arg["steps"], ptr(alpha), ptr(beta),
                            ptr(norm2), ptr(taken), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = lib().efgp_last_error().decode()
    torch.cuda.synchronize()
    assert rc == EFGP_EINVAL and "efgp_lanczos" in msg and what in msg, (rc, msg)
    assert (alpha == -7).all() and (beta == -7).all() and (norm2 == -7).all() and (taken == -7).all()


def _pm1(ns, P=8):
    return L.probes(ns, P, 0)


def _logdet(ns, ws, zs, hook, monkeypatch):
    from efgpnd import logdet_slq
    if hook:
        monkeypatch.setenv(hook, "1")
    try:
        return logdet_slq(ws, D.SIGMASQ, _operator(ns), probes=len(zs), steps=L.QUAD_STEPS, n=D.NPTS, probe_vectors=zs.real)
    finally:
        if hook:
            monkeypatch.delenv(hook)


@pytest.mark.parametrize("ns,ws_key", [((8, 8), "own"), ((16, 17), "own"), ((30, 50), "own"), ((8, 8), "rank1")],
                         ids=["8x8", "16x17", "30x50-fallback-only", "8x8-rank1-breaks-at-2"])
def test_logdet_slq_on_both_paths(ns, ws_key, monkeypatch):
    """The single launch, the batched torch loop (EFGP_NO_PERSISTENT_CG) and the dense value mean_p z_p^H log(A_var) z_p + n log
    sigma^2 on the same operator and probes.  With the rank-one ws every probe stops at step 2 of 25: the tridiagonal matrices are
    assembled under the `live` mask on both paths.  The bound is the quadrature bound, relative to the mean quadratic form; the
    constant n log sigma^2 (2004, against a mean of tens) adds its own rounding, 4 ulp of the total."""
    ws = L.weights(ns, ws_key)
    zs = _pm1(ns)
    refs = _quad_references(ns, 1, ws_key, 8, 0, eigh_max=D.DENSE_MAX)          # (30, 50), M = 1500: one eigh
    mean = sum(e for e, _ in refs) / len(refs)
    dense = mean + D.NPTS * math.log(D.SIGMASQ)
    values = {"dense": dense, "torch loop": _logdet(ns, ws, zs, "EFGP_NO_PERSISTENT_CG", monkeypatch)}
    single = R.single_launch_solves(ns)
    assert single == (ns != (30, 50))
    if single:
        values["single launch"] = _logdet(ns, ws, zs, None, monkeypatch)
        want = [L.lanczos_dense(L.matrix(ns, 1, ws_key), z, L.QUAD_STEPS)[3] for z in zs]
        assert want == ([2] * 8 if ws_key == "rank1" else [L.QUAD_STEPS] * 8)
        assert _run(ns, 1, zs, L.QUAD_STEPS, ws=ws)[3].tolist() == want
    bound = MARGIN * max(max(o for _, o in refs), FLOOR) * abs(mean) + 4 * EPS * abs(dense)
    print(f"\n{ns} {ws_key}: " + ", ".join(f"{k} {v:.15g}" for k, v in values.items()) + f"; mean quadratic form {mean:.6g}, bound {bound:.2e}")
    keys = list(values)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert abs(values[a] - values[b]) <= bound, (a, b, values[a] - values[b])
