"""GPU: the batched helper entries (csrc/variance_ops.hip, csrc/gradient_ops.hip, the pad | FFT | crop arm and the dot product of
csrc/toeplitz_cg.hip, the groups of csrc/cg_multi.hip, the fills of csrc/nufft.hip, the bounding box of csrc/points_layout.hip)
across their slab seams, their 65535-row launches and the wraps of their grid-stride loops.

Every case is the smallest shape that crosses the seam it names; the host rules that place the seams are restated in
tests/_helper_seams.py and asserted here, so a case that stops crossing its seam fails instead of passing for nothing.  References:
torch.fft / the defining formulas on the host in float64, math.fsum of exact products for the dot product, the oracle's CG for the
capped solve; across a seam the rows must also equal, bit for bit, the same rows computed by calls that stay inside one slab.
Each case prints its measured error.
"""
import math

import numpy as np
import pytest
import torch

import _cg_routes as R
import _dense_toeplitz as D
import _helper_seams as H
import _pg_variance as V
import _sampling as S

pytestmark = pytest.mark.gpu

_CD = torch.complex128
EPS64 = 2.0 ** -52
ROWS = H.GRID_ROWS + 6                                   # 65541: one launch of 65535 rows and one of 6
SEAM_ROWS = (0, H.GRID_ROWS - 1, H.GRID_ROWS, H.GRID_ROWS + 1, ROWS - 1)


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. probe slabs of the lag sums
# ------------------------------------------------------------------------------------------------------------------------------
def _lag_error(shape, J, seed, nd=False):
    from efgp_hip import lag_sums
    gam, eta = H.lag_problem(shape, J, seed)
    mtot = list(shape) if nd else shape[0]
    out = lag_sums(gam.cuda(), eta.cuda(), mtot, len(shape)).cpu()
    ref = H.lag_reference(gam, eta, shape)
    assert out.shape == ref.shape
    return float((out - ref).abs().max() / ref.abs().max()), out


def test_lag_sums_general_route_across_probe_slabs_3d():
    """3-D mtot = 33: P = 96^3, 9 probes per slab, so J = 21 is two full slabs and a short one (the accumulate arm, add = 1), and
    both P and S = 65^3 exceed the 262144 threads of one launch: every kernel of the route wraps its grid-stride loop."""
    shape, J = (33, 33, 33), 21
    P, S = H.lag_box(shape), math.prod(2 * n - 1 for n in shape)
    per = H.lag_probes_per_slab(P)
    assert (P, per) == (884736, 9) and S > 262144 and J == 2 * per + 3
    err, _ = _lag_error(shape, J, 31)
    print(f"\nlag_sums 3-D mtot 33, {J} probes in slabs of {per}: {err:.2e} of max|ref|")
    assert err < 1e-12


def test_lag_sums_nd_across_probe_slabs():
    shape = (9, 5, 7)
    P = H.lag_box(shape)
    per = H.lag_probes_per_slab(P)
    J = 2 * per + 3
    assert P == 24 * 12 * 16 and per == (1 << 28) // (32 * P) and -(-J // per) >= 3      # at least three slabs, the last one short
    err, _ = _lag_error(shape, J, 32, nd=True)
    print(f"\nlag_sums_nd {shape}, {J} probes in slabs of {per}: {err:.2e} of max|ref|")
    assert err < 1e-12


def test_lag_sums_64x64_route_across_probe_slabs():
    """2-D mtot = 3 on the library's own 64 x 64 transforms: 2048 probes per slab, the accumulator kept conjugated across them
    (add = 1, conj_out = 1)."""
    per = H.lag_probes_per_slab(4096)
    J = 2 * per + 3
    assert per == 2048 and J == 4099
    err, _ = _lag_error((3, 3), J, 33)
    print(f"\nlag_sums 64 x 64 route, mtot 3, {J} probes in slabs of {per}: {err:.2e} of max|ref|")
    assert err < 1e-12


@pytest.mark.parametrize("mtot", [3, 23])
def test_lag_sums_general_route_for_small_2d_boxes(mtot, monkeypatch):
    """EFGP_NO_LAG64 sends 2-D mtot <= 32 through the general route (hipFFT at the ladder's lengths): same lags, same bound; and
    the two routes agree with each other."""
    monkeypatch.setenv("EFGP_NO_LAG64", "1")
    err, _ = _lag_error((mtot, mtot), 3, 34 + mtot)
    _, general = _lag_error((mtot, mtot), 5, 60 + mtot)
    monkeypatch.delenv("EFGP_NO_LAG64")
    err64, own = _lag_error((mtot, mtot), 5, 60 + mtot)
    between = float((own - general).abs().max() / general.abs().max())
    print(f"\nlag_sums 2-D mtot {mtot}: general route {err:.2e}, 64 x 64 route {err64:.2e}, between the routes at J = 5 {between:.2e}")
    assert err < 1e-12 and err64 < 1e-12 and between < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# 2. row slabs of the Toeplitz product
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nrows,check", [((141, 141), 515, (0, 255, 256, 257, 511, 512, 514)),
                                               ((21, 21, 21), 1027, (0, 511, 512, 513, 1023, 1024, 1026))], ids=["141x141", "21x21x21"])
def test_toeplitz_apply_across_row_slabs(shape, nrows, check):
    from efgp_hip import ToeplitzOp
    g = torch.Generator().manual_seed(len(shape) * 1000 + shape[0] + 7)
    v = H.crandn(shape, g)
    op = ToeplitzOp(v.cuda())
    M = op.size
    per = H.toeplitz_rows_per_slab(op.fft_cells)
    assert per == {2: 256, 3: 512}[len(shape)] and nrows == 2 * per + 3
    x = H.crandn((nrows, M), g)
    pre, post = H.crandn((M,), g), H.crandn((M,), g)
    xd, pred, postd = x.cuda(), pre.cuda(), post.cuda()
    xr = x.real.contiguous()
    rows = list(check)
    plain = op.apply(xd)
    scaled = op.apply_scaled(xd, pre=pred, post=postd)
    real = op.apply_scaled(xr.cuda(), pre=pred, post=postd)
    e_plain = H.rel_rows(plain[rows], H.toeplitz_reference(v, x[rows]))
    e_scaled = H.rel_rows(scaled[rows], post * H.toeplitz_reference(v, pre * x[rows]))
    e_real = H.rel_rows(real[rows], post * H.toeplitz_reference(v, pre * xr[rows].to(_CD)))
    print(f"\nToeplitz {shape}, {nrows} rows in slabs of {per}: apply {e_plain:.2e}, apply_scaled {e_scaled:.2e}, real input {e_real:.2e}")
    assert e_plain < 1e-13 and e_scaled < 1e-13 and e_real < 1e-13
    # every row equals the row of a call that stays inside one slab
    cuts = [(r0, min(r0 + per, nrows)) for r0 in range(0, nrows, per)]
    assert all(b - a <= per for a, b in cuts)
    assert torch.equal(plain, torch.cat([op.apply(xd[a:b]) for a, b in cuts]))
    assert torch.equal(scaled, torch.cat([op.apply_scaled(xd[a:b], pre=pred, post=postd) for a, b in cuts]))
    assert torch.equal(real, torch.cat([op.apply_scaled(xr[a:b].cuda(), pre=pred, post=postd) for a, b in cuts]))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. groups of the multi-launch solve
# ------------------------------------------------------------------------------------------------------------------------------
NS3, NSYS = (17, 19, 33), 131
SAME = (0, 63, 64, 127, 128, 130)


@pytest.fixture
def _serial_oracle():
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def _group_case(herm):
    from efgp_hip import ToeplitzOp
    kernel = "multi_lines3h" if herm else "multi_lines3"
    assert R.route(NS3, herm)[0] == kernel
    s = D.system(NS3, herm, nb=NSYS)
    op = ToeplitzOp(s["v"].cuda())
    per = H.cg_systems_per_group(op.fft_cells)
    assert op.fft_cells == 64 * 64 * 128 and per == 64 and -(-NSYS // per) == 3
    return s, op, per, kernel


def _cg(op, s, b, x0, herm, **kw):
    from efgp_hip import cg_solve
    return cg_solve(op, s["ws"].cuda(), s["sigmasq"], 0, b.cuda(), None if x0 is None else x0.cuda(), kw.pop("tol"), diag=s["diag"].cuda(),
                    batched=True, hermitian=herm, **kw)


@pytest.mark.parametrize("herm", [False, True], ids=["multi_lines3", "multi_lines3h"])
def test_capped_multi_launch_solve_across_groups(herm, _serial_oracle):
    """131 systems in groups of 64, five forced iterations.  The same system at rows 0, 63, 64, 127, 128 and 130 (first and last
    slot of each group) must give the same bits, and row 64 -- slot 0 of the second group -- the oracle's capped recurrence at the
    1e-12 tests/test_gpu_cg_routes.py holds forced iterations to."""
    from oracle import efgp_oracle as O
    s, op, per, kernel = _group_case(herm)
    b, x0 = s["b"].clone(), s["x0"].clone()
    for r in SAME:
        b[r], x0[r] = s["b"][5], s["x0"][5]
    x, it, rows = _cg(op, s, b, x0, herm, tol=1e-30, max_iter=5, early_stop=False)
    x = x.cpu()
    A = O.make_A_mean(s["ws"], O.Toeplitz(s["v"]), s["sigmasq"])
    ref = O.cg_batched(A, b[64:65], x0[64:65], 1e-30, max_iter=5, early=False, diag=s["diag"])[0][0]
    err = float(torch.linalg.norm(x[64] - ref) / torch.linalg.norm(ref))
    apart = max(float((x[r] - x[64]).abs().max()) for r in SAME) / float(x[64].abs().max())
    print(f"\n{kernel}, {NSYS} systems in groups of {per}, 5 forced iterations: row 64 - oracle {err:.2e}; the six equal systems are "
          f"{apart:.2e} apart")
    assert it == 5 and rows == [5] * NSYS
    assert err < 1e-12
    assert float(x[1].abs().max()) == 0.0                          # the zero row of the first group stays zero
    for r in SAME:
        assert torch.equal(x[r], x[64]), f"row {r} differs from row 64"


@pytest.mark.parametrize("herm", [False, True], ids=["multi_lines3", "multi_lines3h"])
def test_stopping_multi_launch_solve_across_groups(herm):
    """Converged solves whose counts differ between the groups: per-row counts and solutions must be those of the same rows solved
    in calls of 64 systems, and the total follows the batched convention.

    The stopping rule is relative to |b|, so one factor per row moves no count (and a tiny row never stops: below |b| ~ 1e-8 the
    1e-16 in the denominator of the step length outweighs <p, A p>, and the row runs to the cap of 2 M = 21318 iterations --
    measured here, and the reference's loop does the same).  The rows of the second and third group are therefore scaled per mode:
    they keep the modes whose ws lies below its 20 % and 70 % quantile, where A is close to sigma^2 I and CG stops early.  ws is
    even on the Hermitian route, so such a row stays conjugate-even."""
    s, op, per, kernel = _group_case(herm)
    b = s["b"].clone()
    w = s["ws"].real
    b[per:2 * per] *= (w < torch.quantile(w, 0.2)).to(torch.float64)
    b[2 * per:] *= (w < torch.quantile(w, 0.7)).to(torch.float64)
    x, it, rows = _cg(op, s, b, None, herm, tol=1e-8)
    tops = [max(rows[r0:r0 + per]) for r0 in range(0, NSYS, per)]
    print(f"\n{kernel}, {NSYS} systems in groups of {per}: largest count per group {tops}, total {it}")
    assert len(set(tops)) == 3 and rows[1] == 1                    # the groups stop at different counts; the zero row at once
    assert it == max(rows) + 1 and max(rows) < 2 * op.size         # cg.py:243: the terminating pass is counted unless capped
    for r0 in (0, per, NSYS - per):                                # the last call holds the short group's rows in its last slots
        xs, its, rs = _cg(op, s, b[r0:r0 + per], None, herm, tol=1e-8)
        assert rs == rows[r0:r0 + per], (r0, rs, rows[r0:r0 + per])
        assert its == max(rs) + 1
        assert torch.equal(xs, x[r0:r0 + per]), f"rows {r0}..{r0 + per - 1}"


# ------------------------------------------------------------------------------------------------------------------------------
# 4. more rows than gridDim.y holds
# ------------------------------------------------------------------------------------------------------------------------------
def _short_spans(n):
    """Two short calls that cover the seam rows: the first rows, and the rows around 65535 to the end."""
    return [(0, 4), (H.GRID_ROWS - 3, n)]


@pytest.mark.parametrize("per_axis", [False, True], ids=["isotropic", "per_axis"])
def test_variance_rhs_across_65535_points(per_axis):
    from efgp_hip import variance_rhs
    g = torch.Generator().manual_seed(41)
    shape, hs = ((3, 3), (0.31, 0.31)) if not per_axis else ((3, 1), (0.31, 0.17))          # 9 and 3 modes per row
    M = math.prod(shape)
    x = torch.rand(ROWS, 2, generator=g, dtype=torch.float64) * 2 - 1
    ws = H.crandn((M,), g)
    args = (list(hs), list(shape)) if per_axis else (hs[0], shape[0])
    out = variance_rhs(x.cuda(), args[0], args[1], ws.cuda())
    rows = list(SEAM_ROWS)
    ref = ws * H.features(x[rows], hs, shape).conj()
    err = float((out[rows].cpu() - ref).abs().max())
    print(f"\nvariance_rhs {'per-axis' if per_axis else 'isotropic'}, {ROWS} points of {M} modes: {err:.2e}")
    assert out.shape == (ROWS, M) and err < 1e-12
    for a, b in _short_spans(ROWS):
        assert torch.equal(out[a:b], variance_rhs(x[a:b].cuda(), args[0], args[1], ws.cuda()))


@pytest.mark.parametrize("with_ws", [False, True], ids=["noise_only", "ws_fz"])
def test_hermitian_normal_rows_across_65535_rows(with_ws):
    from efgp_hip import hermitian_normal_rows, normal_fill, normal_row_offset
    dev, M, seed, a, b = _dev(), 7, 515, 0.37, 0.21
    g = torch.Generator().manual_seed(42)
    ws = fz = None
    if with_ws:
        w = torch.rand(M, generator=g, dtype=torch.float64)
        ws = (0.5 * (w + w.flip(0))).to(_CD).to(dev)                              # real and even
        fz = (S.conj_even_normal(ROWS, M, g) * 40.0).to(dev)
    out = hermitian_normal_rows(dev, seed, ROWS, M, a=a if with_ws else 0.0, ws=ws, fz=fz, b=b)
    assert out.shape == (ROWS, M) and torch.equal(out.flip(1).conj(), out)
    worst = 0.0
    for r in SEAM_ROWS:
        fill = normal_fill(dev, seed, 2, M, index_offset=normal_row_offset(2 * r))  # the pair of row r
        ref = S.hermitian_rows(fill, a=a, ws=ws, fz=None if fz is None else fz[r:r + 1], b=b)[0]
        err = float((out[r] - ref).abs().max()) / float(ref.abs().max())
        worst = max(worst, err)
        assert err <= 64 * EPS64, (r, err)
    print(f"\nhermitian_normal_rows {'a ws fz + b e' if with_ws else 'b e'}, {ROWS} rows: {worst:.2e} of the row's largest entry")
    for r0, r1 in _short_spans(ROWS):
        short = hermitian_normal_rows(dev, seed, r1 - r0, M, a=a if with_ws else 0.0, ws=ws, fz=None if fz is None else fz[r0:r1].contiguous(),
                                      b=b, index_offset=normal_row_offset(2 * r0))
        assert torch.equal(out[r0:r1], short), (r0, r1)


def test_rademacher_fill_across_65535_rows():
    from efgp_hip import normal_row_offset, rademacher_fill
    dev, n, seed, off = _dev(), 5, 987654321, 17
    Z = rademacher_fill(dev, seed, ROWS, n, index_offset=off)
    assert Z.shape == (ROWS, n) and bool((Z.abs() == 1.0).all())
    for r in SEAM_ROWS:
        assert Z[r].tolist() == [H.rademacher(seed, r, i, off) for i in range(n)], r
    mean = float(Z.mean())
    print(f"\nrademacher_fill {ROWS} rows of {n}: the seam rows equal the counter's signs; mean {mean:+.1e}")
    assert abs(mean) < 6.0 / math.sqrt(ROWS * n)                   # six standard deviations of the mean of fair signs
    for r0, r1 in _short_spans(ROWS):                              # row r is row 0 at index + r * stride
        assert torch.equal(Z[r0:r1], rademacher_fill(dev, seed, r1 - r0, n, index_offset=normal_row_offset(2 * r0, off)))


def test_toeplitz_apply_across_65535_rows():
    from efgp_hip import ToeplitzOp
    g = torch.Generator().manual_seed(44)
    v = H.crandn((9,), g)
    op = ToeplitzOp(v.cuda())
    assert op.size == 5 and op.fft_cells == 16 and H.toeplitz_rows_per_slab(op.fft_cells) == H.GRID_ROWS < ROWS
    x = H.crandn((ROWS, 5), g)
    xd = x.cuda()
    out = op.apply(xd)
    rows = list(SEAM_ROWS)
    err = H.rel_rows(out[rows], H.toeplitz_reference(v, x[rows]))
    print(f"\nToeplitz 1-D n = 5, {ROWS} rows: {err:.2e}")
    assert err < 1e-13
    for a, b in _short_spans(ROWS):
        assert torch.equal(out[a:b], op.apply(xd[a:b]))


def test_lag_sums_across_65535_probes():
    """1-D mtot = 35: P = 96 allows 87381 probes per slab of scratch, so 65541 probes were one launch of 65541 rows; now 65535 and 6."""
    P = H.lag_box((35,))
    assert P == 96 and (1 << 28) // (32 * P) == 87381 and H.lag_probes_per_slab(P) == H.GRID_ROWS
    err, _ = _lag_error((35,), ROWS, 45)
    print(f"\nlag_sums 1-D mtot 35, {ROWS} probes: {err:.2e} of max|ref|")
    assert err < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# 5. grid-stride wraps of one launch
# ------------------------------------------------------------------------------------------------------------------------------
def test_gradient_prepare_wraps():
    from efgp_hip import gradient_prepare
    g = torch.Generator().manual_seed(51)
    M = 262144 + 7                                                 # 1024 workgroups of 256 and seven more entries
    ws = torch.rand(M, generator=g, dtype=torch.float64).to(_CD).cuda()
    fy = H.crandn((M,), g).cuda()
    vc = H.crandn((1,), g).cuda()
    diag, rhs = gradient_prepare(ws, fy, vc, 0.37)
    ref_d = vc[0].real * ws.abs().pow(2) + 0.37                    # efgpnd.py:128-133
    err = float((diag - ref_d).abs().max() / ref_d.abs().max())
    print(f"\ngradient_prepare M = {M}: diagonal {err:.2e}; rhs bitwise")
    assert err < 1e-15
    assert torch.equal(rhs, ws * fy)                               # efgpnd.py:141 (ws is real: the products round identically)


def test_variance_rhs_wraps():
    from efgp_hip import variance_rhs
    g = torch.Generator().manual_seed(52)
    mtot, h = 41, 0.013
    M = mtot ** 3
    assert M > 256 * 256                                           # one launch has 256 workgroups of 256 per point
    x = torch.rand(2, 3, generator=g, dtype=torch.float64) * 2 - 1
    ws = H.crandn((M,), g)
    out = variance_rhs(x.cuda(), h, mtot, ws.cuda()).cpu()
    ref = ws * H.features(x, (h,) * 3, (mtot,) * 3).conj()
    err = float((out - ref).abs().max())
    print(f"\nvariance_rhs M = 41^3, 2 points: {err:.2e}")
    assert err < 1e-12 * float(ws.abs().max())


def test_hermitian_normal_rows_wraps():
    from efgp_hip import hermitian_normal_rows, normal_fill
    dev, seed, a, b = _dev(), 53, 0.37, 0.21
    M = 524288 + 3                                                 # the lower half and centre: 262146 entries for 262144 threads
    g = torch.Generator().manual_seed(53)
    w = torch.rand(M, generator=g, dtype=torch.float64)
    ws = (0.5 * (w + w.flip(0))).to(_CD).to(dev)
    fz = (S.conj_even_normal(2, M, g) * 40.0).to(dev)
    fill = normal_fill(dev, seed, 4, M)
    out = hermitian_normal_rows(dev, seed, 2, M, a=a, ws=ws, fz=fz, b=b)
    ref = S.hermitian_rows(fill, a=a, ws=ws, fz=fz, b=b)
    err = max(float((out[s] - ref[s]).abs().max()) / float(ref[s].abs().max()) for s in range(2))
    print(f"\nhermitian_normal_rows M = {M}, 2 rows: {err:.2e} of the row's largest entry")
    assert err <= 64 * EPS64
    assert torch.equal(out.flip(1).conj(), out)


def test_cheb_interp_wraps():
    from efgp_hip.ops import cheb_interp
    shape, npts = (7, 7), 262144 + 5
    axes = [V.cheb_axis(lo, hi, n) for (lo, hi), n in zip([(-0.7, 1.9), (0.3, 2.1)], shape)]
    values = np.random.default_rng(54).normal(size=shape) * 3.0
    x, n_fixed = V.kernel_points([a[0] for a in axes], 254, npts)
    x = x[-npts:]                                                  # every special point is among the last 300
    assert n_fixed <= 300 and x.shape == (npts, 2)
    sel = np.unique(np.concatenate([np.arange(0, npts, 97), np.arange(npts - 300, npts)]))
    mats = [V.bary_matrix(ax[0], ax[1], x[sel, a]) for a, ax in enumerate(axes)]
    dense = V.interp_dense(values, mats)
    nodes, weights = [a[0] for a in axes], [a[1] for a in axes]
    raw = cheb_interp(nodes, weights, torch.as_tensor(values).cuda(), torch.as_tensor(x).cuda(), clamp=False).cpu().numpy()
    tol = 1e-13 * np.abs(values).max()
    err = float(np.abs(raw[sel] - dense).max())
    print(f"\ncheb_interp {shape}, {npts} points, {sel.size} of them against the dense formula: {err:.2e} (tolerance {tol:.2e})")
    assert np.isfinite(raw).all() and err <= tol


def _assemble_case(M, seed):
    from test_gpu_gradient_native import _assemble_reference
    g = torch.Generator().manual_seed(seed)
    T, Hn, variance_idx, trace_idx = 3, 2, 1, [0]
    fy, tg, beta = H.crandn((M,), g), H.crandn((M,), g), H.crandn((M,), g)
    ws = torch.rand(M, generator=g, dtype=torch.float64).to(_CD)
    dp = H.crandn((M, Hn), g)
    fz = H.crandn((T, M), g)
    v = (torch.randint(0, 2, (T, M), generator=g) * 2 - 1).to(torch.float64)
    beta_all = H.crandn((2 * T, M), g)
    kw = dict(variance_idx=variance_idx, trace_idx=trace_idx, sigmasq=0.31, n_obs=12345.0, yy=2.5 * M, variance=1.7)
    ref = _assemble_reference(fy, tg, ws, beta, dp, fz, v, beta_all, variance_idx, trace_idx, 0.31, 12345.0, 2.5 * M, 1.7)
    dev_args = [t.cuda() for t in (fy, tg, ws, beta, dp, fz, v, beta_all)]
    return dev_args, kw, ref, Hn + 1


def _assemble_error(out, ref, nh):
    out = out.cpu()
    scale = float(max(ref[1].abs().max(), ref[2].abs().max()))
    err = max(float((out[q * nh:(q + 1) * nh] - ref[q]).abs().max()) for q in range(3)) / scale
    return max(err, abs(float(out[3 * nh]) - float(ref[3])) / abs(float(ref[3])))


@pytest.mark.parametrize("M", [4096, 4097])
def test_gradient_assemble_at_the_one_launch_limit(M):
    """M = 4096 is the last size of the one-launch kernel (1024 threads, four entries each), 4097 the first of the two launches."""
    from efgp_hip import gradient_assemble
    args, kw, ref, nh = _assemble_case(M, 55)
    out = gradient_assemble(*args, **kw)
    err = _assemble_error(out, ref, nh)
    print(f"\ngradient_assemble M = {M}: {err:.2e}")
    assert err < 1e-12
    assert torch.equal(out, gradient_assemble(*args, **kw))


@pytest.mark.parametrize("M", [529, 4096])
def test_gradient_assemble_two_launches_switch(M, monkeypatch):
    from efgp_hip import gradient_assemble
    args, kw, ref, nh = _assemble_case(M, 56)
    one = gradient_assemble(*args, **kw)
    monkeypatch.setenv("EFGP_ASSEMBLE_TWO_LAUNCHES", "1")
    two = gradient_assemble(*args, **kw)
    monkeypatch.delenv("EFGP_ASSEMBLE_TWO_LAUNCHES")
    e1, e2 = _assemble_error(one, ref, nh), _assemble_error(two, ref, nh)
    scale = float(max(ref[1].abs().max(), ref[2].abs().max()))
    between = float((one - two).abs().max()) / scale
    print(f"\ngradient_assemble M = {M}: one launch {e1:.2e}, two launches {e2:.2e}, between them {between:.2e}")
    assert e1 < 1e-12 and e2 < 1e-12 and between < 1e-12


# ------------------------------------------------------------------------------------------------------------------------------
# 6. first direct tests
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_complex,b_complex", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["real.real", "real.complex", "complex.real", "complex.complex"])
def test_vdot_real_against_the_exact_sum(a_complex, b_complex):
    """Re <a, b> against math.fsum of the exact products.  The kernel adds ceil(n / (2048 * 256)) products per thread, 6 + 2 levels
    of the workgroup's tree, and the host adds the workgroups' sums: the bound is that depth (+ 64 covers the fixed part) times one
    rounding of the sum of the magnitudes."""
    from efgp_hip import vdot_real
    g = torch.Generator().manual_seed(61 + 2 * a_complex + b_complex)
    for n in (0, 1, 255, 257, 524288, 524288 + 9):
        a, b = H.signed_wide(n, g, a_complex), H.signed_wide(n, g, b_complex)
        got = vdot_real(a.cuda(), b.cuda())
        exact, mag = H.exact_vdot_real(a, b)
        bound = (math.ceil(n / (2048 * 256)) + 64) * 2.0 ** -53 * mag
        print(f"\nvdot_real n = {n}: |got - exact| = {abs(got - exact):.3e}, bound {bound:.3e}, sum of magnitudes {mag:.3e}")
        assert abs(got - exact) <= bound, (n, got, exact)
        if n == 0:
            assert got == 0.0


@pytest.mark.parametrize("N", [1, 63, 257, 262144 + 3])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_point_set_bounds_are_the_extremes_bit_for_bit(d, N):
    """Column 0: both signs, duplicates, -0.0 and subnormals inside the range.  Column 1: no negative value and no +0.0, so the
    minimum is -0.0 itself above the subnormals' sign; column 2: the mirror image, -0.0 the maximum."""
    from efgp_hip import PointSet
    g = torch.Generator().manual_seed(70 + 10 * d + N % 7)
    tiny = 5e-324
    x = torch.rand(N, 3, generator=g, dtype=torch.float64) * 4 - 2
    x[:, 1] = x[:, 1].abs() + tiny
    x[:, 2] = -x[:, 2].abs() - tiny
    if N == 1:
        x[0] = torch.tensor([-0.0, tiny, -1.5], dtype=torch.float64)
    else:
        special = torch.tensor([[-0.0, -0.0, -0.0], [tiny, tiny, -tiny], [-tiny, 3 * tiny, -3 * tiny], [2.2e-308, 1e-310, -1e-310]], dtype=torch.float64)
        where = torch.randperm(N, generator=g)[:min(4, N - 1)]
        x[where] = special[:where.numel()]
        x[N // 2] = x[0]                                               # a duplicate point
        x[-1] = x[(N - 1) // 3]                                         # ... and one at the very end (the wrap's last element)
    x = x[:, :d].contiguous()
    lo, hi = PointSet(x.cuda()).bounds()
    ref_lo, ref_hi = x.min(0).values, x.max(0).values
    got_lo, got_hi = torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)
    print(f"\nPointSet.bounds d = {d}, N = {N}: lo {lo}, hi {hi}")
    assert torch.equal(H.bits(got_lo), H.bits(ref_lo)) and torch.equal(H.bits(got_hi), H.bits(ref_hi))


def test_attach_values_replaces_the_sorted_copy():
    from efgp_hip import NufftPlan, PointSet
    g = torch.Generator().manual_seed(80)
    N, h, tol, nm = 30000, 0.25, 1e-7, (23, 23)
    conv = (45, 45)
    x = (torch.rand(N, 2, generator=g, dtype=torch.float64) * 2 - 1).cuda()
    y1 = torch.randn(N, generator=g, dtype=torch.float64).cuda()
    y2 = (3.0 * torch.randn(N, generator=g, dtype=torch.float64)).cuda()
    pts = PointSet(x, values=y1)
    plan = NufftPlan(x, h, tol, points=pts)
    first = [t.clone() for t in plan.type1_pair(y1, nm, conv)]        # builds the layout's sorted level and its copy of y1
    pts.attach_values(y2)
    second = [t.clone() for t in plan.type1_pair(y2, nm, conv)]
    fresh_pts = PointSet(x, values=y2)
    fresh = NufftPlan(x, h, tol, points=fresh_pts).type1_pair(y2, nm, conv)
    plain = NufftPlan(x, h, tol).type1(y2, nm)
    err = float((second[0] - plain).abs().max() / plain.abs().max())
    print(f"\nattach_values: F* y2 on the re-used layout against a plan without a layout {err:.2e}")
    assert torch.equal(second[0], fresh[0]) and torch.equal(second[1], fresh[1])
    assert not torch.equal(second[0], first[0])
    assert err < 4 * tol


@pytest.mark.parametrize("d,mtot", [(1, 35), (2, 23), (3, 9)])
def test_variance_rows_and_contraction_with_complex_ws(d, mtot):
    """The formulas of test_variance_rows_and_contraction with a ws whose imaginary part is not zero (the w.y terms of both
    kernels), isotropic and per-axis; a per-axis call with equal axes gives the isotropic call's bits."""
    from efgp_hip import variance_contract, variance_rhs
    g = torch.Generator().manual_seed(90 + d)
    B, h = 37, 0.31
    M = mtot ** d
    x = torch.rand(B, d, generator=g, dtype=torch.float64) * 2 - 1
    ws = H.crandn((M,), g)
    gamma = H.crandn((B, M), g)
    xd, wsd, gd = x.cuda(), ws.cuda(), gamma.cuda()
    fx = H.features(x, (h,) * d, (mtot,) * d)
    ref_rhs = ws * fx.conj()                                                          # efgpnd.py:1805-1812
    ref_var = torch.real((fx * (ws * gamma)).sum(dim=-1)).clamp_min(0.0)              # efgpnd.py:1817-1820
    assert (ref_var == 0).any() and (ref_var > 0).any()
    rhs = variance_rhs(xd, h, mtot, wsd)
    out = variance_contract(xd, h, mtot, wsd, gd)
    e_rhs = float((rhs.cpu() - ref_rhs).abs().max())
    e_var = float((out.cpu() - ref_var).abs().max())
    print(f"\ncomplex ws, d = {d}, mtot = {mtot}: variance_rhs {e_rhs:.2e}, variance_contract {e_var:.2e}")
    assert e_rhs < 1e-12 * float(ws.abs().max())
    assert e_var < 1e-10 * float(ref_var.abs().max() + 1.0)
    assert bool(((out.cpu() == 0) == (ref_var == 0)).all())
    assert torch.equal(variance_rhs(xd, [h] * d, [mtot] * d, wsd), rhs)
    assert torch.equal(variance_contract(xd, [h] * d, [mtot] * d, wsd, gd), out)
    # unequal axes: the per-axis kernels against the same formulas
    shape, hs = tuple([mtot, 5, 3][:d]), (0.31, 0.17, 0.23)[:d]
    M2 = math.prod(shape)
    ws2, gamma2 = H.crandn((M2,), g), H.crandn((B, M2), g)
    fx2 = H.features(x, hs, shape)
    rhs2 = variance_rhs(xd, list(hs), list(shape), ws2.cuda()).cpu()
    out2 = variance_contract(xd, list(hs), list(shape), ws2.cuda(), gamma2.cuda()).cpu()
    ref2 = torch.real((fx2 * (ws2 * gamma2)).sum(dim=-1)).clamp_min(0.0)
    e2 = float((rhs2 - ws2 * fx2.conj()).abs().max())
    print(f"complex ws, per-axis {shape}: variance_rhs {e2:.2e}, variance_contract {float((out2 - ref2).abs().max()):.2e}")
    assert e2 < 1e-12 * float(ws2.abs().max())
    assert float((out2 - ref2).abs().max()) < 1e-10 * float(ref2.abs().max() + 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. NaN through the clamp
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_axis", [False, True], ids=["isotropic", "per_axis"])
def test_variance_contract_keeps_nan(per_axis):
    """clamp_min(0) keeps NaN (efgpnd.py:1817): a row of gamma that a failed solve left NaN must not come out as zero variance.
    The other rows keep their bits, and a negative sum is still 0."""
    from efgp_hip import variance_contract
    g = torch.Generator().manual_seed(95)
    d, B = 2, 9
    shape, hs = ((7, 7), (0.31, 0.31)) if not per_axis else ((7, 5), (0.31, 0.17))
    M = math.prod(shape)
    x = torch.rand(B, d, generator=g, dtype=torch.float64) * 2 - 1
    ws = H.crandn((M,), g)
    gamma = H.crandn((B, M), g)
    args = (list(hs), list(shape)) if per_axis else (hs[0], shape[0])
    clean = variance_contract(x.cuda(), args[0], args[1], ws.cuda(), gamma.cuda()).cpu()
    signed = torch.real((H.features(x, hs, shape) * (ws * gamma)).sum(dim=-1))
    assert (signed < 0).any() and (signed > 0).any()
    bad = gamma.clone()
    bad[4, M // 2] = complex(float("nan"), 0.0)
    out = variance_contract(x.cuda(), args[0], args[1], ws.cuda(), bad.cuda()).cpu()
    print(f"\nvariance_contract {'per-axis' if per_axis else 'isotropic'} with NaN in row 4: {out.tolist()}")
    assert math.isnan(float(out[4]))
    keep = [r for r in range(B) if r != 4]
    assert torch.equal(H.bits(out[keep]), H.bits(clean[keep]))
    assert bool((clean[signed < 0] == 0).all()) and bool((clean[signed > 0] > 0).all())
