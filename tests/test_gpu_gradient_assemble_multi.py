"""efgp_gradient_assemble_multi (csrc/multi_output.hip) through the C ABI wrapper, against the single-output entry it generalises.

The entry adds, per output row, the inner products of efgp_gradient_assemble and combines them into the gradient of the joint
objective: data entries (term2, y.alpha, the data part of the variance entry) summed over the rows, trace entries (term1) counted
nrows times.  Both entries are float64 reductions of the same products in different orders, so they agree within the reduction
bound  2 * nrows * M * 2^-53 * (sum of the absolute values of the terms that enter an entry)  -- `_abs_terms` forms those sums on the
host.  Bitwise: repeatability, and invariance under exact power-of-two row scales.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

_CD = torch.complex128
U = 2.0 ** -53
SIG, N_OBS, VARIANCE, T = 0.31, 777.0, 1.7, 3


def _herm(shape, g):
    """Rows that are Fourier coefficients of real functions on the symmetric mode grid: u[-k] = conj u[k]."""
    a = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))
    return 0.5 * (a + a.flip(-1).conj())


def _inputs(M, nrows, H, K, seed):
    g = torch.Generator().manual_seed(seed)
    fy, tg, beta = _herm((nrows, M), g), _herm((nrows, M), g), _herm((nrows, M), g)
    w = torch.rand(M, generator=g, dtype=torch.float64)
    ws = (0.5 * (w + w.flip(0))).to(_CD)
    d = torch.randn((M, H), generator=g, dtype=torch.float64)
    dp = (0.5 * (d + d.flip(0))).to(_CD)
    fz = _herm((T, M), g)
    v = (torch.randint(0, 2, (T, M), generator=g) * 2 - 1).to(torch.float64)
    beta_all = _herm(((K + 1) * T, M), g)
    yy = (2.0 + torch.rand(nrows, generator=g, dtype=torch.float64)) * M
    variance_idx = None if K == H else H - 1            # n_trace = H: every hyper traced; n_trace = 0: the last is the variance
    trace_idx = list(range(K))
    return dict(fy=fy, tg=tg, ws=ws, beta=beta, dp=dp, fz=fz, v=v, beta_all=beta_all, yy=yy, variance_idx=variance_idx,
                trace_idx=trace_idx, H=H, K=K, M=M, nrows=nrows)


def _multi(p, row_scale=None, fy=None, tg=None, beta=None, yy=None):
    from efgp_hip import gradient_assemble_multi
    c = lambda t: t.cuda().contiguous()
    rs = torch.ones(p["nrows"], dtype=torch.float64) if row_scale is None else row_scale
    out, rows = gradient_assemble_multi(c(p["fy"] if fy is None else fy), c(p["tg"] if tg is None else tg), c(p["ws"]),
                                        c(p["beta"] if beta is None else beta), c(p["dp"]), c(p["fz"]) if p["K"] else None, c(p["v"]),
                                        c(p["beta_all"]), variance_idx=p["variance_idx"], trace_idx=p["trace_idx"], sigmasq=SIG,
                                        n_obs=N_OBS, yy=c(p["yy"] if yy is None else yy), row_scale=c(rs), variance=VARIANCE)
    return out, rows


def _single(p, b):
    from efgp_hip import gradient_assemble
    c = lambda t: t.cuda().contiguous()
    return gradient_assemble(c(p["fy"][b]), c(p["tg"][b]), c(p["ws"]), c(p["beta"][b]), c(p["dp"]), c(p["fz"]) if p["K"] else None,
                             c(p["v"]), c(p["beta_all"]), variance_idx=p["variance_idx"], trace_idx=p["trace_idx"], sigmasq=SIG,
                             n_obs=N_OBS, yy=float(p["yy"][b]), variance=VARIANCE).cpu()


def _abs_terms(p):
    """For every entry of `out` and `rows_out`: the sum of the absolute values of the terms it is a sum of."""
    H, K, nrows = p["H"], p["K"], p["nrows"]
    nh = H + 1
    ws, dp = p["ws"], p["dp"]
    g = ws[None, :] * p["beta"]
    fa2 = ((p["fy"] - p["tg"]) / SIG).abs() ** 2
    t2 = torch.stack([(dp[:, i].real.abs()[None, :] * fa2).sum(1) for i in range(H)], 1) if H else torch.zeros((nrows, 0))   # (rows, H)
    yz = (p["fy"].real * g.real).abs().sum(1) + (p["fy"].imag * g.imag).abs().sum(1)
    zz = (g.real * p["tg"].real).abs().sum(1) + (g.imag * p["tg"].imag).abs().sum(1)
    a_norm = (p["yy"].abs() + 2 * yz + zz) / SIG ** 2
    y_alpha = (p["yy"].abs() + yz) / SIG
    rows = torch.stack([yz, zz, y_alpha, a_norm], 1)
    term1, term2 = torch.zeros(nh, dtype=torch.float64), torch.zeros(nh, dtype=torch.float64)
    term2[:H] = t2.sum(0)
    term2[H] = a_norm.sum()
    fz = p["fz"]
    for s, ki in enumerate(p["trace_idx"]):
        bk = p["beta_all"][s * T:(s + 1) * T]
        inner = (dp[:, ki].abs()[None, :] * fz.abs() + ws.abs()[None, :] * bk.abs()) * 2
        term1[ki] = nrows * (fz.abs() * inner).sum() / SIG / T
    noise = N_OBS / SIG + (p["v"] * p["beta_all"][K * T:].real).abs().sum() / SIG / T
    term1[H] = nrows * noise
    if p["variance_idx"] is not None:
        term2[p["variance_idx"]] = (y_alpha.sum() + SIG * a_norm.sum()) / VARIANCE
        term1[p["variance_idx"]] = nrows * (N_OBS + SIG * noise) / VARIANCE
    return torch.cat([0.5 * (term1 + term2), term1, term2, y_alpha.sum().reshape(1)]), rows


@pytest.mark.parametrize("ntrace_all", [False, True])
@pytest.mark.parametrize("H", [1, 2, 3])
@pytest.mark.parametrize("nrows", [1, 2, 3, 7])
@pytest.mark.parametrize("M", [9, 529, 4225])        # one launch; 23^2; two launches (beyond 4096)
def test_joint_entries_are_the_sums_of_single_row_calls(M, nrows, H, ntrace_all):
    K = H if ntrace_all else 0
    p = _inputs(M, nrows, H, K, seed=M + 10 * nrows + 100 * H + K)
    nh = H + 1
    out_d, rows_d = _multi(p)
    out2_d, rows2_d = _multi(p)
    assert torch.equal(out_d, out2_d) and torch.equal(rows_d, rows2_d)            # fixed order: bitwise repeatable
    out, rows = out_d.cpu(), rows_d.cpu()
    singles = [_single(p, b) for b in range(nrows)]
    term1 = nrows * singles[0][nh:2 * nh]
    term2 = sum(s[2 * nh:3 * nh] for s in singles)
    want = torch.cat([0.5 * (term1 - term2), term1, term2, sum(s[3 * nh] for s in singles).reshape(1)])
    abs_out, abs_rows = _abs_terms(p)
    bound = 2 * nrows * M * U * abs_out
    diff = (out - want).abs()
    assert bool((diff <= bound).all()), f"out: difference {diff.tolist()} bound {bound.tolist()}"
    # rows_out: y.alpha and |alpha|^2 are entries of the single call; y.z and |z|^2 follow from them and yy
    y_alpha = torch.stack([s[3 * nh] for s in singles])
    a_norm = torch.stack([s[2 * nh + H] for s in singles])
    y_z = p["yy"] - SIG * y_alpha
    z_z = SIG ** 2 * a_norm - p["yy"] + 2 * y_z
    want_rows = torch.stack([y_z, z_z, y_alpha, a_norm], 1)
    # the derived columns inherit the bound of |alpha|^2 times sigma^4 (they are differences of the same terms)
    rb = 2 * nrows * M * U * torch.stack([abs_rows[:, 3] * SIG ** 2, abs_rows[:, 3] * SIG ** 2 * 3, abs_rows[:, 2], abs_rows[:, 3]], 1)
    rdiff = (rows - want_rows).abs()
    assert bool((rdiff <= rb).all()), f"rows_out: difference {rdiff.tolist()} bound {rb.tolist()}"
    if nrows == 1:                       # one plain row: the single-output entry's result
        assert bool(((out - singles[0]).abs() <= 2 * M * U * abs_out).all())


@pytest.mark.parametrize("M,nrows", [(9, 3), (529, 7), (529, 8), (4225, 3)])
def test_power_of_two_row_scales_are_exact(M, nrows):
    p = _inputs(M, nrows, 2, 2, seed=5 * M + nrows)
    out, rows = _multi(p)
    k = torch.tensor([3, -7, 20, 0, -31, 11, 64, -100][:nrows], dtype=torch.float64)
    s = torch.ldexp(torch.ones(nrows, dtype=torch.float64), k.to(torch.int32))
    out_s, rows_s = _multi(p, row_scale=s, fy=p["fy"] / s[:, None], tg=p["tg"] / s[:, None], beta=p["beta"] / s[:, None],
                           yy=p["yy"] / s / s)
    assert torch.equal(out, out_s) and torch.equal(rows, rows_s)


def test_launch_count_switch_gives_the_same_sums(monkeypatch):
    """nrows * M = 3703 takes one launch; the same call forced onto the two-launch path adds the same products in another order."""
    p = _inputs(529, 7, 2, 2, seed=3)
    one, rows_one = _multi(p)
    monkeypatch.setenv("EFGP_ASSEMBLE_TWO_LAUNCHES", "1")
    two, rows_two = _multi(p)
    abs_out, abs_rows = _abs_terms(p)
    assert bool(((one - two).abs().cpu() <= 2 * 7 * 529 * U * abs_out).all())
    assert bool(((rows_one - rows_two).abs().cpu() <= 2 * 7 * 529 * U * abs_rows).all())


def test_more_rows_than_a_grid_dimension_holds():
    """65600 rows: beyond the 65535 workgroups gridDim.y holds, the rows are strided inside the kernel."""
    nrows, M = 65600, 9
    p = _inputs(M, nrows, 1, 0, seed=9)
    out, rows = _multi(p)
    out, rows = out.cpu(), rows.cpu()
    g = p["ws"][None, :] * p["beta"]
    y_z = (p["fy"].conj() * g).sum(1).real
    z_z = (g.conj() * p["tg"]).sum(1).real
    y_alpha = (p["yy"] - y_z) / SIG
    a_norm = (p["yy"] - 2 * y_z + z_z) / SIG ** 2
    want = torch.stack([y_z, z_z, y_alpha, a_norm], 1)
    _, abs_rows = _abs_terms(p)
    assert bool(((rows - want).abs() <= 2 * M * U * abs_rows).all())
    # the joint y.alpha: 65600 numbers added in the kernel's order and in torch's
    assert abs(float(out[-1]) - float(y_alpha.sum())) <= 2 * nrows * M * U * float(abs_rows[:, 2].sum())


def test_data_terms_alone_without_probes():
    """v = None: rows_out, term2 and y.alpha as with probes; no trace estimate."""
    from efgp_hip import gradient_assemble_multi
    p = _inputs(529, 3, 2, 0, seed=4)
    full, rows_full = _multi(p)
    c = lambda t: t.cuda().contiguous()
    out, rows = gradient_assemble_multi(c(p["fy"]), c(p["tg"]), c(p["ws"]), c(p["beta"]), c(p["dp"]), None, None, None,
                                        variance_idx=p["variance_idx"], trace_idx=[], sigmasq=SIG, n_obs=N_OBS, yy=c(p["yy"]),
                                        row_scale=torch.ones(3, dtype=torch.float64).cuda(), variance=VARIANCE)
    assert torch.equal(rows, rows_full) and torch.equal(out[6:], full[6:])          # term2 | y.alpha
    assert bool(torch.isnan(out[4:6]).all())              # term1's estimated entries (variance, noise): no estimate without probes


def test_argument_checks():
    from efgp_hip import gradient_assemble_multi
    p = _inputs(81, 2, 1, 0, seed=1)
    c = lambda t: t.cuda().contiguous()
    kw = dict(variance_idx=0, trace_idx=[], sigmasq=SIG, n_obs=N_OBS, variance=VARIANCE)
    ones = torch.ones(2, dtype=torch.float64).cuda()
    with pytest.raises(ValueError):          # a single vector where rows are expected
        gradient_assemble_multi(c(p["fy"][0]), c(p["tg"][0]), c(p["ws"]), c(p["beta"][0]), c(p["dp"]), None, c(p["v"]), c(p["beta_all"]),
                                yy=ones, row_scale=ones, **kw)
    with pytest.raises(ValueError):          # yy on the host
        gradient_assemble_multi(c(p["fy"]), c(p["tg"]), c(p["ws"]), c(p["beta"]), c(p["dp"]), None, c(p["v"]), c(p["beta_all"]),
                                yy=p["yy"], row_scale=ones, **kw)
    with pytest.raises(ValueError):          # sigmasq must be positive
        gradient_assemble_multi(c(p["fy"]), c(p["tg"]), c(p["ws"]), c(p["beta"]), c(p["dp"]), None, c(p["v"]), c(p["beta_all"]),
                                yy=c(p["yy"]), row_scale=ones, **dict(kw, sigmasq=0.0))
