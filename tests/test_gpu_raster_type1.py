"""The raster type-1 entry point (efgp_raster_type1 through efgp_hip.ops.raster_type1, and efgp_hip.RasterPlan on top of it)
against the exact sums of tests/_nudft.py at the meshgrid points.

Bound: max |out - exact| <= 1e-11 sum_j |values_j scale_j| per batch row, for inputs with h_a (m_a // 2) max |x - xcen_a| <= 70
(`_raster.make_case`, phase 70): the bound of the type-2 tests at the same phase range.  The worst phase rounding there is
2 pi 70 * 3 * 2^-53 = 1.5e-13 per term.  The shapes sit where the kernels can go wrong: last-axis lengths around the 4-cell
instruction step, the 16-cell trip and the 256-cell segment, row counts around the 16-row tile, leading axes around the 16-row reduction chunk, mode
counts around the 4-mode groups, the 16-column tile and the 64-column strip.
"""
import pytest
import torch

import _raster
import _raster_adjoint as _ra

pytestmark = pytest.mark.gpu

BOUND = 1e-11

# mode box, raster, per-axis h (power-of-two multiples of the first), modeord, isign, nbatch, cell scale ("", "scale", "mask", "both"), xcen
CASES = [
    ((1,), (1,), (1.0,), 0, -1, 1, "", True),
    ((4,), (3,), (1.0,), 1, +1, 1, "scale", False),
    ((16,), (4,), (1.0,), 0, -1, 3, "", True),
    ((17,), (5,), (1.0,), 1, -1, 1, "mask", True),
    ((23,), (16,), (1.0,), 0, +1, 1, "", False),
    ((67,), (17,), (1.0,), 0, -1, 3, "both", True),                      # two column strips
    ((4,), (33,), (1.0,), 1, -1, 1, "", False),
    ((201,), (257,), (1.0,), 0, -1, 3, "mask", False),                   # segment + 1 cells: two GEMM segments
    ((9,), (255,), (1.0,), 1, -1, 1, "", True),                          # segment - 1
    ((9,), (256,), (1.0,), 0, +1, 1, "scale", False),                    # one full segment
    ((5, 6), (3, 513), (1.0, 1.0), 0, -1, 3, "mask", True),              # 2 segments + 1 behind a leading axis
    ((3, 4, 5), (2, 3, 260), (1.0, 1.0, 1.0), 1, -1, 1, "both", False),  # segments behind two leading axes
    ((4, 16), (1, 3), (1.0, 1.0), 0, -1, 1, "", True),                   # one row
    ((23, 5), (15, 17), (1.0, 0.5), 0, -1, 1, "mask", True),             # chunk - 1 rows
    ((16, 3), (16, 33), (1.0, 2.0), 1, +1, 3, "", False),                # chunk rows, three batches
    ((17, 4), (17, 5), (1.0, 1.0), 0, -1, 1, "scale", True),             # chunk + 1
    ((1, 23), (33, 16), (1.0, 0.25), 1, -1, 1, "both", False),           # 2 chunk + 1
    ((5, 4), (5, 4), (1.0, 1.0), 0, +1, 3, "", True),                    # 15 rows over three batches
    ((45, 45), (31, 18), (1.0, 1.0), 1, -1, 1, "mask", False),           # the lag box of m = 23, FFT order
    ((7, 4, 9), (5, 17, 3), (1.0, 0.5, 2.0), 0, -1, 3, "both", True),
    ((1, 2, 3), (16, 1, 2), (1.0, 1.0, 1.0), 1, +1, 1, "", False),
    ((13, 13, 13), (17, 9, 33), (1.0, 2.0, 0.5), 0, -1, 1, "mask", False),
    ((5, 17, 70), (33, 3, 4), (1.0, 1.0, 1.0), 1, -1, 1, "scale", True),     # two column strips behind two leading axes
]


def _inputs(case, seed, n_axis=None):
    shape, n0, hrel, modeord, isign, nbatch, kind, center = case
    return _ra.make_values(shape, n_axis or n0, hrel, seed, nbatch=nbatch, masked=0.25 if kind in ("mask", "both") else 0.0,
                           scaled=kind in ("scale", "both"), center=center)


def _call(case, inputs, **kw):
    from efgp_hip import ops
    shape, _, _, modeord, isign, nbatch, _, _ = case
    axes, hs, xcen, values, scale = inputs
    vv = values if nbatch > 1 else values[0]
    return ops.raster_type1([a.cuda() for a in axes], hs, shape, vv.cuda(), cell_scale=None if scale is None else scale.cuda(),
                            modeord=modeord, isign=isign, xcen=xcen, **kw)


def _rel_err(got, want, mag):
    B = want.shape[0]
    return ((got.cpu().reshape(want.shape) - want).abs().reshape(B, -1).max(dim=1).values / mag).max().item()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{c[1]}->{c[0]}".replace(" ", "") for c in CASES])
def test_entry_point_matches_the_exact_sums(case):
    shape, n_axis, hrel, modeord, isign, nbatch, kind, center = CASES[case]
    inputs = _inputs(CASES[case], seed=700 + case)
    got = _call(CASES[case], inputs)
    assert got.is_cuda and got.dtype == torch.complex128
    assert tuple(got.shape) == ((nbatch,) if nbatch > 1 else ()) + tuple(shape)
    axes, hs, xcen, values, scale = inputs
    want, mag = _ra.exact(axes, hs, values, shape, isign, modeord, xcen, scale)
    err = _rel_err(got, want, mag)
    print(f"\nraster {n_axis} -> {shape} modeord {modeord} isign {isign} nbatch {nbatch} {kind}: max err / sum|v s| = {err:.2e}")
    assert err <= BOUND


@pytest.mark.parametrize("shape,n_axis,hrel", [((23,), (37,), (1.0,)), ((9, 6), (18, 21), (1.0, 0.5)), ((5, 4, 7), (6, 17, 5), (1.0, 2.0, 1.0))],
                         ids=["1d", "2d", "3d"])
def test_adjoint_identity(shape, n_axis, hrel):
    """<raster_type2(f, isign=+1), V> = Re <f, raster_type1(V, isign=-1)> within 1e-11 sum|f| sum|V|."""
    from efgp_hip import ops
    axes, hs, xcen, f, _ = _raster.make_case(shape, n_axis, hrel, seed=31, nbatch=1, scale=False)
    g = torch.Generator().manual_seed(32)
    V = torch.randn(n_axis, dtype=torch.float64, generator=g)
    ax = [a.cuda() for a in axes]
    for modeord in (0, 1):
        lhs = (ops.raster_type2(ax, hs, shape, f[0].cuda(), isign=+1, modeord=modeord, xcen=xcen).cpu() * V).sum().item()
        t1 = ops.raster_type1(ax, hs, shape, V.cuda(), isign=-1, modeord=modeord, xcen=xcen).cpu()
        rhs = (f[0].conj() * t1).sum().conj().real.item()        # Re sum_k f_k conj(t1_k)
        tol = BOUND * f.abs().sum().item() * V.abs().sum().item()
        print(f"\nadjoint {n_axis} <-> {shape} modeord {modeord}: |lhs - rhs| = {abs(lhs - rhs):.2e}, bound {tol:.2e}")
        assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("case", [13, 19], ids=["2d", "3d"])
def test_masked_cells_are_selected_out(case):
    """NaN and Inf in cells of scale 0 leave no trace: the bits of the call with zeros there, and the exact sum over the rest."""
    shape, n_axis, hrel, modeord, isign, nbatch, kind, center = CASES[case]
    axes, hs, xcen, values, scale = _inputs(CASES[case], seed=41)
    dead = scale == 0
    assert 0 < int(dead.sum()) < dead.numel()
    clean = values.clone()
    clean[:, dead] = 0.0
    dirty = values.clone()
    dirty[:, dead] = float("nan")
    dirty[0][dead & (torch.arange(dead.numel()).reshape(dead.shape) % 2 == 0)] = float("inf")
    got_clean = _call(CASES[case], (axes, hs, xcen, clean, scale))
    got_dirty = _call(CASES[case], (axes, hs, xcen, dirty, scale))
    assert bool(torch.isfinite(torch.view_as_real(got_dirty)).all())
    assert torch.equal(torch.view_as_real(got_dirty), torch.view_as_real(got_clean))
    want, mag = _ra.exact(axes, hs, dirty, shape, isign, modeord, xcen, scale)
    err = _rel_err(got_dirty, want, mag)
    print(f"\nmasked raster {n_axis} -> {shape}: max err / sum|v s| = {err:.2e}")
    assert err <= BOUND


@pytest.mark.parametrize("case,n_axis", [(13, (50, 15)), (13, (40, 300)), (19, (40, 17, 3))], ids=["2d", "2d-segments", "3d"])
def test_repeatable_and_slab_seams_do_not_show(case, n_axis):
    """Two calls agree bitwise; a cap that cuts the leading axis into >= 3 slabs with a short last one gives the same bits."""
    from efgp_hip import ops
    shape, nbatch = CASES[case][0], CASES[case][5]
    inputs = _inputs(CASES[case], seed=77, n_axis=n_axis)
    one = _call(CASES[case], inputs)
    p0 = _ra.plan(shape, n_axis, nbatch)
    cap = p0["table_bytes"] + 16 * p0["row_bytes"]
    p = ops.raster_type1_plan(n_axis, shape, nbatch, cap)
    assert p["slabs"] >= 3 and n_axis[0] % p["slab_rows"] != 0 and p["workspace_bytes"] <= cap
    assert ops.raster_type1_plan(n_axis, shape, nbatch)["slabs"] == 1
    cut = _call(CASES[case], inputs, max_workspace_bytes=cap)
    again = _call(CASES[case], inputs)
    assert torch.equal(torch.view_as_real(again), torch.view_as_real(one))
    assert torch.equal(torch.view_as_real(cut), torch.view_as_real(one))
    axes, hs, xcen, values, scale = inputs
    want, mag = _ra.exact(axes, hs, values, shape, CASES[case][4], CASES[case][3], xcen, scale)
    err = _rel_err(cut, want, mag)
    print(f"\nraster {n_axis} -> {shape} in {p['slabs']} slabs: max err / sum|v s| = {err:.2e}")
    assert err <= BOUND


@pytest.mark.parametrize("n_modes,n_axis,hrel", [((5,), (19,), (1.0,)), ((4, 7), (18, 21), (1.0, 0.5)), ((3, 4, 5), (6, 17, 5), (1.0, 2.0, 1.0))],
                         ids=["1d", "2d", "3d"])
def test_separable_toeplitz_vector(n_modes, n_axis, hrel):
    """RasterPlan.type1_pair without a mask: the lag-box "ones" output (outer product of d one-dimensional sums) against
    raster_type1 of an all-ones raster, within 1e-11 prod n; the y output is raster_type1 of y, bitwise, and both are views of
    one buffer."""
    from efgp_hip import RasterPlan, ops
    lag = tuple(2 * m - 1 for m in n_modes)
    axes, hs, xcen, values, _ = _ra.make_values(lag, n_axis, hrel, seed=51)
    ax = [a.cuda() for a in axes]
    plan = RasterPlan(ax, hs, xcen=xcen)
    y = values[0].cuda()
    fy, v = plan.type1_pair(y, n_modes, lag)
    assert tuple(fy.shape) == tuple(n_modes) and tuple(v.shape) == lag
    assert fy.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()
    ones = torch.ones(n_axis, dtype=torch.float64, device="cuda")
    want_v = ops.raster_type1(ax, hs, lag, ones, xcen=xcen)
    err = (v - want_v).abs().max().item()
    ncells = 1
    for n in n_axis:
        ncells *= n
    print(f"\nseparable ones {n_axis} -> {lag}: max |diff| = {err:.2e}, bound {BOUND * ncells:.2e}")
    assert err <= BOUND * ncells
    assert torch.equal(torch.view_as_real(fy), torch.view_as_real(ops.raster_type1(ax, hs, n_modes, y, xcen=xcen)))
    assert torch.equal(torch.view_as_real(plan.type1_ones(lag)), torch.view_as_real(v))
    # with a mask the "ones" output is the raster transform of the mask
    mask = (torch.rand(n_axis, generator=torch.Generator().manual_seed(5)) > 0.3).to(torch.float64).cuda()
    mplan = RasterPlan(ax, hs, cell_scale=mask, xcen=xcen)
    _, mv = mplan.type1_pair(y, n_modes, lag)
    assert torch.equal(torch.view_as_real(mv), torch.view_as_real(ops.raster_type1(ax, hs, lag, mask, xcen=xcen)))


def test_generated_probes_are_the_filled_rows():
    """type1_rademacher / type1_normal are raster_type1 of the rows of rademacher_fill / normal_fill, bitwise, with the plan's
    mask, a non-zero index_offset and a batch count that spans two (and a half) blocks."""
    from efgp_hip import RasterPlan, normal_fill, ops, rademacher_fill
    n_modes, n_axis = (6, 5), (18, 21)
    axes, hs, xcen, _, scale = _ra.make_values(n_modes, n_axis, (1.0, 1.0), seed=61, masked=0.2)
    ax = [a.cuda() for a in axes]
    plan = RasterPlan(ax, hs, cell_scale=scale.cuda(), xcen=xcen)
    ncells, T, dev = 18 * 21, 5, torch.device("cuda", torch.cuda.current_device())
    for off in (0, 12345):
        for fill, gen in ((rademacher_fill, plan.type1_rademacher), (normal_fill, plan.type1_normal)):
            plan.probe_block_bytes = 256 << 20
            want = ops.raster_type1(ax, hs, n_modes, fill(dev, 9, T, ncells, off).reshape((T,) + n_axis), cell_scale=scale.cuda(), xcen=xcen)
            whole = gen(9, T, n_modes, index_offset=off)
            plan.probe_block_bytes = 2 * 8 * ncells                   # two rows per block: blocks of 2, 2 and 1 rows
            assert len(plan._probe_blocks(T)) == 3
            blocks = gen(9, T, n_modes, index_offset=off)
            assert tuple(whole.shape) == (T,) + n_modes
            assert torch.equal(torch.view_as_real(whole), torch.view_as_real(want))
            assert torch.equal(torch.view_as_real(blocks), torch.view_as_real(want))


def test_raster_plan_type2_is_raster_type2():
    from efgp_hip import RasterPlan, ops
    shape, n_axis = (6, 5), (18, 21)
    axes, hs, xcen, f, sc = _raster.make_case(shape, n_axis, (1.0, 1.0), seed=71, nbatch=2)
    ax = [a.cuda() for a in axes]
    plan = RasterPlan(ax, hs, xcen=xcen)
    got = plan.type2(f.cuda(), shape, real_only=True, mode_scale=sc.cuda())
    want = ops.raster_type2(ax, hs, shape, f.cuda(), mode_scale=sc.cuda(), xcen=xcen)
    assert tuple(got.shape) == (2, 18 * 21) and torch.equal(got, want.reshape(2, -1))
    assert tuple(plan.type2(f[0].cuda(), shape, real_only=True).shape) == (18 * 21,)
    with pytest.raises(NotImplementedError, match="real"):
        plan.type2(f.cuda(), shape)


def test_argument_errors_launch_nothing():
    from efgp_hip import ops
    x = torch.linspace(0, 1, 5, dtype=torch.float64, device="cuda")
    v = torch.ones(5, 5, dtype=torch.float64, device="cuda")
    out = torch.full((3, 4), -7.25, dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError, match="axes"):
        ops.raster_type1([x, x, x, x], 0.5, (3, 4, 1, 1), v, out=out)
    with pytest.raises(ValueError, match="axes"):
        ops.raster_type1([], 0.5, (), v, out=out)
    with pytest.raises(ValueError, match="n_modes"):
        ops.raster_type1([x, x], 0.5, (3, 4, 1), v, out=out)
    with pytest.raises(ValueError, match="h has"):
        ops.raster_type1([x, x], (0.5, 0.5, 0.5), (3, 4), v, out=out)
    with pytest.raises(ValueError, match="values has"):
        ops.raster_type1([x, x], 0.5, (3, 4), torch.ones(5, 4, dtype=torch.float64, device="cuda"), out=out)
    with pytest.raises(ValueError, match="real"):
        ops.raster_type1([x, x], 0.5, (3, 4), v.to(torch.complex128), out=out)
    with pytest.raises(ValueError, match="cell_scale has"):
        ops.raster_type1([x, x], 0.5, (3, 4), v, cell_scale=torch.ones(5, 4, dtype=torch.float64, device="cuda"), out=out)
    for bad in (-1.0, float("nan"), float("inf")):
        sc = torch.ones(5, 5, dtype=torch.float64, device="cuda")
        sc[2, 3] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            ops.raster_type1([x, x], 0.5, (3, 4), v, cell_scale=sc, out=out)
    with pytest.raises(ValueError, match="xcen"):
        ops.raster_type1([x, x], 0.5, (3, 4), v, xcen=(0.0,), out=out)
    with pytest.raises(ValueError, match="isign"):
        ops.raster_type1([x, x], 0.5, (3, 4), v, isign=0, out=out)
    with pytest.raises(ValueError, match="out must be"):
        ops.raster_type1([x, x], 0.5, (3, 4), v, out=out[:2])
    least = _ra.plan((3, 4), (5, 5))["least_bytes"]
    with pytest.raises(ValueError, match=str(least)):
        ops.raster_type1([x, x], 0.5, (3, 4), v, max_workspace_bytes=least - 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    # the C entry refuses dim 0 and 4 itself, before any launch
    import ctypes as C
    from efgp_hip import lib
    one = (C.c_int64 * 4)(1, 1, 1, 1)
    hs = (C.c_double * 4)(0.5, 0.5, 0.5, 0.5)
    for dim in (0, 4):
        rc = lib().efgp_raster_type1(0, dim, one, hs, None, one, C.c_void_p(x.data_ptr()), C.c_void_p(v.data_ptr()), None, 1, -1, 0,
                                     C.c_void_p(out.data_ptr()), 0, None)
        assert rc == -1 and b"dim must be 1, 2 or 3" in lib().efgp_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    ops.raster_type1([x, x], 0.5, (3, 4), v, max_workspace_bytes=least, out=out)          # the smallest cap works
    assert not bool((out == -7.25).any())
