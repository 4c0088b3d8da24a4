"""The raster transform's entry point (efgp_raster_type2 through efgp_hip.ops.raster_type2) against the exact sums of
tests/_nudft.py at the meshgrid points.

Bound: max |out - exact| <= 1e-11 sum_k |f_k scale_k| for inputs with h_a (n_a // 2) max |x - xcen_a| <= 70.  The worst phase
rounding there is 2 pi 70 * 3 * 2^-53 = 1.5e-13 per term, so the bound has about 50x margin.  The shapes sit where the tiles can go
wrong: mode counts that are no multiple of 4, axis lengths 1, 15, 17, 33 against 16-wide tiles, more than one workgroup.
"""
import pytest
import torch

import _raster

pytestmark = pytest.mark.gpu

BOUND = 1e-11

# mode box, raster, per-axis h (power-of-two multiples of the first), modeord, isign, nbatch, mode_scale given, xcen given
CASES = [
    ((67,), (33,), (1.0,), 0, +1, 1, True, False),
    ((1,), (1,), (1.0,), 0, -1, 1, False, True),
    ((4,), (16,), (1.0,), 1, +1, 3, True, True),
    ((201,), (257,), (1.0,), 0, -1, 3, False, False),
    ((23, 5), (17, 15), (1.0, 0.5), 0, +1, 1, True, True),
    ((16, 3), (1, 33), (1.0, 2.0), 1, -1, 3, False, False),
    ((45, 45), (31, 18), (1.0, 1.0), 1, +1, 1, False, False),             # the lag box of m = 23, FFT order
    ((2, 64), (48, 16), (1.0, 0.25), 0, -1, 3, True, True),
    ((7, 4, 9), (5, 17, 3), (1.0, 0.5, 2.0), 0, +1, 3, True, True),
    ((1, 2, 3), (16, 1, 2), (1.0, 1.0, 1.0), 1, -1, 1, False, False),
    ((13, 13, 13), (20, 9, 33), (1.0, 2.0, 0.5), 0, +1, 1, True, False),
]


def _run(case, seed, n_axis=None, **kw):
    from efgp_hip import ops
    shape, n0, hrel, modeord, isign, nbatch, scale, center = case
    n_axis = n_axis or n0
    axes, hs, xcen, f, sc = _raster.make_case(shape, n_axis, hrel, seed=seed, nbatch=nbatch, scale=scale, center=center)
    ff = f if nbatch > 1 else f[0]
    got = ops.raster_type2([a.cuda() for a in axes], hs, shape, ff.cuda(), modeord=modeord, isign=isign,
                           mode_scale=None if sc is None else sc.cuda(), xcen=xcen, **kw)
    return got, (axes, hs, xcen, f, sc)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{c[0]}->{c[1]}".replace(" ", "") for c in CASES])
def test_entry_point_matches_the_exact_sums(case):
    shape, n_axis, hrel, modeord, isign, nbatch, scale, center = CASES[case]
    got, (axes, hs, xcen, f, sc) = _run(CASES[case], seed=500 + case)
    assert got.is_cuda and got.dtype == torch.float64
    assert tuple(got.shape) == ((nbatch,) if nbatch > 1 else ()) + tuple(n_axis)
    want, mag = _raster.exact(axes, hs, f, shape, isign, modeord, xcen, sc)
    err = ((got.cpu().reshape(want.shape) - want).abs().reshape(nbatch, -1).max(dim=1).values / mag).max().item()
    print(f"\nraster {shape} -> {n_axis} modeord {modeord} isign {isign} nbatch {nbatch}: max err / sum|f scale| = {err:.2e}")
    assert err <= BOUND


@pytest.mark.parametrize("case,n_axis", [(4, (50, 15)), (8, (40, 17, 3))], ids=["2d", "3d"])
def test_slab_seams_do_not_show(case, n_axis):
    """A cap that cuts the leading axis into >= 3 slabs with a short last one gives the bits of the default call."""
    from efgp_hip import ops
    shape, nbatch = CASES[case][0], CASES[case][5]
    one, (axes, hs, xcen, f, sc) = _run(CASES[case], seed=77, n_axis=n_axis)
    cap = _raster.plan(shape, n_axis, nbatch)["table_bytes"] + 16 * _raster.plan(shape, n_axis, nbatch)["row_bytes"]
    p = ops.raster_plan(n_axis, shape, nbatch, cap)
    assert p["slabs"] >= 3 and n_axis[0] % p["slab_rows"] != 0 and p["workspace_bytes"] <= cap
    assert ops.raster_plan(n_axis, shape, nbatch)["slabs"] == 1
    cut, _ = _run(CASES[case], seed=77, n_axis=n_axis, max_workspace_bytes=cap)
    again, _ = _run(CASES[case], seed=77, n_axis=n_axis)
    assert torch.equal(cut, one) and torch.equal(again, one)
    want, mag = _raster.exact(axes, hs, f, shape, CASES[case][4], CASES[case][3], xcen, sc)
    err = ((cut.cpu().reshape(want.shape) - want).abs().reshape(nbatch, -1).max(dim=1).values / mag).max().item()
    print(f"\nraster {shape} -> {n_axis} in {p['slabs']} slabs: max err / sum|f scale| = {err:.2e}")
    assert err <= BOUND


def test_a_cap_that_is_too_small_is_refused_before_any_launch():
    from efgp_hip import ops
    shape, n_axis = (23, 5), (50, 15)
    axes, hs, xcen, f, sc = _raster.make_case(shape, n_axis, (1.0, 1.0), seed=3)
    out = torch.full(n_axis, -7.25, dtype=torch.float64, device="cuda")
    least = _raster.plan(shape, n_axis)["least_bytes"]
    with pytest.raises(ValueError, match=str(least)):
        ops.raster_type2([a.cuda() for a in axes], hs, shape, f[0].cuda(), max_workspace_bytes=least - 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    ops.raster_type2([a.cuda() for a in axes], hs, shape, f[0].cuda(), max_workspace_bytes=least, out=out)     # the smallest cap works
    assert not bool((out == -7.25).any())


def test_argument_errors_name_the_argument():
    from efgp_hip import ops
    x = torch.linspace(0, 1, 5, dtype=torch.float64, device="cuda")
    f = torch.ones(3, 4, dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError, match="axes"):
        ops.raster_type2([x, x, x, x], 0.5, (3, 4, 1, 1), f)
    with pytest.raises(ValueError, match="axes"):
        ops.raster_type2([], 0.5, (), f)
    with pytest.raises(ValueError, match="n_modes"):
        ops.raster_type2([x, x], 0.5, (3, 4, 1), f)
    with pytest.raises(ValueError, match="h has"):
        ops.raster_type2([x, x], (0.5, 0.5, 0.5), (3, 4), f)
    with pytest.raises(ValueError, match=r"axes\[1\] must be 1-D"):
        ops.raster_type2([x, x.reshape(5, 1)], 0.5, (3, 4), f)
    with pytest.raises(ValueError, match=r"axes\[0\] is empty"):
        ops.raster_type2([x[:0], x], 0.5, (3, 4), f)
    with pytest.raises(ValueError, match="f has"):
        ops.raster_type2([x, x], 0.5, (3, 5), f)
    with pytest.raises(ValueError, match="mode_scale"):
        ops.raster_type2([x, x], 0.5, (3, 4), f, mode_scale=torch.ones(11, dtype=torch.complex128, device="cuda"))
    with pytest.raises(ValueError, match="xcen"):
        ops.raster_type2([x, x], 0.5, (3, 4), f, xcen=(0.0,))
    with pytest.raises(ValueError, match="isign"):
        ops.raster_type2([x, x], 0.5, (3, 4), f, isign=0)
    assert tuple(ops.raster_type2([x, x], 0.5, (3, 4), f).shape) == (5, 5)
