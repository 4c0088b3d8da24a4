"""Host: the exact reference tests/_nudft.py against the oracle and against the identities it must not be built from, and the
geometry of the named cases of tests/test_gpu_nufft_options.py by the library's own window rules (no GPU needed: both
efgp_fine_grid_size_nd and efgp_window_width_nd are host functions)."""
import itertools

import pytest
import torch

import _nudft as E
import _nufft_routes as R
from oracle import efgp_oracle as O

BOXES = [(6,), (5, 8), (4, 7, 6)]
H = 0.43


def _err(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _data(shape, N=57, B=None, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    d = len(shape)
    x = (torch.rand(N, d, generator=g, dtype=torch.float64) - 0.3) * 5.0          # several periods (1 / H = 2.3)
    cs = (N,) if B is None else (B, N)
    fs = tuple(shape) if B is None else (B,) + tuple(shape)
    c = torch.complex(torch.randn(cs, generator=g, dtype=torch.float64), torch.randn(cs, generator=g, dtype=torch.float64))
    f = torch.complex(torch.randn(fs, generator=g, dtype=torch.float64), torch.randn(fs, generator=g, dtype=torch.float64))
    return x, c, f


@pytest.mark.parametrize("shape", BOXES + [(7, 7)])
@pytest.mark.parametrize("B", [None, 3])
def test_defaults_equal_the_oracle(shape, B):
    x, c, f = _data(shape, B=B)
    assert E.type1(x, H, c, shape).shape == O.nudft_type1(x, H, c, shape).shape
    assert _err(E.type1(x, H, c, shape), O.nudft_type1(x, H, c, shape)) < 1e-13
    assert _err(E.type1(x, H, c.real, shape), O.nudft_type1(x, H, c.real, shape)) < 1e-13
    assert E.type2(x, H, f, shape).shape == O.nudft_type2(x, H, f, shape).shape
    assert _err(E.type2(x, H, f, shape), O.nudft_type2(x, H, f, shape)) < 1e-13
    assert _err(E.type2(x, H, f, shape, modeord=1), O.nudft_type2(x, H, f, shape, fft_order=True)) < 1e-13
    assert _err(E.type2(x, H, f, shape, chunk=10), O.nudft_type2(x, H, f, shape)) < 1e-13      # chunked over the points
    assert _err(E.type1(x, H, c, shape, chunk=10), O.nudft_type1(x, H, c, shape)) < 1e-13


def test_one_mode_at_a_time():
    """A single non-zero mode k of a (5, 8) box is the plane wave exp(isign 2 pi i h k.(x - xcen)): fixes which k a slot holds."""
    shape, xcen = (5, 8), (0.3, -1.1)
    x, _, _ = _data(shape)
    for modeord, isign in itertools.product((0, 1), (-1, 1)):
        k0, k1 = E.mode_numbers(5, modeord), E.mode_numbers(8, modeord)
        assert sorted(k0.tolist()) == [-2, -1, 0, 1, 2] and sorted(k1.tolist()) == [-4, -3, -2, -1, 0, 1, 2, 3]
        assert (k0[0], k1[0]) == ((0, 0) if modeord else (-2, -4))
        for s0, s1 in [(0, 0), (4, 7), (2, 4), (3, 1)]:
            f = torch.zeros(shape, dtype=torch.complex128)
            f[s0, s1] = 1.0
            ang = 2 * torch.pi * H * (float(k0[s0]) * (x[:, 0] - xcen[0]) + float(k1[s1]) * (x[:, 1] - xcen[1]))
            wave = torch.complex(torch.cos(ang), isign * torch.sin(ang))
            assert _err(E.type2(x, H, f, shape, isign=isign, modeord=modeord, xcen=xcen), wave) < 1e-13
            c = torch.zeros(x.shape[0], dtype=torch.complex128)
            c[5] = 2.0
            assert abs(complex(E.type1(x, H, c, shape, isign=isign, modeord=modeord, xcen=xcen)[s0, s1] - 2.0 * wave[5])) < 1e-13


@pytest.mark.parametrize("shape", BOXES)
def test_identities(shape):
    x, c, f = _data(shape, B=2, seed=3)
    axes = tuple(range(1, 1 + len(shape)))
    xcen = tuple(0.37 * (a + 1) for a in range(len(shape)))
    shifted = x - torch.tensor(xcen, dtype=torch.float64)
    scale = _data(shape, seed=8)[2]
    # isign = +1 is the conjugate of the default transform of the conjugated strengths
    assert _err(E.type1(x, H, c, shape, isign=+1), E.type1(x, H, c.conj(), shape).conj()) < 1e-13
    assert _err(E.type2(x, H, f, shape, isign=-1), E.type2(x, H, f.conj(), shape).conj()) < 1e-13
    # modeord = 1 is ifftshift over the mode axes
    for isign in (-1, 1):
        assert _err(E.type1(x, H, c, shape, isign=isign, modeord=1), torch.fft.ifftshift(E.type1(x, H, c, shape, isign=isign), dim=axes)) < 1e-13
        assert _err(E.type2(x, H, torch.fft.ifftshift(f, dim=axes), shape, isign=isign, modeord=1), E.type2(x, H, f, shape, isign=isign)) < 1e-13
    # xcen is a shift of the points
    assert _err(E.type1(x, H, c, shape, xcen=xcen), E.type1(shifted, H, c, shape)) < 1e-13
    assert _err(E.type2(x, H, f, shape, xcen=xcen), E.type2(shifted, H, f, shape)) < 1e-13
    # mode_scale multiplies the modes of every row
    assert _err(E.type2(x, H, f, shape, mode_scale=scale.reshape(-1)), E.type2(x, H, f * scale[None], shape)) < 1e-13
    # adjointness at matching signs: <type1(c), f> = <c, type2(f)>
    for isign, modeord in itertools.product((-1, 1), (0, 1)):
        lhs = torch.vdot(E.type1(x, H, c[0], shape, isign=isign, modeord=modeord, xcen=xcen).reshape(-1), f[0].reshape(-1))
        rhs = torch.vdot(c[0], E.type2(x, H, f[0], shape, isign=-isign, modeord=modeord, xcen=xcen))
        assert abs(complex(lhs - rhs)) < 1e-12 * abs(complex(rhs))


def test_geometry_of_the_cases():
    """Every named case lands on the route it is named for, by the restated predicates of the host dispatch on the window the
    library reports.  The sizes asserted first are the ones the cases were chosen for."""
    W = R.window
    assert W((23, 45), 1e-7) == ((64, 128), 8)
    assert W((40, 33), 1e-9) == ((96, 96), 10)
    assert W((12, 19), 1e-12) == ((32, 48), 13)
    assert W((33, 40), 1e-7) == ((96, 96), 8)
    assert W((40, 70), 1e-7) == ((96, 192), 8) and W((40, 70), 1e-6) == ((96, 192), 7)
    assert W((30, 45), 1e-7) == ((96, 128), 8)
    assert W((45, 70), 1e-7) == ((128, 192), 8)
    assert W((10, 13, 16), 1e-5) == ((32, 32, 48), 6)
    assert W((21, 12, 9), 1e-6) == ((48, 32, 32), 7)
    assert W((22, 45), 1e-7) == ((48, 128), 8)
    assert W((17, 29), 1e-7) == ((48, 64), 8) and W((33, 57), 1e-7) == ((96, 128), 8)
    assert W((23, 23), 1e-7, dense=True) == ((90, 90), 7) and W((45, 45), 1e-7, dense=True) == ((180, 180), 7)
    assert W((36,), 1e-7) == ((96,), 8) and W((35,), 1e-7) == ((96,), 8)

    for name, (nm, tol, N, cplx, h, expect, kw) in R.TYPE1.items():
        assert R.type1_route(nm, tol, N, 2 if cplx else 1, span_periods=R.SPAN_PERIODS, **kw) == expect, name
    for name, (nm, tol, N, B, real_only, h, expect) in R.TYPE2.items():
        assert R.type2_route(nm, tol, N, B or 1, real_only) == expect, name
    assert any(all(m % 2 == 0 for m in c[0]) for c in R.TYPE2.values() if c[4])                            # all axes even
    assert any(len(c[0]) == 3 and sum(m % 2 == 0 for m in c[0]) == 1 for c in R.TYPE2.values() if c[4])    # one even axis in 3-D

    # the margins the LDS cases sit on
    assert 2 * 64 * (128 + 7) * 8 + 4608 <= R.LDS_BYTES                                  # (23, 45): padded two-channel rows fit
    assert 2 * 96 * 96 * 8 <= R.LDS_BYTES < 2 * 96 * (96 + 9) * 8 + 4608                 # (40, 33): the grid fits, its padded rows do not
    assert 96 * 192 * 8 <= R.LDS_BYTES < 103 * 199 * 8                                   # (40, 70): the real grid fits, its halo copy does not
    assert R.type2_route((40, 70), 1e-6, 3000, 1, True) == ("pruned", "halo")            # ... one cell narrower it does
    assert 103 * 103 * 8 <= R.LDS_BYTES < 2 * 103 * 104 * 8                              # (33, 40): one halo copy fits, two parity copies do not
    assert 2 * 71 * 136 * 8 == 154496 <= R.LDS_BYTES                                     # (23, 45): the pair image fits
    assert 1000 * 2.0 ** -47 > 0.01 * 1e-12                                              # (12, 19) at 1e-12: no 48-bit raw sums
    # the int64 accumulator is read by the pruned transform only where grid-to-modes refuses: an axis with more than 32 modes a side
    assert 70 // 2 > R.G2M_MAX_H >= 45 // 2

    # tiles: each axis gets its own tile count and size; (45, 70) tiles along axis 1 only and still has T[0] > 1 (class order)
    assert R.tile_geom((128, 192), 8, 1) == ((1, 2), (128, 96))
    assert R.tile_geom((96, 128), 8, 2) == ((2, 2), (48, 64))
    assert R.tile_geom((48, 32, 32), 7, 1) == ((3, 2, 2), (16, 16, 16))
    assert R.tile_geom((48, 32, 32), 7, 2) == ((4, 3, 3), (12, 11, 11))
    assert 65536 >= R.ORDER_WINDOW * 16 > 32768                                          # tile_class_order_kernel: only the 65536-point case

    # the layout: both forced band heights find a level at the cases' N; unforced these point counts are below 24 points per run
    assert R.band_level((64, 128), 32768, R.SPAN_PERIODS, 8) == 32 and R.band_level((64, 128), 32768, R.SPAN_PERIODS, 1) == 256
    assert R.band_level((128, 192), 32768, R.SPAN_PERIODS, 8) == 32
    assert R.band_level((128, 192), 32768, R.SPAN_PERIODS, 1) is None and R.band_level((128, 192), 40960, R.SPAN_PERIODS, 1) == 256
    assert R.band_level((180, 180), 32768, R.SPAN_PERIODS, 8) == 32

    # the dense rule's cases
    assert R.type1_route((23, 23), 1e-7, 3000, 2, dense=True) == ("lds_pad_raw48", "g2m")
    assert R.type1_route((45, 45), 1e-7, 3000, 1, dense=True) == ("global", "g2m")
    assert R.type1_route((45, 45), 1e-7, 32768, 1, dense=True, layout_band=8, span_periods=R.SPAN_PERIODS) == ("layout", "g2m")
    assert R.type2_route((23, 23), 1e-7, 3000, 1, False, dense=True) == ("pruned", "lds")
    assert R.type2_route((45, 45), 1e-7, 3000, 1, False, dense=True) == ("pruned", "l2")
    assert R.type2_route((23, 23), 1e-7, 3000, 2, True, dense=True) == ("pruned", "pair")
    assert R.type2_route((45, 45), 1e-7, 3000, 2, True, dense=True) == ("pruned", "l2")

    # the switches
    assert R.type1_route((45, 70), 1e-7, 32768, 1, env=("EFGP_NO_PRUNED_FFT",)) == ("tiles", "fft")
    assert R.type1_route((45, 70), 1e-7, 32768, 1, env=("EFGP_NO_FFT_FROM_ACC",)) == ("tiles", "pruned")
    assert R.type1_route((21, 12, 9), 1e-6, 32768, 1, env=("EFGP_NO_PRUNED_FFT",)) == ("tiles", "fft")
    assert R.type1_route((21, 12, 9), 1e-6, 32768, 1, env=("EFGP_NO_FFT_FROM_ACC",)) == ("tiles", "pruned")
    assert R.type2_route((45, 70), 1e-7, 32768, 1, True, env=("EFGP_NO_PRUNED_FFT",)) == ("fft", "tiles")
    assert R.type2_route((21, 12, 9), 1e-6, 32768, 1, True, env=("EFGP_NO_PRUNED_FFT",)) == ("fft", "tiles")
    assert R.type1_route((23, 45), 1e-7, 3000, 2, env=("EFGP_NO_PAD",)) == ("lds_plain", "g2m")
    assert R.type2_route((33, 40), 1e-7, 3000, 1, True, env=("EFGP_NO_HALO",)) == ("direct", "lds")
    assert R.type2_route((23, 45), 1e-7, 3000, 1, True) == ("image", "pair")
    assert R.type2_route((23, 45), 1e-7, 3000, 1, True, env=("EFGP_NO_PAIR_GATHER",)) == ("direct", "halo")
    assert R.type2_route((33, 40), 1e-7, 3000, 1, True, env=("EFGP_NO_DIRECT_DFT",)) == ("pruned", "halo")
