"""GPU: the gather image of the small 2-D real type 2.

modes_to_grid_real_kernel writes the two halo-padded parity copies that interp_real2_pair_kernel keeps in LDS, and the
gather fills its LDS with a flat copy of them.  EFGP_NO_GATHER_IMAGE=1 selects the earlier route (complex fine grid,
every workgroup redoes wrap / split / shift); both store the same doubles, so the outputs must be identical bits.
Every case is also held to the exact NUDFT with the error measure and bar of tests/test_gpu_nufft.py (relative l2,
2 x tolerance).  Which route ran is read from the library: the image-mode grid launch is timed as "grid_image".

Points: h = 0.5, so the transform has period 2 in x and [0, 2] is one period that starts and ends ON the periodic wrap
of the fine grid.  The first points sit exactly on both ends of each axis and within half a cell of them (cells of the
grids used here are 2/32 ... 2/128 wide), so their stencils read the halo rows and columns; the rest are uniform.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 0.5
PERIOD = 1.0 / H
LDS_BYTES = 160 * 1024


def _rel(a, b):
    a = a.detach().cpu()
    b = b.detach().cpu()
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


def _edge_coords():
    eps = [PERIOD / 300, PERIOD / 140, PERIOD / 70]          # all within half a cell of a 32-cell grid, the first of a 128-cell one
    vals = [0.0, PERIOD]
    for e in eps:
        vals += [e, -e, PERIOD - e, PERIOD + e]
    return torch.tensor(vals, dtype=torch.float64)


_POINTS = {}


def _points(N):
    """(0, PERIOD) first (the N = 1 case), then every pair of edge coordinates, edge x random, random."""
    if N not in _POINTS:
        g = torch.Generator().manual_seed(1234)
        e = _edge_coords()
        corner = torch.tensor([[0.0, PERIOD]], dtype=torch.float64)
        pairs = torch.cartesian_prod(e, e)
        r = torch.rand(2 * e.numel(), generator=g, dtype=torch.float64) * PERIOD
        mixed = torch.cat([torch.stack([e, r[:e.numel()]], 1), torch.stack([r[e.numel():], e], 1)])
        special = torch.cat([corner, pairs, mixed])
        rest = torch.rand(max(N - special.shape[0], 0), 2, generator=g, dtype=torch.float64) * PERIOD
        _POINTS[N] = torch.cat([special, rest])[:N].contiguous()
    return _POINTS[N]


def _modes(nm, B=None, seed=6):
    g = torch.Generator().manual_seed(seed + 100 * nm[0] + nm[1])
    shape = tuple(nm) if B is None else (B,) + tuple(nm)
    return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))


def _geometry(nm, tol, dense=False):
    """(nf0, nf1, W, bytes of the two parity copies) by the library's own window rules."""
    from efgp_hip import lib
    nf = [int(lib().efgp_fine_grid_size_nd(int(m), tol, 2, int(dense))) for m in nm]
    W = int(lib().efgp_window_width_nd(tol, min(f / m for f, m in zip(nf, nm)), 2))
    p0, p1 = nf[0] + W - 1, (nf[1] + 2 * ((W + 1) // 2) + 1) & ~1
    return nf[0], nf[1], W, 2 * p0 * p1 * 8


def _expect_image(nm, tol, dense=False):
    nf0, nf1, W, nbytes = _geometry(nm, tol, dense)
    return max(nf0, nf1) <= 128 and max(nm) <= 64 and nbytes <= LDS_BYTES


def _reference(x, f, nm, isign, modeord, scale):
    from oracle import efgp_oracle as O
    fs = f if scale is None else f * scale
    if isign < 0:
        fs = fs.conj()          # Re sum f e^{-ikx} = Re sum conj(f) e^{+ikx}
    return O.nudft_type2(x, H, fs, tuple(nm), fft_order=bool(modeord)).real


def _both_routes(monkeypatch, x, f, nm, tol, isign=+1, modeord=0, scale=None):
    """-> (default route's output, image-mode grid launches it made, EFGP_NO_GATHER_IMAGE output, launches there)."""
    from efgp_hip import NufftPlan, kernel_timing, kernel_timing_read
    plan = NufftPlan(x.cuda(), H, tol)
    fd = f.cuda()
    sd = None if scale is None else scale.cuda()
    res = []
    try:
        for off in (False, True):
            if off:
                monkeypatch.setenv("EFGP_NO_GATHER_IMAGE", "1")
            else:
                monkeypatch.delenv("EFGP_NO_GATHER_IMAGE", raising=False)
            kernel_timing(True, only="grid_image")
            out = plan.type2(fd, tuple(nm), modeord=modeord, real_only=True, isign=isign, mode_scale=sd)
            res += [out, kernel_timing_read("grid_image")[1]]
    finally:
        kernel_timing(False)
        monkeypatch.delenv("EFGP_NO_GATHER_IMAGE", raising=False)
    return res


def _check(monkeypatch, N, nm, tol, image, isign=+1, modeord=0, scaled=False):
    x = _points(N)
    f = _modes(nm)
    scale = _modes(nm, seed=9) if scaled else None
    out, n_img, out_off, n_off = _both_routes(monkeypatch, x, f, nm, tol, isign, modeord, scale)
    assert n_img == (1 if image else 0) and n_off == 0
    assert out.shape == (N,) and torch.equal(out, out_off)
    assert _rel(out, _reference(x, f, nm, isign, modeord, scale)) < 2 * tol + 1e-13


def test_geometry_of_the_cases():
    """The sizes the cases below are chosen for."""
    assert _geometry((23, 23), 1e-7) == (64, 64, 8, 81792)               # the headline's image
    assert _geometry((5, 7), 1e-7)[:2] == (32, 32)                       # the smallest grids
    assert _geometry((23, 45), 1e-7)[:2] == (64, 128)                    # non-square
    assert _geometry((23, 23), 1e-6)[2] == 7                             # an odd width
    assert _geometry((23, 23), 1e-7, dense=True) == (90, 90, 7, 150528)  # the largest image in use
    assert _geometry((24, 24), 1e-7) == (64, 64, 8, 81792)
    nf0, nf1, W, nbytes = _geometry((32, 32), 1e-7)                      # beyond: the single-copy halo kernel
    assert (nf0, nf1) == (96, 96) and nbytes > LDS_BYTES and (nf0 + W - 1) * (nf1 + W - 1) * 8 <= LDS_BYTES


@pytest.mark.parametrize("N", [4097, 2047, 1])
@pytest.mark.parametrize("nm", [(23, 23), (5, 7), (24, 22), (23, 45)])
def test_image_route_equals_grid_route(N, nm, monkeypatch):
    """Two workgroups / one / a single point; square, smallest, even (the unpaired mode -nm/2) and non-square boxes.
    (23, 45) is 64 x 128 cells with W = 8: 2 * 71 * 136 * 8 = 154,496 B fit the LDS, so it takes the image route too."""
    assert _expect_image(nm, 1e-7)
    _check(monkeypatch, N, nm, 1e-7, image=True)


@pytest.mark.parametrize("isign,modeord,scaled", list(itertools.product([+1, -1], [0, 1], [False, True])))
def test_image_route_sign_order_scale(isign, modeord, scaled, monkeypatch):
    _check(monkeypatch, 4097, (24, 22), 1e-7, image=True, isign=isign, modeord=modeord, scaled=scaled)


def test_image_route_odd_width(monkeypatch):
    _check(monkeypatch, 4097, (23, 23), 1e-6, image=True)


def test_image_route_dense_plan(monkeypatch):
    """EFGP_DENSE_POINTS=1: a small plan takes the dense rule's 90 x 90 grid, W = 7 -- 150,528 B, the largest image in use."""
    monkeypatch.setenv("EFGP_DENSE_POINTS", "1")
    _check(monkeypatch, 4097, (23, 23), 1e-7, image=True)


@pytest.mark.parametrize("nm,image", [(24, True), (32, False)])
def test_boundary_between_pair_and_halo_gather(nm, image, monkeypatch):
    """nm 24: 64 cells, the image route.  nm 32: 96 cells, two copies exceed the LDS, the single-copy halo kernel runs."""
    assert _expect_image((nm, nm), 1e-7) == image
    _check(monkeypatch, 4097, (nm, nm), 1e-7, image=image)


def test_batched_rows_keep_the_grid_route(monkeypatch):
    """B = 3 real rows go through the FFT route and the pair kernel's own fill, whatever the switch says."""
    from efgp_hip import NufftPlan, kernel_timing, kernel_timing_read
    from oracle import efgp_oracle as O
    N, nm, tol = 4097, (23, 23), 1e-7
    x = _points(N)
    f = _modes(nm, B=3)
    plan = NufftPlan(x.cuda(), H, tol)
    try:
        kernel_timing(True, only="grid_image")
        out = plan.type2(f.cuda(), nm, real_only=True)
        assert kernel_timing_read("grid_image")[1] == 0
    finally:
        kernel_timing(False)
    monkeypatch.setenv("EFGP_NO_GATHER_IMAGE", "1")
    assert torch.equal(out, plan.type2(f.cuda(), nm, real_only=True))
    ref = torch.stack([O.nudft_type2(x, H, f[b], nm).real for b in range(3)])
    assert out.shape == (3, N) and _rel(out, ref) < 2 * tol + 1e-13
