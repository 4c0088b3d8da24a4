"""GPU: the two arms of the three small DFT kernels give the same bits.

grid_rows_kernel, rows_modes_kernel (csrc/nufft.hip: accumulator -> modes of a small 2-D type 1) and
modes_to_grid_real_kernel (csrc/small_dft.hip: modes -> real fine grid of a small 2-D real type 2) read their LDS operands
in groups ahead of the multiply-adds and issue their memory loads in front of the twiddle tables; EFGP_SMALL_DFT_SERIAL=1
selects the first version's statement order inside the same kernels (read per call: one plan serves both arms).  Every sum
keeps its partition and its term order, so every output must be identical bits, on every box shape that takes another
path: groups of eight with and without a remainder, one and two passes of rows_modes_kernel (63 / 65 modes), the table on
waves of its own (4 nf1 <= 512) or not, both inputs of grid_rows_kernel (the int64 accumulator of the layout spreader,
from 32768 points on, and the complex grid of the other spreaders), the image and the plain grid of the type 2.
One output per box is also held to the exact sums (relative l2, 2 x tolerance, as tests/test_gpu_nufft.py).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = "EFGP_SMALL_DFT_SERIAL"


def _rel(a, b):
    a = a.detach().cpu()
    b = b.detach().cpu()
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


def _data(N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 2, generator=g, dtype=torch.float64) * 2 - 1
    y = torch.randn(N, generator=g, dtype=torch.float64)
    Z = torch.randn(5, N, generator=g, dtype=torch.float64)
    return x, y, Z


def _type1_calls(plan, yd, Z, Cx, nm, big):
    outs = list(plan.type1_pair(yd, nm, big))
    outs.append(plan.type1(Z, nm))                             # five real rows: two pair grids and a lone row
    outs.append(plan.type1(Cx, nm))                            # complex rows
    outs.append(plan.type1(Z[:4], nm, modeord=1))
    outs.append(plan.type1(Cx, nm, modeord=1, isign=1))
    outs.append(plan.type1(Cx, nm, modeord=0, isign=1))
    outs.append(plan.type1_rademacher(99, 5, nm, index_offset=3))
    outs.append(plan.type1_rademacher(99, 1, nm, modeord=1))
    outs.extend(plan.type1_pair(yd, nm, big))                  # again, after all of the above
    return outs


TYPE1_BOXES = [((23, 23), (45, 45), 0.31, 6e-8), ((17, 29), (33, 57), 0.22, 1e-5), ((8, 12), (15, 23), 0.9, 1e-9),
               ((63, 63), (63, 63), 0.12, 1e-5), ((65, 65), (65, 65), 0.12, 1e-5)]


def _type1_check(monkeypatch, N, layout, nm, big, h, tol):
    from efgp_hip import NufftPlan, PointSet
    from oracle import efgp_oracle as O
    x, y, Z = _data(N, 17 + N % 7)
    xd, yd, Zd = x.cuda(), y.cuda(), Z.cuda()
    Cx = torch.complex(Zd[:2], Zd[2:4]).contiguous()
    plan = NufftPlan(xd, h, tol, points=PointSet(xd, values=yd) if layout else None)
    monkeypatch.delenv(SWITCH, raising=False)
    a = _type1_calls(plan, yd, Zd, Cx, nm, big)
    monkeypatch.setenv(SWITCH, "1")
    b = _type1_calls(plan, yd, Zd, Cx, nm, big)
    monkeypatch.delenv(SWITCH)
    c = _type1_calls(plan, yd, Zd, Cx, nm, big)                # and back: the switch is read per call
    for u, v, w in zip(a, b, c):
        assert u.shape == v.shape and torch.equal(u, v) and torch.equal(u, w)
    assert torch.equal(a[0], a[-2]) and torch.equal(a[1], a[-1])       # the accumulator was left clean
    assert torch.equal(b[0], b[-2]) and torch.equal(b[1], b[-1])
    assert _rel(a[0], O.nudft_type1(x, h, y, nm)) < 2 * tol
    assert _rel(a[1], O.nudft_type1(x, h, torch.ones(N, dtype=torch.float64), big)) < 2 * tol


@pytest.mark.parametrize("nm,big,h,tol", TYPE1_BOXES)
@pytest.mark.parametrize("N,layout", [(4097, True), (3000, False)])
def test_type1_arms_equal_bits(N, layout, nm, big, h, tol, monkeypatch):
    """Few points, with and without a layout: the spreaders that reduce to a complex grid (grid_rows_kernel<true>)."""
    _type1_check(monkeypatch, N, layout, nm, big, h, tol)


@pytest.mark.parametrize("nm,big,h,tol", [TYPE1_BOXES[0], TYPE1_BOXES[-1]])
def test_type1_arms_equal_bits_from_the_accumulator(nm, big, h, tol, monkeypatch):
    """From 32768 points on a layout takes the MFMA spreader, whose int64 accumulator grid_rows_kernel<false> converts and
    clears (the fit's route): the headline's boxes, and the largest."""
    _type1_check(monkeypatch, 32769, True, nm, big, h, tol)


def _modes(nm, B=None, seed=6):
    g = torch.Generator().manual_seed(seed + 100 * nm[0] + nm[1])
    shape = tuple(nm) if B is None else (B,) + tuple(nm)
    return torch.complex(torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64))


def _exact2(x, h, f, nm, isign, modeord):
    from oracle import efgp_oracle as O
    fs = f.conj() if isign < 0 else f                           # Re sum f e^{-ikx} = Re sum conj(f) e^{+ikx}
    return O.nudft_type2(x, h, fs, tuple(nm), fft_order=bool(modeord)).real


_H2 = 0.5
_X2 = {}


def _points2(N=4097):
    if N not in _X2:
        g = torch.Generator().manual_seed(1234)
        x = torch.rand(N, 2, generator=g, dtype=torch.float64) / _H2          # one period, both ends of it included
        x[0] = torch.tensor([0.0, 1.0 / _H2], dtype=torch.float64)
        _X2[N] = (x, x.cuda())
    return _X2[N]


def _type2_arms(monkeypatch, plan, fd, nm, **kw):
    monkeypatch.delenv(SWITCH, raising=False)
    a = plan.type2(fd, nm, real_only=True, **kw)
    monkeypatch.setenv(SWITCH, "1")
    b = plan.type2(fd, nm, real_only=True, **kw)
    monkeypatch.delenv(SWITCH)
    assert torch.equal(a, b)
    return a


@pytest.mark.parametrize("nm,tol", [((23, 23), 1e-7), ((5, 7), 1e-7), ((24, 22), 1e-7), ((23, 45), 1e-7), ((23, 23), 1e-6)])
def test_type2_arms_equal_bits(nm, tol, monkeypatch):
    """Both signs and mode orders on every box; a mode scale on the even box; the plain fine grid (EFGP_NO_GATHER_IMAGE)
    and three rows at once (no dense DFT: the arms share every kernel) on the headline's."""
    from efgp_hip import NufftPlan
    x, xd = _points2()
    plan = NufftPlan(xd, _H2, tol)
    f = _modes(nm)
    fd = f.cuda()
    for isign in (+1, -1):
        for modeord in (0, 1):
            out = _type2_arms(monkeypatch, plan, fd, nm, isign=isign, modeord=modeord)
            assert _rel(out, _exact2(x, _H2, f, nm, isign, modeord)) < 2 * tol
    if nm == (24, 22):
        sc = _modes(nm, seed=9)
        out = _type2_arms(monkeypatch, plan, fd, nm, mode_scale=sc.cuda())
        assert _rel(out, _exact2(x, _H2, f * sc, nm, +1, 0)) < 2 * tol
    if nm == (23, 23) and tol == 1e-7:
        monkeypatch.setenv("EFGP_NO_GATHER_IMAGE", "1")
        out = _type2_arms(monkeypatch, plan, fd, nm)
        monkeypatch.delenv("EFGP_NO_GATHER_IMAGE")
        assert torch.equal(out, plan.type2(fd, nm, real_only=True))             # image and plain grid: the same doubles
        assert _rel(out, _exact2(x, _H2, f, nm, +1, 0)) < 2 * tol
        f3 = _modes(nm, B=3)
        out3 = _type2_arms(monkeypatch, plan, f3.cuda(), nm)
        for b in range(3):
            assert _rel(out3[b], _exact2(x, _H2, f3[b], nm, +1, 0)) < 2 * tol
