"""efgp_mode_jet_rows (csrc/mode_jet.hip) through `efgp_hip.mode_jet_rows`, against its formula in float64 torch on the CPU:

    out[b, 0, k] = s_k f[b, k],      out[b, 1 + a, k] = (2 pi h_a k_a) i (s_k f[b, k])

with k_a from tests/_nudft.mode_numbers.  Bound per entry: 8 * 2^-53 |reference entry| (complex moduli) -- one complex product at
sqrt(5) u, whether or not its multiply-adds are contracted, plus one real multiplication, with room.  Slots with k_a = 0 must hold
+0.0 + 0.0i, two calls must agree bit for bit, and 65600 rows must come out of the one launch whose grid holds fewer rows than that.
"""
import math

import pytest
import torch

import _nudft as E

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BOXES = [(1,), (9,), (8,), (23, 23), (6, 5), (1, 7), (9, 9, 9), (4, 5, 3)]
HS = (0.37, 0.21, 0.53)


def _mode_table(shape, modeord):
    """(d, M): k_a of every flat slot, row-major."""
    ks = [E.mode_numbers(n, modeord) for n in shape]
    return torch.stack([m.reshape(-1) for m in torch.meshgrid(*ks, indexing="ij")])


def _reference(f, shape, hs, scale, modeord):
    p = f if scale is None else f * scale[None, :]
    rows = [p]
    for a, ka in enumerate(_mode_table(shape, modeord)):
        t = (2.0 * math.pi * hs[a]) * ka
        rows.append(torch.complex(-(t[None, :] * p.imag), t[None, :] * p.real))
    return torch.stack(rows, dim=1)


def _inputs(shape, rows, seed):
    g = torch.Generator().manual_seed(seed)
    M = math.prod(shape)
    f = torch.complex(torch.randn(rows, M, generator=g, dtype=torch.float64), torch.randn(rows, M, generator=g, dtype=torch.float64))
    s = torch.complex(torch.rand(M, generator=g, dtype=torch.float64) + 0.5, torch.randn(M, generator=g, dtype=torch.float64))
    return f, s


def _check(got, ref, shape, modeord):
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.complex128
    err, mag = (got - ref).abs(), ref.abs()
    worst = float((err / mag.clamp_min(1e-300)).max())
    assert bool((err <= 8 * U * mag).all()), f"worst entry {worst / U:.2f} u"
    for a, ka in enumerate(_mode_table(shape, modeord)):
        z = got[:, 1 + a, ka == 0]
        assert z.numel() > 0
        assert bool((z.real == 0).all() and (z.imag == 0).all())
        assert not bool(torch.signbit(z.real).any() or torch.signbit(z.imag).any())          # +0.0, not -0.0
    return worst / U


@pytest.mark.parametrize("shape", BOXES, ids=lambda s: "x".join(map(str, s)))
def test_rows_match_the_formula(shape):
    from efgp_hip import mode_jet_rows
    d = len(shape)
    hs = HS[:d]
    worst = 0.0
    for rows in (1, 3):
        f, s = _inputs(shape, rows, 17 * rows + d)
        for modeord in (0, 1):
            for scale in (None, s):
                got = mode_jet_rows(f.cuda(), shape, hs, mode_scale=None if scale is None else scale.cuda(), modeord=modeord)
                again = mode_jet_rows(f.cuda(), shape, hs, mode_scale=None if scale is None else scale.cuda(), modeord=modeord)
                assert torch.equal(torch.view_as_real(got), torch.view_as_real(again))       # bitwise repeatable
                worst = max(worst, _check(got.cpu(), _reference(f, shape, hs, scale, modeord), shape, modeord))
    print(f"\nbox {shape}: worst entry {worst:.2f} u (bound 8 u)")


def test_one_spacing_and_a_single_row_vector():
    from efgp_hip import mode_jet_rows
    shape = (6, 5)
    f, s = _inputs(shape, 1, 5)
    got = mode_jet_rows(f[0].cuda(), shape, 0.29, mode_scale=s.cuda())
    assert tuple(got.shape) == (1, 3, 30)
    _check(got.cpu(), _reference(f, shape, (0.29, 0.29), s, 0), shape, 0)


def test_more_rows_than_the_grid_holds():
    """65600 rows of M = 9: beyond the 65535 of gridDim.y, and beyond the rows the bounded grid holds -- the rows wrap in the kernel."""
    from efgp_hip import mode_jet_rows
    shape, rows = (9,), 65600
    f, s = _inputs(shape, rows, 3)
    got = mode_jet_rows(f.cuda(), shape, HS[:1], mode_scale=s.cuda(), modeord=1).cpu()
    _check(got, _reference(f, shape, HS[:1], s, 1), shape, 1)


def test_zero_rows_and_refusals():
    from efgp_hip import mode_jet_rows
    out = mode_jet_rows(torch.zeros((0, 30), dtype=torch.complex128, device="cuda"), (6, 5), 0.3)
    assert tuple(out.shape) == (0, 3, 30)
    f = torch.zeros((2, 30), dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError, match="mode_scale has 29 entries, the mode box .* has 30"):
        mode_jet_rows(f, (6, 5), 0.3, mode_scale=torch.ones(29, dtype=torch.complex128, device="cuda"))
    with pytest.raises(ValueError, match="36 entries per row"):
        mode_jet_rows(f, (6, 6), 0.3)
    with pytest.raises(ValueError, match="1, 2 or 3"):
        mode_jet_rows(f, (1, 2, 3, 5), 0.3)
    with pytest.raises(ValueError, match="spacings"):
        mode_jet_rows(f, (6, 5), (0.3, 0.2, 0.1))
