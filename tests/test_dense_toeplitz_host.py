"""CPU checks of the dense reference of the CG tests (tests/_dense_toeplitz.py) and of the restated dispatch (tests/_cg_routes.py).

The dense block Toeplitz matrix is held to the oracle's FFT product on every dense case of tests/test_gpu_cg_routes.py, to the
point sums of the definition at two small shapes, and the oracle's CG driven by the dense matrix to the same CG driven by the FFT
product after three forced iterations.  Distances measured when this was written: apply at most 9e-16, three iterations at most
3.2e-15 (relative, 2-norm); the bounds below are 1e-13.
"""
import math

import pytest
import torch

import _cg_routes as R
import _dense_toeplitz as D


def _rel(a, b):
    return float(torch.linalg.norm((a - b).reshape(-1)) / torch.linalg.norm(b.reshape(-1)))


@pytest.fixture(autouse=True)
def _serial():
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


SHAPES = sorted({(ns, herm) for ns, herm, _ in R.DENSE.values()})


@pytest.mark.parametrize("ns,herm", SHAPES, ids=[f"{'x'.join(map(str, ns))}{'-herm' if h else ''}" for ns, h in SHAPES])
def test_dense_matrix_equals_fft_product_and_is_hermitian(ns, herm):
    from oracle import efgp_oracle as O
    s = D.system(ns, herm)
    T = D.dense_T(s["v"])
    M = math.prod(ns)
    assert T.shape == (M, M)
    assert torch.equal(T, T.conj().T)                              # v[-k] = conj v[k] by construction of the point sums
    To = O.Toeplitz(s["v"])
    assert tuple(To.fft_shape) == R.fft_shape(ns) and To.size == M
    g = torch.Generator().manual_seed(5)
    u = torch.complex(torch.randn(2, M, generator=g, dtype=torch.float64), torch.randn(2, M, generator=g, dtype=torch.float64))
    assert _rel(D.matvec(T)(u), To(u)) < 1e-13
    if herm:                                                       # the Hermitian systems are what they say
        shape = (-1,) + tuple(ns)
        dims = tuple(range(1, len(ns) + 1))
        assert torch.equal(s["ws"].reshape(shape), s["ws"].reshape(shape).flip(dims)) and float(s["ws"].imag.abs().max()) == 0.0
        for t in (s["b"], s["x0"]):
            assert _rel(t.reshape(shape).flip(dims).conj(), t.reshape(shape)) < 1e-15 or float(t.abs().max()) == 0.0


@pytest.mark.parametrize("ns", [(3, 4), (2, 3, 2)])
def test_dense_matrix_equals_the_point_sums(ns):
    """T[k, k'] = sum_p exp(-2 pi i h (k - k') . x_p), every entry, with k over the block in row-major order."""
    s = D.system(ns)
    x = s["points"]
    d = len(ns)
    k = torch.cartesian_prod(*[torch.arange(n, dtype=torch.float64) for n in ns]).reshape(-1, d)
    h = torch.tensor(D.H[:d], dtype=torch.float64)
    diff = (k[:, None, :] - k[None, :, :]) * h                     # (M, M, d)
    ref = torch.exp(-2j * math.pi * torch.einsum("ijd,pd->ijp", diff, x)).sum(-1)
    assert _rel(D.dense_T(s["v"]), ref) < 1e-13
    assert abs(complex(D.dense_T(s["v"])[0, 0]) - D.NPTS) < 1e-10


@pytest.mark.parametrize("ns,herm", SHAPES, ids=[f"{'x'.join(map(str, ns))}{'-herm' if h else ''}" for ns, h in SHAPES])
def test_dense_cg_equals_fft_cg_after_three_iterations(ns, herm):
    from oracle import efgp_oracle as O
    s = D.system(ns, herm)
    To = O.Toeplitz(s["v"])
    for variant, make in ((0, O.make_A_mean), (1, O.make_A_var)):
        A = D.system_A(ns, herm, variant)
        Af = make(s["ws"], To, s["sigmasq"])
        xd, itd = D.cg_dense(A, s["b"][0], s["x0"][0], 1e-30, max_iter=3, early=False, diag=s["diag"])
        xf, itf = O.cg_single(Af, s["b"][0], s["x0"][0], 1e-30, max_iter=3, early=False, diag=s["diag"])
        assert itd == itf == 3 and _rel(xd, xf) < 1e-13
        xd, itd = D.cg_dense(A, s["b"], s["x0"], 1e-30, max_iter=3, early=False)
        xf, itf = O.cg_batched(Af, s["b"], s["x0"], 1e-30, max_iter=3, early=False)
        assert itd == itf == 3 and _rel(xd, xf) < 1e-13


@pytest.mark.parametrize("ns,herm", SHAPES, ids=[f"{'x'.join(map(str, ns))}{'-herm' if h else ''}" for ns, h in SHAPES])
def test_stopping_index_is_decided_by_the_system(ns, herm):
    """The converged solves of tests/test_gpu_cg_routes.py compare iteration counts: the two references (equal in exact arithmetic)
    must agree on them, single system and rows of a batch, and their residual histories to 1e-3 -- else a count says nothing."""
    from oracle import efgp_oracle as O
    s = D.system(ns, herm)
    A = D.matvec(D.system_A(ns, herm, 0))
    Af = O.make_A_mean(s["ws"], O.Toeplitz(s["v"]), s["sigmasq"])
    zero = torch.zeros_like(s["b"])
    hd, hf = [], []
    _, itd = O.cg_single(A, s["b"][0], zero[0], 1e-8, diag=s["diag"], history=hd)
    _, itf = O.cg_single(Af, s["b"][0], zero[0], 1e-8, diag=s["diag"], history=hf)
    assert itd == itf and itd <= max(2, math.prod(ns))            # not past the exhaustion of the Krylov space
    assert max(abs(p - q) / q for p, q in zip(hd, hf)) < 1e-3
    for r in (0, 2):
        assert O.cg_batched(A, s["b"][r:r + 1], zero[r:r + 1], 1e-8, diag=s["diag"])[1] == \
               O.cg_batched(Af, s["b"][r:r + 1], zero[r:r + 1], 1e-8, diag=s["diag"])[1]


def test_direct_solve_and_row_counts():
    """The direct solve satisfies the system; the per-row counts are those of the batch (one for the zero row)."""
    ns = (8, 64)
    s = D.system(ns)
    A = D.system_A(ns, False, 0)
    xs = D.direct_solve(A, s["b"])
    assert _rel(D.matvec(A)(xs), s["b"]) < 1e-13
    rows = D.row_counts(D.matvec(A), s["b"], 1e-8, diag=s["diag"])
    xb, itb = D.cg_dense(A, s["b"], None, 1e-8, diag=s["diag"])
    assert rows[1] == 1 and itb == max(rows) + 1
    assert _rel(xb, xs) < D.cond(A) * 1.05e-8


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_take_their_routes(name):
    ns, herm, kernel = R.CASES[name]
    got, grid = R.route(ns, herm)
    assert got == kernel, (name, got, grid)
    assert name not in R.DENSE or math.prod(ns) <= D.DENSE_MAX


def test_geometry_of_the_cases():
    """The figures the case list quotes: grids, padded sizes against kMaxGrid, radix lists, the route boundaries."""
    assert R.radices_for(4) == [4] and R.radices_for(512) == [8, 8, 8] and R.radices_for(2048) == [8, 8, 8, 4]
    assert R.radices_for(4096) == [8, 8, 8, 8] and R.radices_for(16) == [4, 4] and R.radices_for(1) == []
    assert R.fft_shape((4, 256)) == (8, 512) and R.padded_cells((8, 512)) == 4104
    assert R.fft_shape((8, 16, 4)) == (16, 32, 8) and R.padded_cells((16, 32, 8)) == R.K_MAX_GRID
    assert R.fft_shape((5, 7, 12)) == (16, 16, 32) and R.padded_cells((16, 16, 32)) == 8448
    assert R.fft_shape((30, 50)) == (64, 128) and R.fft_shape((20, 30)) == (64, 64) and R.fft_shape((16, 17)) == (32, 64)
    assert R.fft_shape((17, 19, 33)) == R.fft_shape((17, 18, 33)) == (64, 64, 128)
    assert math.prod((2048,)) == R.K_SLOTS * R.K_THREADS and not R.persistent_cg_eligible((2049,), R.fft_shape((2049,)))
    # the boundaries, side by side
    assert [R.route((n, n), True)[0] for n in (23, 25, 31, 32)] == ["herm48", "herm64", "herm64", "2d64"]
    assert [R.route((n,))[0] for n in (2, 3, 255, 256)] == ["generic", "line1d", "line1d", "generic"]
    assert R.route((23, 23), True, env=("EFGP_NO_CG48",)) == ("herm64", (64, 64))
    assert R.route((9, 9), True) == ("herm48", (48, 48)) and R.route((9, 9), True, env=("EFGP_NO_CG64_EMBED",))[0] == "generic"
    assert R.route((1, 1)) == ("2d64", (64, 64)) and R.route((1, 1, 1))[0] == "multi_fft"
    # hooks: every fused path has one that leads to the multi-launch solver
    assert R.route((8, 64), env=("EFGP_NO_PERSISTENT_CG",))[0] == "multi_fft"
    assert R.route((33, 40), env=("EFGP_NO_CG_COOP",))[0] == "multi_lines2"
    assert R.route((17, 19, 33), True, env=("EFGP_NO_CG_LINES",))[0] == "multi_fft"
    assert R.cg_shape((33, 40)) == (96, 96) and R.cg_shape((33, 40), env=("EFGP_NO_CG_COOP",)) == (128, 128)
    assert R.cg_shape((16, 16)) == (64, 64) and R.cg_shape((23, 23), True) == (48, 48) and R.cg_shape((20, 30)) == (64, 64)
    # unit axes leave the generic kernel's geometry
    assert R.route((1, 37)) == ("generic", (128,)) and R.route((7, 1, 7)) == ("generic", (16, 16))
    # ... and the specialised kernels are picked by the caller's shape: what is left of these blocks would fit 2d64 and line1d
    assert R.route((1, 20, 20)) == ("generic", (64, 64)) and R.route((20, 20))[0] == "2d64"
    assert R.route((1, 1, 9)) == ("generic", (32,)) and R.route((9,))[0] == "line1d"
    print("\n" + R.geometry_table())
