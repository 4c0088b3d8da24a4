"""Tensor-level wrappers over the C ABI: torch tensors carry the device memory and the stream,
every computation happens in libefgp_hip.so."""
import ctypes as C
import math
import os

import torch

from .lib import EFGP_EUNSUPPORTED, check, lib

_CD = torch.complex128
_RD = torch.float64


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("the EFGP HIP path needs an AMD GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback in this package")


def compute_device(*tensors, device=None):
    """Device the kernels run on: an explicit cuda device, else the device of the first cuda tensor,
    else cuda:LOCAL_RANK (one process per GPU)."""
    require_gpu()
    if device is not None:
        dev = torch.device(device)
        if dev.type == "cuda":
            return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    idx = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    return torch.device("cuda", idx)


# The wrappers below run a dozen times per fit / gradient step, and the step had become HOST-bound (round 4: 300 us of kernels in a
# 430-us gradient step): `torch.cuda.current_stream(dev)` builds a Stream object (5.7 us) and `torch.cuda.device(dev)` resolves its
# argument through `_get_device_index` (2.7 us, twice per wrapper) -- ~25 such calls per step.  Both have direct C entry points.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_exchange = getattr(torch._C, "_cuda_exchangeDevice", None)
_maybe_exchange = getattr(torch._C, "_cuda_maybeExchangeDevice", None) or _exchange


def _stream(dev):
    if _raw_stream is not None and dev.index is not None:
        return C.c_void_p(_raw_stream(dev.index))
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _on:
    """`with _on(dev):` is `with torch.cuda.device(dev):` without the argument resolution and object churn."""
    __slots__ = ("idx", "prev", "ctx", "_dev")

    def __init__(self, dev):
        self._dev = dev
        self.idx = dev.index if (_exchange is not None and getattr(dev, "index", None) is not None) else -1
        self.prev = -1
        self.ctx = None

    def __enter__(self):
        if self.idx >= 0:
            self.prev = _exchange(self.idx)
        else:
            self.ctx = torch.cuda.device(self._dev)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.idx >= 0:
            _maybe_exchange(self.prev)
            return False
        return self.ctx.__exit__(*exc)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dc(t, dev, dtype):
    """`t.to(device=dev, dtype=dtype).contiguous()`, returning `t` itself when it already is all that: the no-op conversions cost
    ~2 us each and a step makes some thirty of them."""
    if t.dtype is dtype and t.device == dev and t.is_contiguous():
        return t
    return t.to(device=dev, dtype=dtype).contiguous()


NORMAL_ROW_STRIDE = 0xD1342543DE82EF95      # csrc/nufft_dev.hpp: pair p at index n is pair 0 at index n + p * stride (mod 2^64)


def _wrap_i64(v):
    """An index offset in wrapping 64-bit arithmetic as the signed value the C ABI takes."""
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def normal_row_offset(first_row, index_offset=0):
    """index_offset that makes row r of a generated-normal call the global row first_row + r (first_row even)."""
    if first_row % 2:
        raise ValueError("normal rows are generated in pairs: the first row of a block must be even")
    return _wrap_i64(int(index_offset) + (int(first_row) // 2) * NORMAL_ROW_STRIDE)


def _per_axis(v):
    """None for one number (Python or numpy scalar, 0-dim tensor), else the values of a sequence / array / tensor as a tuple."""
    if torch.is_tensor(v):
        return None if v.ndim == 0 else tuple(v.reshape(-1).tolist())
    if hasattr(v, "__len__"):
        return tuple(v.tolist()) if hasattr(v, "tolist") else tuple(v)
    return None


def _i64(vals):
    return (C.c_int64 * len(vals))(*[int(v) for v in vals])


class PointSet:
    """Per-model layout of the observation points (C ABI: efgp_points_*): bounding box and, for d = 2, copies
    sorted by a grid-independent key that the type-1 pass of every later plan streams (csrc/points_layout.hpp).
    `values` (the model's targets) may be attached so that plans read a sorted copy and max|y| is computed once."""

    def __init__(self, x, values=None):
        assert x.is_cuda and x.dtype == _RD and x.ndim == 2 and x.is_contiguous()
        self.x = x                    # keeps the storage alive; the library does not copy
        self.dev = x.device
        self.npts, self.dim = x.shape
        self.values = None
        self._h = C.c_void_p()
        with _on(self.dev):
            check(lib().efgp_points_create(C.byref(self._h), self.dev.index, self.dim, self.npts, _ptr(x), _stream(self.dev)),
                  "efgp_points_create")
        if values is not None:
            self.attach_values(values)

    def attach_values(self, y):
        assert y.is_cuda and y.dtype == _RD and y.is_contiguous() and y.numel() == self.npts
        self.values = y
        with _on(self.dev):
            check(lib().efgp_points_attach_values(self._h, _ptr(y), _stream(self.dev)), "efgp_points_attach_values")

    def bounds(self):
        lo = (C.c_double * 3)()
        hi = (C.c_double * 3)()
        check(lib().efgp_points_bounds(self._h, lo, hi), "efgp_points_bounds")
        return [float(lo[a]) for a in range(self.dim)], [float(hi[a]) for a in range(self.dim)]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().efgp_points_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NufftPlan:
    """Type-1 / type-2 transforms for a fixed point set (C ABI: efgp_nufft_*).  With `points` (a PointSet over the
    same x) the plan is made on the model's layout (efgp_nufft_create_on).  `h`: one grid spacing, or a sequence of d for a
    per-axis grid (efgp_nufft_create_nd / efgp_nufft_create_on_nd)."""

    def __init__(self, x, h, tol, xcen=None, points=None):
        assert x.is_cuda and x.dtype == _RD and x.ndim == 2 and x.is_contiguous()
        self.x = x                    # keeps the storage alive; the library does not copy
        self.points = points          # the layout must outlive the plan
        self.dev = x.device
        self.npts, self.dim = x.shape
        hv = _per_axis(h)
        per_axis = hv is not None
        self.h = tuple(float(v) for v in hv) if per_axis else float(h)
        if per_axis and len(self.h) != self.dim:
            raise ValueError(f"NufftPlan: {len(self.h)} spacings for {self.dim}-dimensional points")
        self.tol = float(tol)
        xc = None
        if xcen is not None:
            vals = [float(v) for v in xcen]
            if any(v != 0.0 for v in vals):
                xc = (C.c_double * self.dim)(*vals)
        self._h = C.c_void_p()
        if points is not None:
            assert points.x.data_ptr() == x.data_ptr() and points.npts == self.npts
        if per_axis:
            hs = (C.c_double * self.dim)(*self.h)
            if points is not None:
                check(lib().efgp_nufft_create_on_nd(C.byref(self._h), points._h, xc, hs, self.tol), "efgp_nufft_create_on_nd")
            else:
                check(lib().efgp_nufft_create_nd(C.byref(self._h), self.dev.index, self.dim, self.npts, _ptr(x), xc, hs, self.tol),
                      "efgp_nufft_create_nd")
        elif points is not None:
            check(lib().efgp_nufft_create_on(C.byref(self._h), points._h, xc, self.h, self.tol), "efgp_nufft_create_on")
        else:
            check(lib().efgp_nufft_create(C.byref(self._h), self.dev.index, self.dim, self.npts, _ptr(x), xc,
                                          self.h, self.tol), "efgp_nufft_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().efgp_nufft_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def type1(self, c, n_modes, modeord=0, isign=-1):
        """c (N,) or (B,N) real or complex -> (B?, *n_modes) complex128."""
        batched = c.ndim > 1
        cc = c.reshape(-1, self.npts)
        is_c = cc.is_complex()
        cc = cc.to(device=self.dev, dtype=_CD if is_c else _RD).contiguous()
        B = cc.shape[0]
        out = torch.empty((B,) + tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        with _on(self.dev):
            check(lib().efgp_nufft_type1(self._h, _ptr(cc), int(is_c), B, _i64(n_modes), isign, int(modeord),
                                         _ptr(out), _stream(self.dev)), "efgp_nufft_type1")
        return out if batched else out[0]

    def type1_rademacher(self, seed, nbatch, n_modes, index_offset=0, modeord=0):
        """F* Z for Z[b,n] = +-1 generated in the kernel from (seed, b, n + index_offset) -> (B, *n_modes)."""
        out = torch.empty((int(nbatch),) + tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        with _on(self.dev):
            check(lib().efgp_nufft_type1_rademacher(self._h, int(seed) & (2 ** 64 - 1), int(index_offset), int(nbatch),
                                                    _i64(n_modes), int(modeord), _ptr(out), _stream(self.dev)),
                  "efgp_nufft_type1_rademacher")
        return out

    def type1_normal(self, seed, nbatch, n_modes, index_offset=0, modeord=0):
        """F* Z for Z[b,n] ~ N(0, 1) generated in the kernel from (seed, b, n + index_offset) -> (B, *n_modes); `normal_fill`
        materialises the same Z."""
        out = torch.empty((int(nbatch),) + tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        with _on(self.dev):
            check(lib().efgp_nufft_type1_normal(self._h, int(seed) & (2 ** 64 - 1), _wrap_i64(index_offset), int(nbatch),
                                                _i64(n_modes), int(modeord), _ptr(out), _stream(self.dev)),
                  "efgp_nufft_type1_normal")
        return out

    def type1_normal_scaled(self, seed, nbatch, n_modes, scale, index_offset=0, modeord=0):
        """F* (scale .* Z[b]) for the normals of `type1_normal` and a per-point factor `scale` ((N,) float64, finite, >= 0, in the
        order of x) -> (B, *n_modes); the scaled rows are never materialised (efgp_nufft_type1_normal_scaled)."""
        sc = _dc(scale, self.dev, _RD).reshape(-1)
        if sc.numel() != self.npts:
            raise ValueError(f"type1_normal_scaled: scale has {sc.numel()} entries, the plan has {self.npts} points")
        out = torch.empty((int(nbatch),) + tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        with _on(self.dev):
            check(lib().efgp_nufft_type1_normal_scaled(self._h, int(seed) & (2 ** 64 - 1), _wrap_i64(index_offset), int(nbatch),
                                                       _ptr(sc), _i64(n_modes), int(modeord), _ptr(out), _stream(self.dev)),
                  "efgp_nufft_type1_normal_scaled")
        return out

    def type1_pair(self, y, n_modes_y, n_modes_one):
        """One pass over the points: (F* y on n_modes_y, F* 1 on n_modes_one)."""
        yy = _dc(y, self.dev, _RD)
        shape_y, shape_o = tuple(int(m) for m in n_modes_y), tuple(int(m) for m in n_modes_one)
        My = 1
        for m in shape_y:
            My *= m
        Mo = 1
        for m in shape_o:
            Mo *= m
        # one buffer, two views: the sharded fit all-reduces both results in place with a single collective
        flat = torch.empty(My + Mo, dtype=_CD, device=self.dev)
        out_y, out_o = flat[:My].view(shape_y), flat[My:].view(shape_o)
        with _on(self.dev):
            check(lib().efgp_nufft_type1_pair(self._h, _ptr(yy), _i64(n_modes_y), _ptr(out_y), _i64(n_modes_one),
                                              _ptr(out_o), _stream(self.dev)), "efgp_nufft_type1_pair")
        return out_y, out_o

    def type1_ones(self, n_modes):
        out_o = torch.empty(tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        with _on(self.dev):
            check(lib().efgp_nufft_type1_pair(self._h, None, None, None, _i64(n_modes), _ptr(out_o),
                                              _stream(self.dev)), "efgp_nufft_type1_pair")
        return out_o

    def type2(self, f, n_modes, modeord=0, real_only=False, isign=+1, batched=None, mode_scale=None):
        """f (prod,) | (*n_modes) | (B, ...) complex -> (N,) | (B,N) complex128 (float64 if real_only).
        mode_scale (prod,) complex: the modes are multiplied by it inside the transform (F (ws * beta))."""
        M = 1
        for m in n_modes:
            M *= int(m)
        if batched is None:
            batched = not (f.ndim == 1 or tuple(f.shape) == tuple(int(m) for m in n_modes))
        ff = _dc(f.reshape(-1, M), self.dev, _CD)
        B = ff.shape[0]
        out = torch.empty((B, self.npts), dtype=_RD if real_only else _CD, device=self.dev)
        with _on(self.dev):
            if mode_scale is None:
                check(lib().efgp_nufft_type2(self._h, _ptr(ff), B, _i64(n_modes), isign, int(modeord), _ptr(out),
                                             int(bool(real_only)), _stream(self.dev)), "efgp_nufft_type2")
            else:
                sc = _dc(mode_scale.reshape(-1), self.dev, _CD)
                if sc.numel() != M:
                    raise ValueError(f"mode_scale has {sc.numel()} entries, the mode box has {M}")
                check(lib().efgp_nufft_type2_scaled(self._h, _ptr(ff), _ptr(sc), B, _i64(n_modes), isign, int(modeord),
                                                    _ptr(out), int(bool(real_only)), _stream(self.dev)),
                      "efgp_nufft_type2_scaled")
        return out if batched else out[0]

    def type2_jet(self, f, n_modes, *, mode_scale=None):
        """Value and gradient of Re F (mode_scale * f) at the plan's points: f (M,) | (nrows, M) complex -> (nrows, 1 + d, N)
        float64, entry [b, 0] the value and [b, 1 + a] the partial along axis a.  `mode_jet_rows` makes the 1 + d coefficient rows of
        every row of f; they go through the batched real-only `type2`, which pairs them two per complex fine grid, in blocks of at
        most `_SAMPLE_BLOCK[d]` rows (the fine-grid memory of one call)."""
        shape = tuple(int(m) for m in n_modes)
        jets = mode_jet_rows(f, shape, self.h, mode_scale=mode_scale)
        R, J, M = jets.shape
        rows = jets.view(R * J, M)
        block = _SAMPLE_BLOCK[self.dim]
        if R * J <= block:
            return self.type2(rows, shape, real_only=True, batched=True).view(R, J, self.npts)
        out = torch.empty((R * J, self.npts), dtype=_RD, device=self.dev)
        for lo in range(0, R * J, block):
            out[lo:lo + block] = self.type2(rows[lo:lo + block], shape, real_only=True, batched=True)
        return out.view(R, J, self.npts)


# Rows per batched type-2 call of the function draws, the multi-output means and the jets: a call holds one complex fine grid per
# TWO real-only rows (efgpnd.py states the memory reasoning where it uses the blocks)
_SAMPLE_BLOCK = {1: 64, 2: 64, 3: 8}


class ToeplitzOp:
    """d-dimensional Toeplitz mat-vec (C ABI: efgp_toeplitz_*)."""

    def __init__(self, v, force_pow2=True, defer_spectra=False):
        """defer_spectra: on the 48 x 48 Hermitian grids (2-D blocks of up to 23 x 23 modes) launch nothing now -- the fused mean
        solve (cg_solve_mean_fused) makes the spectrum it needs, any other use the rest (efgp_toeplitz_create_ex).  The library
        then reads `self.v` later: it must not be changed in place while the operator lives."""
        assert v.is_cuda
        self.dev = v.device
        self.v = v.to(_CD).contiguous()
        self.d = self.v.ndim
        self.Ls = list(self.v.shape)
        self.ns = [(L + 1) // 2 for L in self.Ls]
        self.size = 1
        for n in self.ns:
            self.size *= n
        self._h = C.c_void_p()
        with _on(self.dev):
            check(lib().efgp_toeplitz_create_ex(C.byref(self._h), self.dev.index, self.d, _i64(self.Ls), _ptr(self.v),
                                                int(bool(force_pow2)), 1 if defer_spectra else 0, _stream(self.dev)),
                  "efgp_toeplitz_create")
        shp = (C.c_int64 * 3)()
        check(lib().efgp_toeplitz_fft_shape(self._h, shp), "efgp_toeplitz_fft_shape")
        self.fft_shape = [int(shp[a]) for a in range(self.d)]
        self.fft_cells = math.prod(self.fft_shape)
        # up to 4096 cells (64 x 64, 16^3, short lines) one workgroup solves a CG system; 2-D grids beyond run cooperative launches
        self.one_workgroup_per_system = self.fft_cells <= 4096
        self.may_hold_dead_rows = self.d == 2 and not self.one_workgroup_per_system

    def cg_shape(self, hermitian=False):
        """Circulant grid the fused CG solves of this operator run on (efgp_toeplitz_cg_shape): the smallest one the solvers'
        transforms cover that holds 2 n - 1 per axis; `fft_shape` stays the reference's grid."""
        shp = (C.c_int64 * 3)()
        check(lib().efgp_toeplitz_cg_shape(self._h, int(bool(hermitian)), shp), "efgp_toeplitz_cg_shape")
        return [int(shp[a]) for a in range(self.d)]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().efgp_toeplitz_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, u):
        """u (..., size) complex on the device -> same shape."""
        uu = _dc(u.reshape(-1, self.size), self.dev, _CD)
        out = torch.empty_like(uu)
        with _on(self.dev):
            check(lib().efgp_toeplitz_apply(self._h, _ptr(uu), uu.shape[0], _ptr(out), _stream(self.dev)),
                  "efgp_toeplitz_apply")
        return out.reshape(u.shape)

    def apply_scaled(self, u, pre=None, post=None, out=None):
        """post .* T(pre .* u) for u (..., size) complex or real float64 on the device (efgp_toeplitz_apply_scaled); pre / post:
        (size,) complex128 device tensors or None.  `out`: a contiguous complex128 (rows, size) device tensor to write into."""
        real = not u.is_complex()
        uu = u.reshape(-1, self.size).to(device=self.dev, dtype=_RD if real else _CD).contiguous()
        res = out if out is not None else torch.empty(uu.shape, dtype=_CD, device=self.dev)
        assert res.is_contiguous() and res.dtype == _CD and res.numel() == uu.numel()
        for dgl in (pre, post):
            assert dgl is None or (dgl.is_cuda and dgl.dtype == _CD and dgl.is_contiguous() and dgl.numel() == self.size)
        with _on(self.dev):
            check(lib().efgp_toeplitz_apply_scaled(self._h, _ptr(uu), int(real), uu.shape[0], _ptr(pre) if pre is not None else None,
                                                   _ptr(post) if post is not None else None, _ptr(res), _stream(self.dev)),
                  "efgp_toeplitz_apply_scaled")
        return res if out is not None else res.reshape(u.shape)


def gradient_prepare(ws, fy, v_center, sigmasq, want_diag=True, want_rhs=True):
    """(diag, rhs) = (Re v_center |ws|^2 + sigmasq, ws .* fy) in one launch (efgp_gradient_prepare); v_center: a one-element
    complex128 device view of the Toeplitz vector's centre."""
    dev = ws.device
    M = ws.numel()
    assert ws.dtype == _CD and ws.is_contiguous()
    diag = torch.empty(M, dtype=_RD, device=dev) if want_diag else None
    rhs = torch.empty(M, dtype=_CD, device=dev) if want_rhs else None
    ff = fy.reshape(-1).to(dtype=_CD).contiguous() if want_rhs else None
    if want_diag:
        assert v_center.is_cuda and v_center.dtype == _CD and v_center.numel() == 1
    with _on(dev):
        check(lib().efgp_gradient_prepare(dev.index, M, _ptr(ws), _ptr(ff) if ff is not None else None,
                                          _ptr(v_center) if want_diag else None, float(sigmasq), _ptr(diag) if want_diag else None,
                                          _ptr(rhs) if want_rhs else None, _stream(dev)), "efgp_gradient_prepare")
    return diag, rhs


def gradient_assemble(fy, tg, ws, beta, dprime, fz, v, beta_all, *, variance_idx, trace_idx, sigmasq, n_obs, yy, variance):
    """grad | term1 | term2 | y.alpha as ONE device vector of 3 (H + 1) + 1 doubles (efgp_gradient_assemble)."""
    dev = ws.device
    M = ws.numel()
    H = dprime.shape[1] if dprime is not None and dprime.ndim == 2 else 0
    T = v.shape[0]
    K = len(trace_idx)
    for t_ in (fy, tg, ws, beta, beta_all) + ((dprime,) if H else ()) + ((fz,) if K else ()):
        assert t_.is_cuda and t_.dtype == _CD and t_.is_contiguous()
    assert v.dtype == _RD and v.is_contiguous() and v.shape == (T, M)
    assert beta_all.numel() == (K + 1) * T * M and (K == 0 or fz.numel() == T * M)
    out = torch.empty(3 * (H + 1) + 1, dtype=_RD, device=dev)
    tix = (C.c_int * max(1, K))(*[int(i) for i in trace_idx])
    with _on(dev):
        check(lib().efgp_gradient_assemble(dev.index, M, T, H, -1 if variance_idx is None else int(variance_idx), K, tix,
                                           _ptr(fy), _ptr(tg), _ptr(ws), _ptr(beta), _ptr(dprime) if H else None,
                                           _ptr(fz) if K else None, _ptr(v), _ptr(beta_all), float(sigmasq), float(n_obs), float(yy),
                                           float(variance), _ptr(out), _stream(dev)), "efgp_gradient_assemble")
    return out


def gradient_assemble_multi(fy, tg, ws, beta, dprime, fz, v, beta_all, *, variance_idx, trace_idx, sigmasq, n_obs, yy, row_scale, variance):
    """`gradient_assemble` for the joint objective of R outputs at shared points (efgp_gradient_assemble_multi): fy, tg, beta (R, M),
    one row per output in units of row_scale[r] (exact powers of two); yy, row_scale (R,) float64 DEVICE tensors, yy[r] the sum of
    squares of output r in the same units.  Returns (out, rows_out): out the 3 (H + 1) + 1 doubles grad | term1 | term2 | y.alpha of
    the sum over outputs, rows_out (R, 4) = y.z, |z|^2, y.alpha, |alpha|^2 per output, scaled back.  v = None (then fz, beta_all
    are not looked at): no probes -- the data terms alone; the estimated entries of term1 (and of grad) are NaN."""
    dev = ws.device
    M = ws.numel()
    H = dprime.shape[1] if dprime is not None and dprime.ndim == 2 else 0
    T = v.shape[0] if v is not None else 0
    K = len(trace_idx) if T else 0
    if T == 0:
        trace_idx = []
        v = torch.empty((0, M), dtype=_RD, device=dev)
        fz = beta_all = torch.empty((0, M), dtype=_CD, device=dev)
    if fy.ndim != 2 or fy.shape[1] != M or tuple(tg.shape) != tuple(fy.shape) or tuple(beta.shape) != tuple(fy.shape):
        raise ValueError(f"gradient_assemble_multi: fy, tg and beta must be (rows, {M}) (got {tuple(fy.shape)}, {tuple(tg.shape)}, "
                         f"{tuple(beta.shape)})")
    R = fy.shape[0]
    for t_ in (fy, tg, ws, beta, beta_all) + ((dprime,) if H else ()) + ((fz,) if K else ()):
        assert t_.is_cuda and t_.dtype == _CD and t_.is_contiguous()
    assert v.dtype == _RD and v.is_contiguous() and v.shape == (T, M)
    assert beta_all.numel() == (K + 1) * T * M and (K == 0 or fz.numel() == T * M)
    for t_ in (yy, row_scale):
        if not (torch.is_tensor(t_) and t_.is_cuda and t_.dtype == _RD and t_.is_contiguous() and t_.numel() == R):
            raise ValueError(f"gradient_assemble_multi: yy and row_scale must be contiguous float64 GPU tensors of {R} entries")
    out = torch.empty(3 * (H + 1) + 1, dtype=_RD, device=dev)
    rows_out = torch.empty((R, 4), dtype=_RD, device=dev)
    tix = (C.c_int * max(1, K))(*[int(i) for i in trace_idx])
    with _on(dev):
        check(lib().efgp_gradient_assemble_multi(dev.index, M, R, T, H, -1 if variance_idx is None else int(variance_idx), K, tix,
                                                 _ptr(fy), _ptr(tg), _ptr(ws), _ptr(beta), _ptr(dprime) if H else None,
                                                 _ptr(fz) if K else None, _ptr(v) if T else None, _ptr(beta_all) if T else None,
                                                 float(sigmasq), float(n_obs), _ptr(yy), _ptr(row_scale), float(variance), _ptr(out), _ptr(rows_out), _stream(dev)),
              "efgp_gradient_assemble_multi")
    return out, rows_out


def _start_vector(x0, bb, op, dev):
    """The solver's in/out buffer: a copy of x0, or zeros when x0 is None (one fill instead of a fill and a copy)."""
    if x0 is None:
        return torch.zeros(bb.shape, dtype=_CD, device=dev)
    return _dc(x0.reshape(-1, op.size), dev, _CD).clone()


def cg_solve(op, ws, sigmasq, variant, b, x0, tol, max_iter=None, early_stop=True, diag=None, batched=None, hermitian=False):
    """Fused device CG on ws*T(ws*.) (+sigma^2 | /sigma^2 + 1).  Returns (x, iters, row_iters).
    hermitian=True: see cg_solve_async, whose kernels run where the grid allows (settled); elsewhere the general solver."""
    if not hermitian:
        return _cg_solve_sync(op, ws, sigmasq, variant, b, x0, tol, max_iter, early_stop, diag, batched, False)
    x, its = cg_solve_lazy(op, ws, sigmasq, variant, b, x0, tol, max_iter=max_iter, early_stop=early_stop, diag=diag,
                           batched=batched, hermitian=True)
    its.settle()
    return x, int(its), list(its.rows)


def _cg_solve_sync(op, ws, sigmasq, variant, b, x0, tol, max_iter, early_stop, diag, batched, hermitian):
    """efgp_cg_solve[_hermitian]: returns when every system is solved (those of a dead grid barrier re-solved inside)."""
    dev = op.dev
    if batched is None:
        batched = b.ndim > 1
    bb = _dc(b.reshape(-1, op.size), dev, _CD)
    x = _start_vector(x0, bb, op, dev)
    wsd = _dc(ws, dev, _CD)
    dg = _dc(diag, dev, _RD) if diag is not None else None
    B = bb.shape[0]
    iters = C.c_int(0)
    rows = (C.c_int * B)()
    with _on(dev):
        # hermitian: the synchronous entry keeps the promise too (3-D grids carry the planes k0 >= 0 only)
        fn = lib().efgp_cg_solve_hermitian if hermitian else lib().efgp_cg_solve
        check(fn(op._h, _ptr(wsd), float(sigmasq), int(variant), _ptr(dg) if dg is not None else None,
                 _ptr(bb), _ptr(x), B, float(tol), int(max_iter) if max_iter is not None else 0,
                 int(bool(early_stop)), int(bool(batched)), C.byref(iters), rows, _stream(dev)),
              "efgp_cg_solve")
    return x.reshape(b.shape), int(iters.value), [int(r) for r in rows]


_REFUSED = ("efgp_hip: a system given to the Hermitian CG kernel is not the transform of real data "
            "(right-hand side not conjugate-even, or ws not real and even); its solution is NaN")


class LazyIterations:
    """Iteration counts of an asynchronous CG solve; reading them waits for the solve (device tensor -> host).  `x` and `redo`
    (row indices -> the synchronous entry's result for them) come with a solve that may hold dead rows (-3, NaN): settle()."""

    def __init__(self, rows_dev, batched, max_iter, x=None, redo=None):
        self.rows_tensor = rows_dev         # per-system counts (int32) as the solve writes them: readable without waiting
        self._batched = batched
        self._max_iter = max_iter
        self._rows = None
        self._x, self._redo = x, redo

    @property
    def needs_settle(self):
        return self._redo is not None

    def settle(self):
        """One read of the counts of a solve that may hold dead rows (a no-op otherwise): -2 raises, -3 rows are solved again by
        `redo` and written into x and the counts in place.  Returns whether a row was solved again."""
        if not self.needs_settle:
            return False
        rows = [int(v) for v in self.rows_tensor.tolist()]
        if -2 in rows:
            raise RuntimeError(_REFUSED)
        dead = [i for i, v in enumerate(rows) if v == -3]
        if dead:
            xd, _, rd = self._redo(dead)
            self._x.view(len(rows), -1)[dead] = xd.reshape(len(dead), -1)
            for i, v in zip(dead, rd):
                rows[i] = int(v)
            self.rows_tensor = self.rows_tensor.new_tensor(rows)
        self._rows = rows
        self._x = self._redo = None         # the operands of a re-solve need not outlive the settled solve
        return bool(dead)

    @property
    def rows(self):
        if self._rows is None:
            self._rows = [int(v) for v in self.rows_tensor.tolist()]
            if any(v == -3 for v in self._rows):
                raise RuntimeError("efgp_hip: a cooperative CG launch could not get its workgroups resident together; the affected "
                                   "systems hold NaN -- settle() re-solves them; EFGP_NO_CG_COOP=1 avoids the cooperative path")
            if any(v == -2 for v in self._rows):
                raise RuntimeError(_REFUSED)
        return self._rows

    def __int__(self):
        mx = max(self.rows)
        # cg.py:193-199,243: the batched loop counts the terminating pass too
        return mx + 1 if (self._batched and mx < self._max_iter) else mx

    __index__ = __int__

    def __repr__(self):
        return str(int(self))

    # number-like: callers of the reference's API compare, add and format iteration counts
    def __eq__(self, other):
        return int(self) == other

    def __lt__(self, other):
        return int(self) < other

    def __le__(self, other):
        return int(self) <= other

    def __gt__(self, other):
        return int(self) > other

    def __ge__(self, other):
        return int(self) >= other

    def __hash__(self):
        return hash(int(self))

    def __add__(self, other):
        return int(self) + other

    __radd__ = __add__

    def __format__(self, spec):
        return format(int(self), spec)


def cg_solve_async(op, ws, sigmasq, variant, b, x0, tol, max_iter=None, early_stop=True, diag=None, batched=None,
                   hermitian=False):
    """Like cg_solve but without host synchronisation: returns (x, LazyIterations) or None when the operator's
    grid does not fit the persistent kernel (cg_solve_lazy then takes the synchronous entry).  hermitian=True: b, x0 are Fourier
    coefficients of real functions and ws is real and even (efgp_cg_solve_hermitian_async; refused with an error when
    the data say otherwise)."""
    dev = op.dev
    if batched is None:
        batched = b.ndim > 1
    bb = _dc(b.reshape(-1, op.size), dev, _CD)
    wsd = _dc(ws, dev, _CD)
    dg = _dc(diag, dev, _RD) if diag is not None else None
    B = bb.shape[0]
    mi = int(max_iter) if max_iter is not None else 2 * op.size
    rows_dev = torch.empty(B, dtype=torch.int32, device=dev)
    if x0 is None:
        # from zero: the kernels start from x = 0 themselves (no fill launch, no initial operator application)
        x = torch.empty(bb.shape, dtype=_CD, device=dev)
        with _on(dev):
            rc = lib().efgp_cg_solve_from_zero_async(op._h, _ptr(wsd), float(sigmasq), int(variant), _ptr(dg) if dg is not None else None,
                                                     _ptr(bb), _ptr(x), B, float(tol), mi, int(bool(early_stop)), int(bool(batched)),
                                                     int(bool(hermitian)), _ptr(rows_dev), _stream(dev))
    else:
        x = _start_vector(x0, bb, op, dev)
        with _on(dev):
            fn = lib().efgp_cg_solve_hermitian_async if hermitian else lib().efgp_cg_solve_async
            rc = fn(op._h, _ptr(wsd), float(sigmasq), int(variant), _ptr(dg) if dg is not None else None, _ptr(bb), _ptr(x), B,
                    float(tol), mi, int(bool(early_stop)), int(bool(batched)), _ptr(rows_dev), _stream(dev))
    if rc == EFGP_EUNSUPPORTED:
        return None
    check(rc, "efgp_cg_solve_async")
    redo = None
    if op.may_hold_dead_rows:           # settle(): the rows a dead grid barrier left, from the caller's start vector
        def redo(ix):
            return _cg_solve_sync(op, wsd, sigmasq, variant, bb[ix], x0.reshape(-1, op.size)[ix] if x0 is not None else None,
                                  tol, mi, early_stop, dg, batched, hermitian)
    # keep the operands alive until the stream has consumed them: torch's caching allocator only reuses a block
    # for work enqueued later on the same stream, so dropping the Python references here is safe
    return x.reshape(b.shape), LazyIterations(rows_dev, bool(batched), mi, x, redo)


def cg_solve_lazy(op, ws, sigmasq, variant, b, x0, tol, max_iter=None, early_stop=True, diag=None, batched=None,
                  hermitian=False):
    """cg_solve_async where the grid fits its kernels, the synchronous entry otherwise: (x, LazyIterations) on every grid.
    Settle the counts before x is used without reading them (a no-op unless the solve may hold dead rows)."""
    res = cg_solve_async(op, ws, sigmasq, variant, b, x0, tol, max_iter=max_iter, early_stop=early_stop, diag=diag,
                         batched=batched, hermitian=hermitian)
    if res is not None:
        return res
    batched = b.ndim > 1 if batched is None else bool(batched)
    x, _, rows = _cg_solve_sync(op, ws, sigmasq, variant, b, x0, tol, max_iter, early_stop, diag, batched, hermitian)
    return x, LazyIterations(torch.tensor(rows, dtype=torch.int32), batched, int(max_iter) if max_iter is not None else 2 * op.size)


def cg_solve_mean_fused(op, kind, nu, c0, lengthscale, h, mtot, sigmasq, diag_scale, fy, tol, max_iter=None, early_stop=True):
    """cg_solve_mean_async with its set-up in the same launch (efgp_cg_solve_mean_fused), for an operator made with
    defer_spectra=True on a 48 x 48 Hermitian grid: ws of the built-in kernel (kind 0 SE, 1 Matern nu; c0 as
    utils.kernels.kernel_constants forms it) is evaluated in the kernel, and so is the operator's 48 x 48 spectrum.
    Returns (beta, ws (M,) complex128, LazyIterations), or None (nothing enqueued) for any other operator."""
    dev = op.dev
    ff = _dc(fy.reshape(-1), dev, _CD)
    if ff.numel() != op.size or op.size != int(mtot) ** op.d:
        raise ValueError(f"fy has {ff.numel()} entries, the operator has {op.size} (mtot {mtot})")
    ws = torch.empty(op.size, dtype=_CD, device=dev)
    x = torch.empty(op.size, dtype=_CD, device=dev)
    ds = None
    if diag_scale is not None:
        ds = diag_scale.to(device=dev, dtype=_RD)        # no copy for a float64 view on the device
        if ds.numel() != 1:
            raise ValueError("diag_scale must hold one value")
    mi = int(max_iter) if max_iter is not None else 2 * op.size
    rows_dev = torch.empty(1, dtype=torch.int32, device=dev)
    with _on(dev):
        rc = lib().efgp_cg_solve_mean_fused(op._h, int(kind), float(nu), float(lengthscale), float(c0), float(h), int(mtot), _ptr(ws),
                                            float(sigmasq), _ptr(ds) if ds is not None else None, _ptr(ff), _ptr(x), float(tol), mi,
                                            int(bool(early_stop)), _ptr(rows_dev), _stream(dev))
    if rc == EFGP_EUNSUPPORTED:
        return None
    check(rc, "efgp_cg_solve_mean_fused")
    return x.reshape(fy.shape), ws, LazyIterations(rows_dev, False, mi, x, None)


def cg_solve_mean_async(op, ws, sigmasq, diag_scale, fy, tol, max_iter=None, early_stop=True):
    """The fit's mean system (D T D + sigmasq I) beta = D fy from beta_0 = 0 in ONE launch and without host
    synchronisation: the right-hand side ws*fy, the Jacobi diagonal diag_scale*|ws|^2 + sigmasq and the zero start
    are formed inside the kernel.  diag_scale: 0-dim float64 device tensor (may be a view, e.g. v[centre].real) or
    None for no preconditioner.  Returns (beta, LazyIterations) or None when the grid does not fit the kernel."""
    dev = op.dev
    ff = _dc(fy.reshape(-1), dev, _CD)
    if ff.numel() != op.size:
        raise ValueError(f"fy has {ff.numel()} entries, the operator has {op.size}")
    wsd = _dc(ws.reshape(-1), dev, _CD)
    x = torch.empty(op.size, dtype=_CD, device=dev)
    ds = None
    if diag_scale is not None:
        ds = diag_scale.to(device=dev, dtype=_RD)        # no copy for a float64 view on the device
        if ds.numel() != 1:
            raise ValueError("diag_scale must hold one value")
    mi = int(max_iter) if max_iter is not None else 2 * op.size
    rows_dev = torch.empty(1, dtype=torch.int32, device=dev)
    with _on(dev):
        rc = lib().efgp_cg_solve_mean_async(op._h, _ptr(wsd), float(sigmasq), _ptr(ds) if ds is not None else None, _ptr(ff),
                                            _ptr(x), float(tol), mi, int(bool(early_stop)), _ptr(rows_dev), _stream(dev))
    if rc == EFGP_EUNSUPPORTED:
        return None
    check(rc, "efgp_cg_solve_mean_async")
    redo = None
    if op.may_hold_dead_rows:           # settle(): rhs and Jacobi diagonal as the kernel forms them, the synchronous entry from zero
        def redo(_):
            vc = ds.reshape(1).to(_CD) if ds is not None else None
            diag, rhs = gradient_prepare(wsd, ff, vc, sigmasq, want_diag=vc is not None)
            return _cg_solve_sync(op, wsd, sigmasq, 0, rhs, None, tol, mi, early_stop, diag, False, True)
    return x.reshape(fy.shape), LazyIterations(rows_dev, False, mi, x, redo)


def lanczos(op, ws, sigmasq, variant, z, steps):
    """`steps` Lanczos steps on A (variant 0: ws*T(ws*.) + sigmasq, 1: /sigmasq + 1) from every row of z (P, M), all inside
    one launch (efgp_lanczos).  Returns (alpha (P,steps), beta (P,steps), |z|^2 (P,), steps_taken (P,) int32) as DEVICE
    tensors -- nothing is read back -- or None when the grid does not fit the persistent kernel."""
    dev = op.dev
    zz = _dc(z.reshape(-1, op.size), dev, _CD)
    P = zz.shape[0]
    wsd = _dc(ws, dev, _CD)
    alpha = torch.zeros((P, int(steps)), dtype=_RD, device=dev)
    beta = torch.zeros((P, int(steps)), dtype=_RD, device=dev)
    norm2 = torch.empty(P, dtype=_RD, device=dev)
    taken = torch.empty(P, dtype=torch.int32, device=dev)
    with _on(dev):
        rc = lib().efgp_lanczos(op._h, _ptr(wsd), float(sigmasq), int(variant), _ptr(zz), P, int(steps), _ptr(alpha), _ptr(beta),
                                _ptr(norm2), _ptr(taken), _stream(dev))
    if rc == EFGP_EUNSUPPORTED:
        return None
    check(rc, "efgp_lanczos")
    return alpha, beta, norm2, taken


def _f64(vals):
    return (C.c_double * len(vals))(*[float(v) for v in vals])


def lag_sums(gamma, eta, mtot, dim):
    """c[r] = mean_j sum_{k-l=r} gamma[j,k] eta[j,l] on the (2 mtot - 1)^d lag box in FFT order (efgp_lag_sums); `mtot` a sequence
    of d mode counts: the box (2 mtot[a] - 1) per axis (efgp_lag_sums_nd)."""
    dev = gamma.device
    if _per_axis(mtot) is not None:
        shape = tuple(int(n) for n in _per_axis(mtot))
        if len(shape) != int(dim):
            raise ValueError(f"lag_sums: {len(shape)} mode counts for dimension {dim}")
        M = math.prod(shape)
        gg = gamma.reshape(-1, M).to(_CD).contiguous()
        ee = _dc(eta.reshape(-1, M), dev, _RD)
        out = torch.empty(tuple(2 * n - 1 for n in shape), dtype=_CD, device=dev)
        with _on(dev):
            check(lib().efgp_lag_sums_nd(dev.index, int(dim), _i64(shape), _ptr(gg), _ptr(ee), gg.shape[0], _ptr(out), _stream(dev)),
                  "efgp_lag_sums_nd")
        return out
    M = int(mtot) ** int(dim)
    gg = gamma.reshape(-1, M).to(_CD).contiguous()
    ee = _dc(eta.reshape(-1, M), dev, _RD)
    out = torch.empty((2 * int(mtot) - 1,) * int(dim), dtype=_CD, device=dev)
    with _on(dev):
        check(lib().efgp_lag_sums(dev.index, int(dim), int(mtot), _ptr(gg), _ptr(ee), gg.shape[0], _ptr(out), _stream(dev)),
              "efgp_lag_sums")
    return out


def variance_rhs(x_new, h, mtot, ws):
    """rhs[b, k] = ws[k] conj(f_k(x*_b)) for the 'regular' variance solves (efgp_variance_rhs); `h` and `mtot` sequences of d:
    the per-axis grid (efgp_variance_rhs_nd)."""
    dev = ws.device
    xn = _dc(x_new, dev, _RD)
    B, d = xn.shape
    wsd = ws.to(_CD).contiguous()
    out = torch.empty((B, wsd.numel()), dtype=_CD, device=dev)
    with _on(dev):
        if _per_axis(mtot) is None:
            check(lib().efgp_variance_rhs(dev.index, d, int(mtot), float(h), _ptr(xn), B, _ptr(wsd), _ptr(out), _stream(dev)),
                  "efgp_variance_rhs")
        else:
            mtot, h = _per_axis(mtot), _per_axis(h) or ()
            if len(mtot) != d or len(h) != d or math.prod(int(n) for n in mtot) != wsd.numel():
                raise ValueError("variance_rhs: per-axis h and mode counts must match the points and ws")
            check(lib().efgp_variance_rhs_nd(dev.index, d, _i64(mtot), _f64(h), _ptr(xn), B, _ptr(wsd), _ptr(out), _stream(dev)),
                  "efgp_variance_rhs_nd")
    return out


def variance_contract(x_new, h, mtot, ws, gamma):
    """s^2[b] = max(0, Re sum_k f_k(x*_b) ws[k] gamma[b, k]) (efgp_variance_contract; per-axis `h`, `mtot`:
    efgp_variance_contract_nd)."""
    dev = ws.device
    xn = _dc(x_new, dev, _RD)
    B, d = xn.shape
    wsd = ws.to(_CD).contiguous()
    gg = gamma.reshape(B, -1).to(_CD).contiguous()
    out = torch.empty(B, dtype=_RD, device=dev)
    with _on(dev):
        if _per_axis(mtot) is None:
            check(lib().efgp_variance_contract(dev.index, d, int(mtot), float(h), _ptr(xn), B, _ptr(wsd), _ptr(gg), _ptr(out),
                                               _stream(dev)), "efgp_variance_contract")
        else:
            mtot, h = _per_axis(mtot), _per_axis(h) or ()
            if len(mtot) != d or len(h) != d or math.prod(int(n) for n in mtot) != wsd.numel() or gg.shape[1] != wsd.numel():
                raise ValueError("variance_contract: per-axis h and mode counts must match the points, ws and gamma")
            check(lib().efgp_variance_contract_nd(dev.index, d, _i64(mtot), _f64(h), _ptr(xn), B, _ptr(wsd), _ptr(gg), _ptr(out),
                                                  _stream(dev)), "efgp_variance_contract_nd")
    return out


def _raster_args(what, axes, h, n_modes):
    """The checked per-axis arguments of the raster entries: (list of 1-D axes, spacings, mode counts)."""
    if torch.is_tensor(axes) or not hasattr(axes, "__len__"):
        axes = [axes]
    axes = [a if torch.is_tensor(a) else torch.as_tensor(a) for a in axes]
    d = len(axes)
    if not 1 <= d <= 3:
        raise ValueError(f"{what}: axes must hold 1, 2 or 3 coordinate vectors (got {d})")
    shape = tuple(int(m) for m in (_per_axis(n_modes) or (n_modes,)))
    if len(shape) != d:
        raise ValueError(f"{what}: n_modes has {len(shape)} mode counts for {d} axes")
    hv = _per_axis(h)
    hv = tuple(float(v) for v in hv) if hv is not None else (float(h),) * d
    if len(hv) != d:
        raise ValueError(f"{what}: h has {len(hv)} spacings for {d} axes")
    for a, ax in enumerate(axes):
        if ax.ndim != 1:
            raise ValueError(f"{what}: axes[{a}] must be 1-D (got shape {tuple(ax.shape)})")
        if ax.numel() == 0:
            raise ValueError(f"{what}: axes[{a}] is empty")
    if any(m < 1 for m in shape):
        raise ValueError(f"{what}: n_modes must be positive (got {shape})")
    return axes, hv, shape


def raster_plan(n_axis, n_modes, nbatch=1, max_workspace_bytes=0):
    """Slabs and workspace of a raster_type2 call on a raster of n_axis cells per axis (efgp_raster_plan, host only):
    dict(slab_rows, slabs, workspace_bytes).  ValueError when the cap cannot hold the phase tables and one 16-row slab."""
    n_axis = tuple(int(n) for n in (_per_axis(n_axis) or (n_axis,)))
    shape = tuple(int(m) for m in (_per_axis(n_modes) or (n_modes,)))
    if len(n_axis) != len(shape) or not 1 <= len(shape) <= 3:
        raise ValueError(f"raster_plan: n_axis has {len(n_axis)} entries and n_modes {len(shape)}; both must have 1, 2 or 3")
    rows, slabs, nbytes = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().efgp_raster_plan(len(shape), _i64(shape), _i64(n_axis), int(nbatch), int(max_workspace_bytes), C.byref(rows), C.byref(slabs),
                                 C.byref(nbytes)), "efgp_raster_plan")
    return dict(slab_rows=rows.value, slabs=slabs.value, workspace_bytes=nbytes.value)


def raster_type2(axes, h, n_modes, f, *, modeord=0, isign=+1, mode_scale=None, xcen=None, batched=None, max_workspace_bytes=0, out=None):
    """Exact type-2 transform onto the rectilinear raster axes[0] x .. x axes[d-1] ("ij" order), real part only (efgp_raster_type2):

        out[b, j0..] = Re sum_k (f[b,k] * mode_scale[k]) exp(isign 2 pi i sum_a h[a] k_a (axes[a][j_a] - xcen[a]))

    axes: d one-dimensional tensors (any spacing, any order); h: one spacing or d; f (prod,) | (*n_modes) | (B, ...) complex;
    returns float64 (*n_axis) or (B, *n_axis) on the GPU.  No window and no tolerance: the sum separates per axis.  Bitwise
    repeatable, independent of max_workspace_bytes (0: the library's default cap of the pooled workspace).  `out`: a contiguous
    float64 tensor of the result's size to write into."""
    axes, hv, shape = _raster_args("raster_type2", axes, h, n_modes)
    d, M = len(shape), math.prod(shape)
    if not torch.is_tensor(f):
        f = torch.as_tensor(f)
    if f.numel() == 0 or f.numel() % M:
        raise ValueError(f"raster_type2: f has {f.numel()} entries, the mode box {shape} has {M}")
    if batched is None:
        batched = not (f.ndim == 1 or tuple(f.shape) == shape)
    if not batched and f.numel() != M:
        raise ValueError(f"raster_type2: f has {f.numel()} entries, the mode box {shape} has {M}")
    if xcen is not None:
        xc = _per_axis(xcen)
        xc = tuple(float(v) for v in xc) if xc is not None else (float(xcen),) * d
        if len(xc) != d:
            raise ValueError(f"raster_type2: xcen has {len(xc)} entries for {d} axes")
    if isign not in (-1, 1):
        raise ValueError(f"raster_type2: isign must be +1 or -1 (got {isign})")
    dev = compute_device(f, *axes)
    sc = None
    if mode_scale is not None:
        if mode_scale.numel() != M:
            raise ValueError(f"raster_type2: mode_scale has {mode_scale.numel()} entries, the mode box {shape} has {M}")
        sc = _dc(mode_scale.reshape(-1), dev, _CD)
    ff = _dc(f.reshape(-1, M), dev, _CD)
    B = ff.shape[0]
    n_axis = tuple(int(a.numel()) for a in axes)
    ax = _dc(axes[0], dev, _RD) if d == 1 else torch.cat([a.to(device=dev, dtype=_RD) for a in axes])
    if out is None:
        out = torch.empty((B,) + n_axis, dtype=_RD, device=dev)
    elif not (out.is_cuda and out.dtype is _RD and out.is_contiguous() and out.numel() == B * math.prod(n_axis)):
        raise ValueError("raster_type2: out must be a contiguous float64 GPU tensor of the result's size")
    with _on(dev):
        check(lib().efgp_raster_type2(dev.index, d, _i64(shape), _f64(hv), _f64(xc) if xcen is not None else None, _i64(n_axis), _ptr(ax),
                                      _ptr(ff), _ptr(sc) if sc is not None else None, B, int(isign), int(modeord), _ptr(out),
                                      int(max_workspace_bytes), _stream(dev)), "efgp_raster_type2")
    res = out.reshape((B,) + n_axis)
    return res if batched else res[0]


def mode_jet_rows(f, n_modes, h, *, mode_scale=None, modeord=0):
    """The coefficient rows of a trigonometric sum and of its d first partial derivatives (efgp_mode_jet_rows):

        out[b, 0, k] = mode_scale[k] f[b, k],      out[b, 1 + a, k] = (2 pi h[a] k_a) i out[b, 0, k]

    with k_a the mode number of slot k on axis a (-(n // 2) .. (n - 1) // 2; FFT order for modeord = 1).  f (M,) | (nrows, M)
    complex, M = prod n_modes; h: one spacing or d; mode_scale (M,) complex or None.  Returns (nrows, 1 + d, M) complex128 on the
    GPU.  Wrong sizes are a ValueError before anything touches the device."""
    pa = _per_axis(n_modes)
    shape = tuple(int(m) for m in (pa if pa is not None else (n_modes,)))
    d = len(shape)
    if not 1 <= d <= 3:
        raise ValueError(f"mode_jet_rows: n_modes must hold 1, 2 or 3 mode counts (got {d})")
    if any(m < 1 for m in shape):
        raise ValueError(f"mode_jet_rows: n_modes must be positive (got {shape})")
    M = math.prod(shape)
    hv = _per_axis(h)
    hv = tuple(float(v) for v in hv) if hv is not None else (float(h),) * d
    if len(hv) != d:
        raise ValueError(f"mode_jet_rows: h has {len(hv)} spacings for {d} axes")
    if modeord not in (0, 1):
        raise ValueError(f"mode_jet_rows: modeord must be 0 or 1 (got {modeord})")
    if not torch.is_tensor(f):
        f = torch.as_tensor(f)
    if f.ndim not in (1, 2) or f.shape[-1] != M:
        raise ValueError(f"mode_jet_rows: f has shape {tuple(f.shape)}, the mode box {shape} has {M} entries per row")
    if mode_scale is not None and mode_scale.numel() != M:
        raise ValueError(f"mode_jet_rows: mode_scale has {mode_scale.numel()} entries, the mode box {shape} has {M}")
    dev = compute_device(f, mode_scale)
    ff = _dc(f.reshape(-1, M), dev, _CD)
    sc = _dc(mode_scale.reshape(-1), dev, _CD) if mode_scale is not None else None
    R = ff.shape[0]
    out = torch.empty((R, 1 + d, M), dtype=_CD, device=dev)
    with _on(dev):
        check(lib().efgp_mode_jet_rows(dev.index, d, _i64(shape), _f64(hv), _ptr(ff), _ptr(sc) if sc is not None else None, R,
                                       int(modeord), _ptr(out), _stream(dev)), "efgp_mode_jet_rows")
    return out


def raster_type2_jet(axes, h, n_modes, f, *, mode_scale=None, xcen=None):
    """Value and gradient of Re F (mode_scale * f) on the rectilinear raster axes[0] x .. x axes[d-1]: f (M,) | (nrows, M) complex ->
    (nrows, 1 + d, n_0, .., n_{d-1}) float64, entry [b, 0] the value and [b, 1 + a] the partial along axis a: the rows of
    `mode_jet_rows` through the exact `raster_type2` (its slab planning, its arguments)."""
    axes, hv, shape = _raster_args("raster_type2_jet", axes, h, n_modes)
    jets = mode_jet_rows(f, shape, hv, mode_scale=mode_scale)
    R, J, M = jets.shape
    res = raster_type2(axes, hv, shape, jets.view(R * J, M), batched=True, xcen=xcen)
    return res.view((R, J) + tuple(res.shape[1:]))


def raster_type1_plan(n_axis, n_modes, nbatch=1, max_workspace_bytes=0):
    """Slabs and workspace of a raster_type1 call from a raster of n_axis cells per axis (efgp_raster_type1_plan, host only):
    dict(slab_rows, slabs, workspace_bytes).  ValueError when the cap cannot hold the phase tables and one 16-row slab."""
    n_axis = tuple(int(n) for n in (_per_axis(n_axis) or (n_axis,)))
    shape = tuple(int(m) for m in (_per_axis(n_modes) or (n_modes,)))
    if len(n_axis) != len(shape) or not 1 <= len(shape) <= 3:
        raise ValueError(f"raster_type1_plan: n_axis has {len(n_axis)} entries and n_modes {len(shape)}; both must have 1, 2 or 3")
    rows, slabs, nbytes = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().efgp_raster_type1_plan(len(shape), _i64(shape), _i64(n_axis), int(nbatch), int(max_workspace_bytes), C.byref(rows),
                                       C.byref(slabs), C.byref(nbytes)), "efgp_raster_type1_plan")
    return dict(slab_rows=rows.value, slabs=slabs.value, workspace_bytes=nbytes.value)


def _checked_cell_scale(what, cell_scale, n_axis, dev):
    """cell_scale as a contiguous float64 tensor of the raster's size on `dev`; ValueError unless finite and >= 0."""
    if not torch.is_tensor(cell_scale):
        cell_scale = torch.as_tensor(cell_scale)
    if cell_scale.numel() != math.prod(n_axis):
        raise ValueError(f"{what}: cell_scale has {cell_scale.numel()} entries, the raster {n_axis} has {math.prod(n_axis)}")
    sc = _dc(cell_scale.reshape(-1), dev, _RD)
    if not bool((torch.isfinite(sc) & (sc >= 0)).all()):
        raise ValueError(f"{what}: cell_scale must be finite and >= 0")
    return sc


def raster_type1(axes, h, n_modes, values, *, cell_scale=None, modeord=0, isign=-1, xcen=None, batched=None, max_workspace_bytes=0, out=None,
                 _scale_checked=False):
    """Exact type-1 transform from the rectilinear raster axes[0] x .. x axes[d-1] ("ij" order) onto a mode box (efgp_raster_type1),
    the adjoint of `raster_type2`:

        out[b, k] = sum_j values[b, j] cell_scale[j] exp(isign 2 pi i sum_a h[a] k_a (axes[a][j_a] - xcen[a]))

    axes: d one-dimensional tensors (any spacing, any order); h: one spacing or d; values (prod n,) | (*n_axis) | (B, ...) real;
    cell_scale (*n_axis) real, finite and >= 0, or None: a cell whose scale is 0 is left out whatever its value holds (NaN included).
    Returns complex128 (*n_modes) or (B, *n_modes) on the GPU.  No window and no tolerance.  Bitwise repeatable, independent of
    max_workspace_bytes (0: the library's default cap of the pooled workspace).  `out`: a contiguous complex128 tensor of the
    result's size to write into."""
    axes, hv, shape = _raster_args("raster_type1", axes, h, n_modes)
    d, M = len(shape), math.prod(shape)
    n_axis = tuple(int(a.numel()) for a in axes)
    ncells = math.prod(n_axis)
    if not torch.is_tensor(values):
        values = torch.as_tensor(values)
    if values.is_complex():
        raise ValueError("raster_type1: values must be real")
    if values.numel() == 0 or values.numel() % ncells:
        raise ValueError(f"raster_type1: values has {values.numel()} entries, the raster {n_axis} has {ncells}")
    if batched is None:
        batched = not (values.ndim == 1 or tuple(values.shape) == n_axis)
    if not batched and values.numel() != ncells:
        raise ValueError(f"raster_type1: values has {values.numel()} entries, the raster {n_axis} has {ncells}")
    if xcen is not None:
        xc = _per_axis(xcen)
        xc = tuple(float(v) for v in xc) if xc is not None else (float(xcen),) * d
        if len(xc) != d:
            raise ValueError(f"raster_type1: xcen has {len(xc)} entries for {d} axes")
    if isign not in (-1, 1):
        raise ValueError(f"raster_type1: isign must be +1 or -1 (got {isign})")
    if modeord not in (0, 1):
        raise ValueError(f"raster_type1: modeord must be 0 or 1 (got {modeord})")
    dev = compute_device(values, *axes)
    sc = None
    if cell_scale is not None:
        sc = cell_scale if _scale_checked else _checked_cell_scale("raster_type1", cell_scale, n_axis, dev)
    vv = _dc(values.reshape(-1, ncells), dev, _RD)
    B = vv.shape[0]
    ax = _dc(axes[0], dev, _RD) if d == 1 else torch.cat([a.to(device=dev, dtype=_RD) for a in axes])
    if out is None:
        out = torch.empty((B,) + shape, dtype=_CD, device=dev)
    elif not (out.is_cuda and out.dtype is _CD and out.is_contiguous() and out.numel() == B * M):
        raise ValueError("raster_type1: out must be a contiguous complex128 GPU tensor of the result's size")
    with _on(dev):
        check(lib().efgp_raster_type1(dev.index, d, _i64(shape), _f64(hv), _f64(xc) if xcen is not None else None, _i64(n_axis), _ptr(ax),
                                      _ptr(vv), _ptr(sc) if sc is not None else None, B, int(isign), int(modeord), _ptr(out),
                                      int(max_workspace_bytes), _stream(dev)), "efgp_raster_type1")
    res = out.reshape((B,) + shape)
    return res if batched else res[0]


class RasterPlan:
    """The transforms of a model whose observations lie on the rectilinear raster axes[0] x .. x axes[d-1]: the part of the
    `NufftPlan` surface that a model uses on its training points, on `raster_type1` / `raster_type2` -- exact, with no point layout and no
    coordinate tensor.  "Points" are the raster cells in row-major order (`npts` of them); `cell_scale` (the raster's shape, finite,
    >= 0; a 0/1 mask of observed cells in the model) multiplies every type-1 input, and a cell of scale 0 is left out whatever
    the input holds there."""

    def __init__(self, axes, h, cell_scale=None, xcen=None, _scale_checked=False):
        if torch.is_tensor(axes) or not hasattr(axes, "__len__"):
            axes = [axes]
        axes, _, _ = _raster_args("RasterPlan", axes, h, (1,) * len(axes))
        self.dev = compute_device(*axes)
        self.axes = [_dc(a, self.dev, _RD) for a in axes]
        self.dim = len(self.axes)
        self.n_axis = tuple(int(a.numel()) for a in self.axes)
        self.npts = math.prod(self.n_axis)
        hv = _per_axis(h)
        self.h = tuple(float(v) for v in hv) if hv is not None else float(h)
        self.xcen = None if xcen is None else tuple(float(v) for v in xcen)
        # _scale_checked: a model makes a plan per fit over one mask it has checked once (the check reads back from the device)
        if cell_scale is not None and not _scale_checked:
            cell_scale = _checked_cell_scale("RasterPlan", cell_scale, self.n_axis, self.dev)
        self.scale = cell_scale
        self.probe_block_bytes = 256 << 20          # bound on the generated probe rows held at once

    def close(self):
        pass

    def _t1(self, values, n_modes, modeord=0, isign=-1, batched=None, scale=True, out=None):
        return raster_type1(self.axes, self.h, n_modes, values, cell_scale=self.scale if scale else None, modeord=modeord, isign=isign,
                            xcen=self.xcen, batched=batched, out=out, _scale_checked=True)

    def type1(self, c, n_modes, modeord=0, isign=-1):
        """c (ncells,) | (*n_axis) | (B, ...) real -> (B?, *n_modes) complex128."""
        if c.is_complex():
            raise NotImplementedError("RasterPlan.type1 takes real rows")
        return self._t1(c, n_modes, modeord, isign)

    def type1_ones(self, n_modes):
        """F* (cell_scale): with a scale, its raster transform; without one, the outer product of the d one-dimensional sums."""
        shape = tuple(int(m) for m in n_modes)
        if self.scale is not None:
            return self._t1(self.scale, shape, batched=False, scale=False)
        xc = self.xcen or (0.0,) * self.dim
        hs = self.h if isinstance(self.h, tuple) else (self.h,) * self.dim
        sums = [raster_type1([self.axes[a]], hs[a], (shape[a],), torch.ones(self.n_axis[a], dtype=_RD, device=self.dev), xcen=(xc[a],))
                for a in range(self.dim)]
        spec = {1: "i->i", 2: "i,j->ij", 3: "i,j,k->ijk"}[self.dim]
        return torch.einsum(spec, *sums).contiguous()

    def type1_pair(self, y, n_modes_y, n_modes_one):
        """(F* y on n_modes_y, F* 1 on n_modes_one) as two views of one buffer, like `NufftPlan.type1_pair`."""
        shape_y, shape_o = tuple(int(m) for m in n_modes_y), tuple(int(m) for m in n_modes_one)
        My, Mo = math.prod(shape_y), math.prod(shape_o)
        flat = torch.empty(My + Mo, dtype=_CD, device=self.dev)
        out_y, out_o = flat[:My].view(shape_y), flat[My:].view(shape_o)
        self._t1(y, shape_y, batched=False, out=out_y)
        out_o.copy_(self.type1_ones(shape_o))
        return out_y, out_o

    def _probe_blocks(self, nbatch):
        rows = max(2, self.probe_block_bytes // (8 * self.npts) // 2 * 2)         # even: normal rows come in pairs
        return [(b0, min(int(nbatch), b0 + rows)) for b0 in range(0, int(nbatch), rows)]

    def type1_rademacher(self, seed, nbatch, n_modes, index_offset=0, modeord=0):
        """F* Z for the rows Z = rademacher_fill(dev, seed, nbatch, ncells, index_offset), indexed by the row-major cell index and
        materialised a block of rows at a time -> (B, *n_modes).  Cells of scale 0 draw and are dropped."""
        out = torch.empty((int(nbatch),) + tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        for b0, b1 in self._probe_blocks(nbatch):
            z = rademacher_fill(self.dev, seed, b1 - b0, self.npts, _wrap_i64(int(index_offset) + b0 * NORMAL_ROW_STRIDE))
            self._t1(z, n_modes, modeord, batched=True, out=out[b0:b1])
        return out

    def type1_normal(self, seed, nbatch, n_modes, index_offset=0, modeord=0):
        """The same for the rows of normal_fill(dev, seed, nbatch, ncells, index_offset)."""
        out = torch.empty((int(nbatch),) + tuple(int(m) for m in n_modes), dtype=_CD, device=self.dev)
        for b0, b1 in self._probe_blocks(nbatch):
            z = normal_fill(self.dev, seed, b1 - b0, self.npts, normal_row_offset(b0, index_offset))
            self._t1(z, n_modes, modeord, batched=True, out=out[b0:b1])
        return out

    def type2(self, f, n_modes, modeord=0, real_only=False, isign=+1, batched=None, mode_scale=None):
        """f (prod,) | (*n_modes) | (B, ...) complex -> float64 (ncells,) | (B, ncells), cells in row-major order (raster_type2)."""
        if not real_only:
            raise NotImplementedError("RasterPlan.type2 returns the real part only (real_only=True): a complex output onto the raster "
                                      "is not implemented")
        shape = tuple(int(m) for m in n_modes)
        if batched is None:
            batched = not (f.ndim == 1 or tuple(f.shape) == shape)
        res = raster_type2(self.axes, self.h, shape, f, modeord=modeord, isign=isign, mode_scale=mode_scale, xcen=self.xcen, batched=True)
        res = res.reshape(res.shape[0], self.npts)
        return res if batched else res[0]


def cheb_interp(nodes_per_axis, weights_per_axis, node_values, x_new, clamp=True):
    """Tensor-product barycentric interpolation (efgp_cheb_interp): `nodes_per_axis` / `weights_per_axis` are d sequences (arrays,
    tensors) of the ascending nodes and their barycentric weights, `node_values` holds prod n_a doubles with the last axis fastest
    and `x_new` is (npts, d) on the GPU -> (npts,) float64 there, clamped at 0 when `clamp`.  Sizes are checked by the entry
    point (d 1..3, 2..64 nodes per axis, at most 4096 node values): a breach is a ValueError naming the argument."""
    dev = x_new.device
    xn = _dc(x_new, dev, _RD)
    if xn.ndim != 2:
        raise ValueError(f"cheb_interp: x_new must be (npts, d), got {tuple(xn.shape)}")
    npts, d = xn.shape
    if len(nodes_per_axis) != d or len(weights_per_axis) != d:
        raise ValueError(f"cheb_interp: {len(nodes_per_axis)} node axes and {len(weights_per_axis)} weight axes for {d}-D points")
    nd = [torch.as_tensor(a, dtype=_RD).reshape(-1) for a in nodes_per_axis]
    wt = [torch.as_tensor(a, dtype=_RD).reshape(-1) for a in weights_per_axis]
    counts = [int(a.numel()) for a in nd]
    if [int(a.numel()) for a in wt] != counts:
        raise ValueError("cheb_interp: every axis needs as many weights as nodes")
    vals = _dc(torch.as_tensor(node_values).reshape(-1), dev, _RD)
    if vals.numel() != math.prod(counts):
        raise ValueError(f"cheb_interp: {vals.numel()} node values for a node box of {tuple(counts)}")
    nodes = torch.cat(nd).to(dev)
    weights = torch.cat(wt).to(dev)
    out = torch.empty(npts, dtype=_RD, device=dev)
    with _on(dev):
        check(lib().efgp_cheb_interp(dev.index, d, _i64(counts), _ptr(nodes), _ptr(weights), _ptr(vals), _ptr(xn), npts, int(bool(clamp)),
                                     _ptr(out), _stream(dev)), "efgp_cheb_interp")
    return out


def spectral_weights_nd(dev, kind, nu, lengthscales, variance, hs, shape, want_grad=False):
    """(ws (M,), dprime (M, d + 1) or None) of an ARD kernel on the per-axis grid, complex128 on `dev`, in one launch
    (efgp_spectral_weights_nd)."""
    d = len(shape)
    if len(lengthscales) != d or len(hs) != d:
        raise ValueError("spectral_weights_nd: one lengthscale, spacing and mode count per axis")
    M = math.prod(int(n) for n in shape)
    ws = torch.empty(M, dtype=_CD, device=dev)
    dp = torch.empty((M, d + 1), dtype=_CD, device=dev) if want_grad else None
    with _on(dev):
        check(lib().efgp_spectral_weights_nd(dev.index, int(kind), d, float(nu), _f64(lengthscales), float(variance), _f64(hs),
                                             _i64(shape), _ptr(ws), _ptr(dp) if want_grad else None, _stream(dev)),
              "efgp_spectral_weights_nd")
    return ws, dp


def spectral_weights_host_nd(kind, nu, lengthscales, variance, hs, shape, want_grad=False):
    """The host twin (efgp_spectral_weights_host_nd): CPU complex128 tensors, no device involved."""
    d = len(shape)
    if len(lengthscales) != d or len(hs) != d:
        raise ValueError("spectral_weights_host_nd: one lengthscale, spacing and mode count per axis")
    M = math.prod(int(n) for n in shape)
    ws = torch.empty(M, dtype=_CD)
    dp = torch.empty((M, d + 1), dtype=_CD) if want_grad else None
    check(lib().efgp_spectral_weights_host_nd(int(kind), d, float(nu), _f64(lengthscales), float(variance), _f64(hs), _i64(shape),
                                              _ptr(ws), _ptr(dp) if want_grad else None), "efgp_spectral_weights_host_nd")
    return ws, dp


def pg_estep_update(s_rows, delta, targets, rho, *, probes=None, seed=0, pg_b=None):
    """The E-step's pass over the points (efgp_pg_estep_update): s_rows (J+1, N) float64 = [mean; S z_1..z_J]; probes (J, N) or
    None for the counter-hash probes of `seed`; delta (N,) is updated in place.  Returns (mean, sigma_diag, residual, correct) --
    residual (1,) float64 and correct (1,) int64 are device tensors (nothing is read back)."""
    dev = delta.device
    J = s_rows.shape[0] - 1
    N = delta.numel()
    for t_ in (s_rows, delta, targets) + tuple(t for t in (probes, pg_b) if t is not None):
        assert t_.is_cuda and t_.device == dev and t_.dtype == _RD and t_.is_contiguous()
    assert s_rows.shape == (J + 1, N) and targets.numel() == N
    assert probes is None or probes.shape == (J, N)
    assert pg_b is None or pg_b.numel() == N
    mean = torch.empty(N, dtype=_RD, device=dev)
    sdiag = torch.empty(N, dtype=_RD, device=dev)
    resid = torch.empty(1, dtype=_RD, device=dev)
    correct = torch.empty(1, dtype=torch.int64, device=dev)
    with _on(dev):
        check(lib().efgp_pg_estep_update(dev.index, N, J, _ptr(s_rows), _ptr(probes) if probes is not None else None,
                                         int(seed) & (2 ** 64 - 1), _ptr(pg_b) if pg_b is not None else None, _ptr(targets), float(rho),
                                         _ptr(delta), _ptr(mean), _ptr(sdiag), _ptr(resid), _ptr(correct), _stream(dev)),
              "efgp_pg_estep_update")
    return mean, sdiag, resid, correct


def pg_nb_estep_update(s_rows, delta, targets, total_count, rho, *, probes=None, seed=0, out=None):
    """The negative-binomial E-step pass (efgp_pg_nb_estep_update): as pg_estep_update with b = targets + total_count formed in
    the kernel.  Returns (mean, sigma_diag, scalars) -- scalars (2,) float64 on the device = [residual, sum_n |r exp(mean +
    max(sigma_diag, 0)/2) - y|] (one read-back for both); `out` may pass that (2,) buffer in."""
    dev = delta.device
    J = s_rows.shape[0] - 1
    N = delta.numel()
    for t_ in (s_rows, delta, targets) + ((probes,) if probes is not None else ()):
        assert t_.is_cuda and t_.device == dev and t_.dtype == _RD and t_.is_contiguous()
    assert s_rows.shape == (J + 1, N) and targets.numel() == N
    assert probes is None or probes.shape == (J, N)
    mean = torch.empty(N, dtype=_RD, device=dev)
    sdiag = torch.empty(N, dtype=_RD, device=dev)
    scalars = torch.empty(2, dtype=_RD, device=dev) if out is None else out
    assert scalars.dtype == _RD and scalars.device == dev and scalars.numel() == 2 and scalars.is_contiguous()
    with _on(dev):
        check(lib().efgp_pg_nb_estep_update(dev.index, N, J, _ptr(s_rows), _ptr(probes) if probes is not None else None,
                                            int(seed) & (2 ** 64 - 1), _ptr(targets), float(total_count), float(rho), _ptr(delta),
                                            _ptr(mean), _ptr(sdiag), _ptr(scalars), _ptr(scalars[1:]), _stream(dev)),
              "efgp_pg_nb_estep_update")
    return mean, sdiag, scalars


def pg_nb_total_count_grad(targets, mean, sigma_diag, total_count, nodes, weights, *, out=None):
    """sum_n [digamma(y + r) - digamma(r) + sum_q w_q logsigmoid(-(mean + sqrt(max(sigma_diag, 0)) x_q))]
    (efgp_pg_nb_total_count_grad) -> (1,) float64 on the device; nodes / weights: the (Q,) Gauss-Hermite rule, Q <= 128."""
    dev = mean.device
    N = mean.numel()
    for t_ in (targets, mean, sigma_diag, nodes, weights):
        assert t_.is_cuda and t_.device == dev and t_.dtype == _RD and t_.is_contiguous()
    assert targets.numel() == N and sigma_diag.numel() == N and nodes.numel() == weights.numel()
    grad = torch.empty(1, dtype=_RD, device=dev) if out is None else out
    with _on(dev):
        check(lib().efgp_pg_nb_total_count_grad(dev.index, N, _ptr(targets), _ptr(mean), _ptr(sigma_diag), float(total_count),
                                                nodes.numel(), _ptr(nodes), _ptr(weights), _ptr(grad), _stream(dev)),
              "efgp_pg_nb_total_count_grad")
    return grad


def pg_weight_rows(omega, nrows, *, probes=None, seed=0):
    """omega .* z for z = probes (nrows, N) or the counter-hash probes of `seed` (efgp_pg_weight_rows) -> (nrows, N) float64."""
    dev = omega.device
    N = omega.numel()
    assert omega.dtype == _RD and omega.is_contiguous()
    assert probes is None or (probes.dtype == _RD and probes.is_contiguous() and probes.shape == (int(nrows), N))
    out = torch.empty((int(nrows), N), dtype=_RD, device=dev)
    with _on(dev):
        check(lib().efgp_pg_weight_rows(dev.index, N, int(nrows), _ptr(probes) if probes is not None else None, int(seed) & (2 ** 64 - 1),
                                        _ptr(omega), _ptr(out), _stream(dev)), "efgp_pg_weight_rows")
    return out


def pg_mstep_terms(beta_x, beta_probes, r_probes, dprime):
    """term1 | term2 | grad of the PG M-step as ONE device vector of 3 P doubles (efgp_pg_mstep_terms); dprime (M, P) real or
    complex (real part read)."""
    dev = beta_x.device
    M = beta_x.numel()
    J = beta_probes.shape[0] if beta_probes is not None else 0
    P = dprime.shape[1]
    for t_ in (beta_x,) + ((beta_probes, r_probes) if J else ()):
        assert t_.is_cuda and t_.dtype == _CD and t_.is_contiguous()
    assert dprime.is_contiguous() and dprime.dtype in (_CD, _RD) and dprime.shape == (M, P)
    assert J == 0 or (beta_probes.numel() == J * M and r_probes.numel() == J * M)
    out = torch.empty(3 * P, dtype=_RD, device=dev)
    with _on(dev):
        check(lib().efgp_pg_mstep_terms(dev.index, M, J, P, _ptr(beta_x), _ptr(beta_probes) if J else None, _ptr(r_probes) if J else None,
                                        _ptr(dprime), int(dprime.is_complex()), _ptr(out), _stream(dev)), "efgp_pg_mstep_terms")
    return out


class RcclComm:
    """Sum / min / max all-reduce and broadcast over RCCL without a torch process group (C ABI: efgp_comm_*).
    `unique_id` (128 bytes) comes from `RcclComm.make_id()` on rank 0 and reaches the other ranks by the caller's channel."""

    @staticmethod
    def make_id():
        buf = (C.c_char * 128)()
        check(lib().efgp_comm_unique_id(buf), "efgp_comm_unique_id")
        return bytes(buf)

    def __init__(self, dev, rank, world, unique_id):
        assert len(unique_id) == 128
        self.dev, self.rank, self.world = dev, int(rank), int(world)
        self._h = C.c_void_p()
        with _on(dev):
            check(lib().efgp_comm_init(C.byref(self._h), dev.index, self.rank, self.world, C.c_char_p(unique_id)), "efgp_comm_init")

    def all_reduce_sum_(self, t):
        buf = torch.view_as_real(t) if t.is_complex() else t
        assert buf.is_cuda and buf.dtype == _RD and buf.is_contiguous()
        with _on(self.dev):
            check(lib().efgp_comm_allreduce_sum(self._h, _ptr(buf), buf.numel(), _stream(self.dev)), "efgp_comm_allreduce_sum")
        return t

    def all_reduce_minmax_(self, t, take_max):
        assert t.is_cuda and t.dtype == _RD and t.is_contiguous()
        with _on(self.dev):
            check(lib().efgp_comm_allreduce_minmax(self._h, _ptr(t), t.numel(), int(bool(take_max)), _stream(self.dev)),
                  "efgp_comm_allreduce_minmax")
        return t

    def broadcast_(self, t, root=0):
        assert t.is_cuda and t.is_contiguous()
        with _on(self.dev):
            check(lib().efgp_comm_broadcast(self._h, _ptr(t), t.numel() * t.element_size(), int(root), _stream(self.dev)),
                  "efgp_comm_broadcast")
        return t

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().efgp_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vdot_real(a, b):
    """Re <a, b> = Re sum conj(a) b for real or complex device vectors, reduced by the HIP kernel."""
    dev = a.device
    aa = a.reshape(-1).to(_CD if a.is_complex() else _RD).contiguous()
    bb = b.reshape(-1).to(device=dev, dtype=_CD if b.is_complex() else _RD).contiguous()
    out = C.c_double(0.0)
    with _on(dev):
        check(lib().efgp_vdot_real(dev.index, _ptr(aa), int(aa.is_complex()), _ptr(bb), int(bb.is_complex()),
                                   aa.numel(), C.byref(out), _stream(dev)), "efgp_vdot_real")
    return float(out.value)


def gradient_step(xd, yd, points, *, h, mtot, kconst, lengthscale, variance, sigmasq, tol_pair, tol_probe, cg_tol, early_stop,
                  nprobes, probe_seed, v_seed, use_mean_pc, use_trace_pc, variance_idx, trace_idx, beta0, n_obs, yy):
    """One hyper-gradient step of the adjoint estimator in ONE library call (efgp_gradient_step; csrc/gradient_step.cpp).
    kconst = (kind, nu, c0) of utils.kernels.kernel_constants.  Returns (out_vec, beta, mean LazyIterations, trace
    LazyIterations) -- all device-resident, nothing read back -- or None when the grid's solves are not single launches."""
    dev = xd.device
    npts, d = xd.shape
    M = int(mtot) ** d
    K = len(trace_idx)
    R = (K + 1) * int(nprobes)
    out = torch.empty(3 * 3 + 1, dtype=_RD, device=dev)
    beta = torch.empty(M, dtype=_CD, device=dev)
    its = torch.empty(1 + R, dtype=torch.int32, device=dev)
    tix = (C.c_int * max(1, K))(*[int(i) for i in trace_idx])
    b0 = _dc(beta0.reshape(-1), dev, _CD) if beta0 is not None else None
    with _on(dev):
        rc = lib().efgp_gradient_step(points._h if points is not None else None, dev.index, int(d), int(npts), _ptr(xd), _ptr(yd),
                                      float(h), int(mtot), int(kconst[0]), float(kconst[1]), float(lengthscale), float(variance),
                                      float(kconst[2]), float(sigmasq), float(tol_pair), float(tol_probe), float(cg_tol),
                                      int(bool(early_stop)), int(nprobes), int(probe_seed) & (2 ** 64 - 1), int(v_seed) & (2 ** 64 - 1),
                                      int(bool(use_mean_pc)), int(bool(use_trace_pc)), -1 if variance_idx is None else int(variance_idx),
                                      K, tix, _ptr(b0) if b0 is not None else None, float(n_obs), float(yy), _ptr(beta), _ptr(out),
                                      _ptr(its), _ptr(its[1:]), _stream(dev))
    if rc == EFGP_EUNSUPPORTED:
        return None
    check(rc, "efgp_gradient_step")
    return out, beta, LazyIterations(its[:1], False, 2 * M), LazyIterations(its[1:], True, 2 * M)


def normal_fill(dev, seed, nbatch, npts, index_offset=0):
    """The standard normals `NufftPlan.type1_normal` uses, materialised as a (nbatch, npts) float64 tensor."""
    out = torch.empty((int(nbatch), int(npts)), dtype=_RD, device=dev)
    with _on(dev):
        check(lib().efgp_normal_fill(dev.index, int(seed) & (2 ** 64 - 1), _wrap_i64(index_offset), int(nbatch), int(npts),
                                     _ptr(out), _stream(dev)), "efgp_normal_fill")
    return out


def hermitian_normal_rows(dev, seed, nrows, nmodes, a=0.0, ws=None, fz=None, b=1.0, index_offset=0):
    """(nrows, nmodes) complex128: a * ws * fz + b * e with e a conjugate-even standard complex normal row generated in the
    kernel (efgp_hermitian_normal_rows; e is defined through `normal_fill(dev, seed, 2 * nrows, nmodes, index_offset)`).
    ws (nmodes,) and fz (nrows, nmodes) go together or are both None (then the result is b * e).  ws and the rows of fz must be
    conjugate-even (real, even spectral weights; transforms of real rows): the kernel reads their lower halves only and writes
    the upper half of the result as the conjugate of the lower."""
    nrows, nmodes = int(nrows), int(nmodes)
    if (ws is None) != (fz is None):
        raise ValueError("hermitian_normal_rows: ws and fz go together (both or neither)")
    out = torch.empty((nrows, nmodes), dtype=_CD, device=dev)
    wsc = fzc = None
    if ws is not None:
        wsc = _dc(ws.reshape(-1), dev, _CD)
        fzc = _dc(fz.reshape(nrows, -1), dev, _CD)
        if wsc.numel() != nmodes or fzc.shape[1] != nmodes:
            raise ValueError(f"hermitian_normal_rows: ws has {wsc.numel()} and fz {fzc.shape[1]} entries per row, expected {nmodes}")
    with _on(dev):
        check(lib().efgp_hermitian_normal_rows(dev.index, int(seed) & (2 ** 64 - 1), _wrap_i64(index_offset), nrows, nmodes, float(a),
                                               _ptr(wsc) if wsc is not None else None, _ptr(fzc) if fzc is not None else None,
                                               float(b), _ptr(out), _stream(dev)), "efgp_hermitian_normal_rows")
    return out


def rademacher_fill(dev, seed, nbatch, npts, index_offset=0):
    """The +-1 probes `NufftPlan.type1_rademacher` uses, materialised as a (nbatch, npts) float64 tensor."""
    out = torch.empty((int(nbatch), int(npts)), dtype=_RD, device=dev)
    with _on(dev):
        check(lib().efgp_rademacher_fill(dev.index, int(seed) & (2 ** 64 - 1), int(index_offset), int(nbatch), int(npts),
                                         _ptr(out), _stream(dev)), "efgp_rademacher_fill")
    return out


def kernel_timing(enable, only=None):
    """HIP-event timers around the library's main launches; `only`: record the launches of this name alone (every timed
    launch puts two event records into the stream)."""
    check(lib().efgp_kernel_timing_only(only.encode() if only else None), "efgp_kernel_timing_only")
    check(lib().efgp_kernel_timing(int(bool(enable))), "efgp_kernel_timing")


def kernel_timing_read(name):
    """-> (total milliseconds, launches) of the named kernel since kernel_timing(True)."""
    ms = C.c_double(0.0)
    n = C.c_int64(0)
    check(lib().efgp_kernel_timing_read(name.encode(), C.byref(ms), C.byref(n)), "efgp_kernel_timing_read")
    return float(ms.value), int(n.value)


class cg_residual_history:
    """Context manager: records row 0's relative residuals |r_i| / |b| of the CG solves enqueued inside it
    (efgp_cg_record_history).  `.values()` -> 1-D float64 tensor of the recorded iterations (zeros beyond the last)."""

    def __init__(self, dev, capacity=4096):
        self.buf = torch.zeros(int(capacity), dtype=_RD, device=dev)

    def __enter__(self):
        check(lib().efgp_cg_record_history(_ptr(self.buf), self.buf.numel()), "efgp_cg_record_history")
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize(self.buf.device)
        check(lib().efgp_cg_record_history(None, 0), "efgp_cg_record_history")
        return False

    def values(self):
        return self.buf.detach().cpu()
