"""EFGP (equispaced-Fourier Gaussian process) regression on MI355X -- host side.

Drop-in for the reference module of the same name (danbider/gp-quadrature `efgpnd.py`): the
public names, argument meanings and error behaviour follow it (`EFGPND`, `efgpnd_gradient_batched`,
`efgp_nd`, `NUFFT`, `ToeplitzND`, `compute_convolution_vector_vectorized_dD`, `create_A_mean`, ...),
but every hot operation -- NUFFT spreading/interpolation, the FFT Toeplitz mat-vec, the
preconditioned CG iterations and the N-length reductions -- runs in hand-written HIP kernels
behind the C ABI of `libefgp_hip.so` (include/efgp_hip.h).  torch tensors carry device memory,
streams and (for multi-GPU) the process group; there is no CPU fallback: without a GPU or without
the built library the solve raises RuntimeError.

Maths (reference conventions): features F[n,k] = exp(2 pi i h k.x_n) on the tensor grid
k in {-m..m}^d, weights ws = sqrt(S(h k) h^d); F* = type-1 NUFFT, F = type-2; F*F is the Toeplitz
operator T with vector v[k] = sum_n exp(-2 pi i h k.x_n), |k| <= 2m; the posterior-mean weights
solve (D T D + sigma^2 I) beta = D F* y  (D = diag ws) by Jacobi-preconditioned CG.
"""
from __future__ import annotations

import math
import os
import time
import warnings
from functools import partial
from math import prod
from typing import Dict, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn
from torch.optim import Adam

from cg import ConjugateGradients
from kernels.kernel_params import GPParams
from utils.kernels import get_xis, get_xis_nd

from efgp_hip import NufftPlan, PointSet, ToeplitzOp, lanczos, lag_sums, variance_rhs, variance_contract, cg_solve, cg_solve_lazy, cg_solve_mean_async, cg_solve_mean_fused, vdot_real, compute_device, rademacher_fill, gradient_prepare, gradient_assemble, hermitian_normal_rows, normal_row_offset, spectral_weights_nd, raster_type2, raster_type2_jet, RasterPlan
from efgp_hip.dist import PointShards
from efgp_hip.ops import _per_axis, _SAMPLE_BLOCK

TWO_PI = 2.0 * math.pi
_CONV_TOL = 6e-8       # tolerance the reference hard-codes for the Toeplitz vector (efgpnd.py:1418)


class _StageRanges:
    """roctx ranges named after the reference's stage timers (efgpnd.py:61-280 `stage_times`, :888-966 predict), so that a
    `rocprofv3 --marker-trace --kernel-trace` timeline of a gradient step or a prediction reads by stage.  Off unless
    EFGP_ROCTX=1 (a push / pop pair costs about a microsecond of host time each; a 0.4-ms step has ten stages).
    torch.cuda.nvtx IS roctx on ROCm builds.  Stage names are known when a stage ENDS (`lap(name)`), so the range of the
    stage that follows is opened from the fixed order below."""
    ORDER = ["0_book_keeping", "1_frequency_grid_setup", "2_nufft_setup", "3_toeplitz_setup", "4_solve_cg", "5_compute_term2",
             "6_monte_carlo_trace", "7_batch_cg_solve", "7.5_compute_alpha", "8_gradient_calculation", "9_log_marginal_likelihood"]
    enabled = os.environ.get("EFGP_ROCTX", "0") == "1"

    def __init__(self, outer, first=None):
        self.depth = 0
        if self.enabled:
            self._push(outer)
            if first is not None:
                self._push(first)

    def _push(self, name):
        torch.cuda.nvtx.range_push(name)
        self.depth += 1

    def _pop(self):
        if self.depth > 0:
            torch.cuda.nvtx.range_pop()
            self.depth -= 1

    def lap(self, name):
        """Stage `name` has ended: close its range, open the one of the stage that follows it."""
        if not self.enabled:
            return
        if self.depth > 1:
            self._pop()
        k = self.ORDER.index(name) if name in self.ORDER else -1
        if 0 <= k < len(self.ORDER) - 1:
            self._push(self.ORDER[k + 1])

    def stage(self, name):
        """Open a named range inside the outer one (predict: 'predict_mean', 'compute_variance')."""
        if self.enabled:
            if self.depth > 1:
                self._pop()
            self._push(name)

    def close(self):
        while self.depth > 0:
            self._pop()


def _cmplx(real_dtype: torch.dtype) -> torch.dtype:
    """complex dtype matching a real dtype (reference: efgpnd.py:1233-1234)."""
    return torch.complex64 if real_dtype == torch.float32 else torch.complex128


def _as2d(x: torch.Tensor) -> torch.Tensor:
    return x.unsqueeze(-1) if x.ndim == 1 else x


def _dev_points(x: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """(N,d) float64 contiguous copy (or view) of x on the compute device."""
    return _as2d(x).detach().to(device=dev, dtype=torch.float64).contiguous()


# ======================================================================================
# NUFFT  (reference: efgpnd.py:1423-1549)
# ======================================================================================
class NUFFT:
    """Type-1 (points -> modes, F*) and type-2 (modes -> points, F) transforms for fixed points.

    ``NUFFT(x, xcen, h, eps, cdtype=None, device=None)``: x (N,d), phases phi = 2 pi h (x - xcen),
    requested accuracy ``eps``.  Results come back on ``device or x.device`` in ``cdtype``.
    """

    def __init__(self, x, xcen, h, eps, cdtype=None, device=None):
        self.device = device or x.device
        self.dtype = x.dtype
        self.cdtype = cdtype or _cmplx(self.dtype)
        self.eps = eps
        self._hval = tuple(float(v) for v in _per_axis(h)) if _per_axis(h) is not None else float(h)      # per-axis spacings: a sequence of d
        x2 = _as2d(x)
        self.d = x2.shape[1]
        if torch.is_tensor(xcen):
            self._xcen = [float(v) for v in xcen.detach().reshape(-1).tolist()]
        elif xcen is None:
            self._xcen = [0.0] * self.d
        else:
            self._xcen = [float(v) for v in np.atleast_1d(xcen)]
        if len(self._xcen) == 1 and self.d > 1:
            self._xcen = self._xcen * self.d
        self._dev = compute_device(x, device=self.device)
        self._x = _dev_points(x2, self._dev)
        self._plan = NufftPlan(self._x, self._hval, float(eps), self._xcen)
        self._x_ref = x2

    @property
    def phi(self) -> torch.Tensor:
        """(d,N) phases, as the reference exposes them (efgpnd.py:1451)."""
        xc = torch.tensor(self._xcen, dtype=self._x_ref.dtype, device=self._x_ref.device)
        hv = torch.tensor(self._hval, dtype=self._x_ref.dtype, device=self._x_ref.device) if isinstance(self._hval, tuple) else self._hval
        return (TWO_PI * hv * (self._x_ref - xc)).T.contiguous().to(device=self.device, dtype=self.dtype)

    # device-level entry points (cuda tensors in, cuda complex128 out) used inside this module
    def _type1_dev(self, vals, out_shape):
        return self._plan.type1(vals, tuple(out_shape))

    def _type2_dev(self, fk, out_shape, modeord=0, real_only=False, batched=None):
        return self._plan.type2(fk, tuple(out_shape), modeord=modeord, real_only=real_only, batched=batched)

    def type1(self, vals, out_shape):
        """f[k] = sum_n vals_n exp(-i k.phi_n); vals (N,) or (B,N) -> (*out_shape) or (B,*out_shape)."""
        if isinstance(out_shape, int):
            out_shape = (out_shape,)
        res = self._type1_dev(vals.detach(), out_shape)
        return res.to(device=self.device, dtype=self.cdtype)

    def type2(self, fk, out_shape=None):
        """c_n = sum_k fk[k] exp(+i k.phi_n); fk flat (M,)/(B,M) with out_shape, or already shaped."""
        fk = fk.detach()
        if out_shape is None:
            if fk.ndim == self.d:
                shape, batched = tuple(fk.shape), False
            elif fk.ndim == self.d + 1:
                shape, batched = tuple(fk.shape[1:]), True
            else:
                raise ValueError("type2 needs out_shape for flattened input")
        else:
            if isinstance(out_shape, int):
                out_shape = (out_shape,)
            shape = tuple(out_shape)
            batched = fk.ndim > 1 and tuple(fk.shape) != shape
        res = self._type2_dev(fk, shape, batched=batched)
        return res.to(device=self.device, dtype=self.cdtype)


def setup_nufft(x, xcen, h, nufft_eps, cdtype):
    """Deprecated shim kept for import compatibility (reference: efgpnd.py:1551-1568)."""
    op = NUFFT(x, xcen, h, nufft_eps, cdtype=cdtype)
    return op.phi, (lambda phi_in, vals, OUT=None: op.type1(vals, out_shape=OUT)), \
        (lambda phi_in, fk_flat, OUT=None: op.type2(fk_flat, out_shape=OUT))


def compute_convolution_vector_vectorized_dD(m: int, x: torch.Tensor, h) -> torch.Tensor:
    """v[k] = sum_n exp(-2 pi i h k.x_n) for k in [-2m, 2m]^d (reference: efgpnd.py:1395-1421)."""
    x2 = _as2d(x)
    dev = compute_device(x2)
    plan = NufftPlan(_dev_points(x2, dev), float(h), _CONV_TOL)
    v = plan.type1_ones((4 * m + 1,) * x2.shape[1])
    return v.to(device=x.device, dtype=_cmplx(x.dtype))


# ======================================================================================
# Toeplitz operator (reference: efgpnd.py:1239-1393)
# ======================================================================================
class ToeplitzND:
    """y = T x with T[j,l] = v[j-l]; v has shape (L_1..L_d), blocks n_a = (L_a+1)//2.

    Accepts flat ``(..., prod n)`` or block ``(..., n_1..n_d)`` inputs like the reference; the
    circulant embedding (pad, rocFFT, multiply by the cached transform of v, inverse, crop) runs in
    libefgp_hip.  ``precompute_fft`` is accepted for compatibility; the transform of v is always cached.
    """

    def __init__(self, v: torch.Tensor, *, force_pow2: bool = True, precompute_fft: bool = True, defer_spectra: bool = False):
        if not torch.is_complex(v):
            v = v.to(torch.complex128 if v.dtype == torch.float64 else torch.complex64)
        self.Ls = list(v.shape)
        self.ns = [(L + 1) // 2 for L in self.Ls]
        self.size = prod(self.ns)
        self.d = len(self.Ls)
        self.device = v.device
        self.dtype = v.dtype
        self._dev = compute_device(v)
        self._op = ToeplitzOp(v.detach().to(self._dev), force_pow2=force_pow2, defer_spectra=defer_spectra)
        self.fft_shape = list(self._op.fft_shape)
        self.starts = [n - 1 for n in self.ns]
        self.ends = [s + n for s, n in zip(self.starts, self.ns)]

    def _apply_dev(self, u_flat):
        return self._op.apply(u_flat)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape[-1] == self.size:
            flat_in = True
            lead = x.shape[:-1]
        elif list(x.shape[-self.d:]) == self.ns:
            flat_in = False
            lead = x.shape[:-self.d]
        else:
            raise ValueError(f"Expected trailing dim {self.size} or block {tuple(self.ns)}, got {tuple(x.shape)}")
        out_dtype = x.dtype if x.is_complex() else self.dtype
        y = self._op.apply(x.detach().reshape(*lead, self.size))
        y = y if flat_in else y.reshape(*lead, *self.ns)
        return y.to(device=x.device if x.is_cuda else self.device, dtype=out_dtype)


# ======================================================================================
# operators on feature space (reference: efgpnd.py:1572-1631)
# ======================================================================================
class _FeatureOperator:
    """u -> ws*T(ws*u) [kind 'G'], + sigma^2 u ['mean'], or /sigma^2 + u ['var'].

    Callable like the reference's closures; additionally recognised by `ConjugateGradients`,
    which then runs the whole solve inside the fused HIP CG (`efgp_cg_solve`)."""

    def __init__(self, ws, toeplitz, sigmasq, cdtype, kind):
        self.ws = ws
        self.toeplitz = toeplitz
        self.sigmasq = None if sigmasq is None else float(sigmasq)
        self.cdtype = cdtype
        self.kind = kind
        self.variant = {"mean": 0, "var": 1}.get(kind, -1)
        self._efgp_fusable = kind in ("mean", "var")

    def __call__(self, u):
        u = u.to(dtype=self.cdtype)
        ws = self.ws.to(u.device)
        g = ws * self.toeplitz(ws * u)
        if self.kind == "mean":
            return g + self.sigmasq * u
        if self.kind == "var":
            return g / self.sigmasq + u
        return g


def create_Gv(ws, toeplitz, cdtype):
    return _FeatureOperator(ws, toeplitz, None, cdtype, "G")


def create_A_mean(ws, toeplitz, sigmasq_scalar, cdtype):
    return _FeatureOperator(ws, toeplitz, sigmasq_scalar, cdtype, "mean")


def create_A_var(ws, toeplitz, sigmasq_scalar, cdtype):
    return _FeatureOperator(ws, toeplitz, sigmasq_scalar, cdtype, "var")


def setup_operators(ws, toeplitz, sigmasq_scalar, cdtype):
    return (create_A_mean(ws, toeplitz, sigmasq_scalar, cdtype), create_A_var(ws, toeplitz, sigmasq_scalar, cdtype),
            create_Gv(ws, toeplitz, cdtype))


class _JacobiPreconditioner:
    """v -> v / (diag_scale |ws|^2 + sigma^2)  (reference: efgpnd.py:1619-1631)."""
    _efgp_jacobi = True

    def __init__(self, ws, sigmasq_scalar, diag_scale):
        scale = diag_scale if torch.is_tensor(diag_scale) else float(diag_scale)
        sig = sigmasq_scalar.detach() if torch.is_tensor(sigmasq_scalar) else float(sigmasq_scalar)
        self.diag = (scale * ws.abs().pow(2).real + sig).detach()

    def __call__(self, v):
        return v / self.diag.to(v.device)


def create_jacobi_precond(ws, sigmasq_scalar, diag_scale=1.0):
    return _JacobiPreconditioner(ws, sigmasq_scalar, diag_scale)


# ======================================================================================
# shared pieces of fit / gradient
# ======================================================================================
class _PinnedStage:
    """Two reusable pinned staging buffers per device (grown on demand), each guarded by the event of its last copy."""

    def __init__(self):
        self.bufs = [None, None]
        self.events = [None, None]
        self.turn = 0

    def upload(self, t: torch.Tensor, dev: torch.device) -> torch.Tensor:
        src = t.contiguous()
        raw = src.reshape(-1).view(torch.uint8)
        nbytes = raw.numel()
        k = self.turn
        self.turn ^= 1
        if self.events[k] is not None:
            self.events[k].synchronize()          # the copy issued two uploads ago: long finished in steady state
        if self.bufs[k] is None or self.bufs[k].numel() < nbytes:
            self.bufs[k] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        self.bufs[k][:nbytes].copy_(raw)
        out = torch.empty(src.shape, dtype=src.dtype, device=dev)
        out.reshape(-1).view(torch.uint8).copy_(self.bufs[k][:nbytes], non_blocking=True)
        if self.events[k] is None:
            self.events[k] = torch.cuda.Event()
        self.events[k].record(torch.cuda.current_stream(dev))
        return out


_STAGES: Dict[int, Optional[_PinnedStage]] = {}


def _upload(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """Host -> device copy that does not stall the host: a pageable-memory copy makes the host wait until the stream
    has drained (measured: the weights' upload at the top of every fit exposed ~50 us of launch gaps per step at
    N = 1e6).  Staged through a persistent pinned buffer the copy is just another stream-ordered operation
    (`Tensor.pin_memory()` per call is no alternative: 14 ms per call measured for a 292-KB grid)."""
    if t.device.type == "cpu" and dev.type == "cuda" and t.numel() > 0 and not os.environ.get("EFGP_NO_PINNED_UPLOAD"):
        stage = _STAGES.setdefault(dev.index or 0, _PinnedStage())
        if stage is not None:
            try:
                with torch.cuda.device(dev):
                    return stage.upload(t, dev)
            except RuntimeError:          # no pinned memory to be had (locked-memory limit): plain copies from now on
                _STAGES[dev.index or 0] = None
    return t.to(dev)


class _Grid:
    """Frequency grid and weights for the current hyper-parameters (host scalars + device vectors)."""

    def __init__(self, kernel, eps, L, d, dev, want_grad=False, defer_weights=False, trunc_eps=None):
        """defer_weights=True: only the grid (h, mtot) is set up; the caller enqueues the N-scale pass over the points -- which
        needs nothing else -- and calls `make_weights` behind it (the gradient step waits for its result on the host every step,
        so what the host does before the first big launch is dead time on the device: ~35 us of a 0.4-ms step).
        trunc_eps: tolerance of the frequency truncation when it differs from `eps` (get_xis; the PG classifier passes its
        spectral_eps and trunc_eps separately, pg_classifier.py:326-333); None keeps trunc_eps = eps."""
        self.ard = hasattr(kernel, "ard_kind")
        self.d = d
        if self.ard:
            # one lengthscale per axis (kernels/ard.py): a spacing and a mode count per axis, L = the d sides of the bounding box
            if not isinstance(L, (tuple, list)):
                raise ValueError(f"{type(kernel).__name__} needs the box side of every axis, got one length")
            self.hs, self.shape = get_xis_nd(kernel, eps, L, trunc_eps=trunc_eps)
            self.h = self.mtot = None       # scalars of the isotropic grid only; `hs` / `shape` describe every grid
            self.plan_h = self.hs
            self.M = prod(self.shape)
            self.hprod = prod(self.hs)
            self.xis_axes = [torch.arange(-(n // 2), n // 2 + 1, dtype=torch.float64) * hj for hj, n in zip(self.hs, self.shape)]
        else:
            xis_1d, h, mtot = get_xis(kernel_obj=kernel, eps=eps, L=L, use_integral=True, l2scaled=False, trunc_eps=trunc_eps)
            self.h = float(h)
            self.mtot = int(mtot)
            self.hs = (self.h,) * d
            self.shape = (self.mtot,) * d
            self.M = self.mtot ** d
            self.hprod = self.h ** d
            self.plan_h = self.h            # what a NufftPlan takes: one spacing here, the d spacings of an ARD grid
            self.xis_1d = xis_1d
            self.xis_axes = [xis_1d] * d
        self._xis = None                                                         # (M,d) host float64, built on first use
        # Non-blocking uploads where the whole solve is one launch (circulant grid small enough for the persistent kernel:
        # F^d <= 4096 with F = next_pow2(2 mtot - 1)) -- that is where the host running ahead pays (launch gaps of the
        # N = 1e6 step).  The multi-kernel solves synchronise with the device per burst anyway and keep the plain copy
        # (with torch's CPU pool capped, EFGP_ASYNC_UPLOAD_ALL=1 measures 7.11 vs 7.28 ms on the 3-D 64^3 fit and no
        # difference at 2-D 256^2; with an uncapped pool under a CPU quota the host running ahead made the throttling
        # stalls of efgp_hip/cpu_quota.py appear there too, so the conservative choice stays the default).
        async_ok = prod(1 << (2 * n - 2).bit_length() for n in self.shape) <= 4096 or bool(os.environ.get("EFGP_ASYNC_UPLOAD_ALL"))
        up = _upload if async_ok else (lambda t, dv: t.to(dv))
        self.dprime = None
        self.ws = None
        self._weights_args = (kernel, want_grad, dev, up)
        if not defer_weights:
            self.make_weights()

    def make_weights(self):
        if self.ws is not None:
            return
        kernel, want_grad, dev, up = self._weights_args
        d = self.d
        # Built-in kernels: ws (and the hyper-derivatives) in ONE C call on the host (efgp_spectral_weights_host) instead of
        # meshgrid + stack + spectral_density + sqrt + casts, ~10 torch CPU ops whose dispatch (60-150 us per fit) the 0.3-ms
        # step had started to wait for; 3-D grids too (torch's own CPU ops go multi-threaded and slow above 32768 elements)
        native = self._native_weights(kernel, want_grad, dev)
        if native is not None:
            self.ws, self.dprime = native
            return
        # Small grids: evaluate the spectral density on the host (one upload instead of several launches).  Large
        # grids (3-D): on the device -- torch's CPU reductions switch to their threaded path above 32768 elements,
        # which costs tens of milliseconds per call on a many-core host (measured: 89 ms for M = 12167, d = 3).
        # The same host pathology hits torch.pow with a real exponent even on a few hundred elements (12 ms per call
        # measured on the 256-thread host): Matern densities always go to the device.
        host_ok = self.M * d <= 16384 and type(kernel).__name__ != "Matern"
        where = self.xis if host_ok else up(self.xis, dev)
        S = kernel.spectral_density(where).to(torch.float64)
        # The fused solvers treat every system of a model as coefficients of REAL functions (LABNOTES.md section 4.4), which
        # needs ws real and even on the symmetric grid -- true for the spectral density of any real stationary kernel.  The
        # built-in kernels (native path above) are even by construction; a user-supplied spectral_density is checked here, once
        # per grid, so that a broken one is a ValueError at the fit and not NaN coefficients from the kernel's refusal.
        Sf = S.reshape(-1)
        if not bool(torch.isfinite(Sf).all()) or bool((Sf < 0).any()) or \
                float((Sf - Sf.flip(0)).abs().max()) > 1e-12 * float(Sf.abs().max()):
            raise ValueError(f"{type(kernel).__name__}.spectral_density must be finite, non-negative and even (S(-xi) = S(xi)) on "
                             "the frequency grid: it is the spectral density of a real stationary kernel")
        self.ws = up(torch.sqrt(S.to(torch.complex128) * self.hprod), dev)       # (M,) complex, imag 0
        if want_grad:
            self.dprime = up((self.hprod * kernel.spectral_grad(where)).to(torch.complex128), dev)   # (M,H)

    @property
    def xis(self):
        if self._xis is None:
            mesh = torch.meshgrid(*self.xis_axes, indexing="ij")
            self._xis = torch.stack(mesh, dim=-1).view(-1, self.d)
        return self._xis

    def _native_weights(self, kernel, want_grad, dev):
        """(ws, dprime) as device tensors from ONE launch (efgp_spectral_weights) for the built-in kernels, else None."""
        if os.environ.get("EFGP_NO_NATIVE_GRID") or self.M > (1 << 24) or torch.device(dev).type != "cuda":
            return None
        if self.ard:
            # ws and the d + 1 derivative rows of an ARD kernel in one launch (efgp_spectral_weights_nd)
            if not 1 <= self.d <= 3:
                return None
            dev = torch.device(dev)
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            vals = kernel.get_hypers()
            return spectral_weights_nd(dev, kernel.ard_kind, kernel.nu, vals[:-1], vals[-1], self.hs, self.shape, want_grad=want_grad)
        bk = _builtin_kernel_constants(kernel)
        if bk is None:
            return None
        kc, ell, var = bk
        from efgp_hip.lib import lib
        dev = torch.device(dev)
        ws_d = torch.empty(self.M, dtype=torch.complex128, device=dev)
        dp_d = torch.empty((self.M, 2), dtype=torch.complex128, device=dev) if want_grad else None
        from efgp_hip.ops import _on, _stream
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        with _on(dev):
            rc = lib().efgp_spectral_weights(dev.index, kc[0], int(self.d),
                                             float(kc[1]), float(ell), float(var), float(kc[2]), float(self.h), int(self.mtot),
                                             ws_d.data_ptr(), dp_d.data_ptr() if want_grad else None, _stream(dev))
        return (ws_d, dp_d) if rc == 0 else None


def _builtin_kernel_constants(kernel):
    """((kind, nu, c0), lengthscale, variance) for the kernels efgp_spectral_weights evaluates itself, else None."""
    from utils.kernels import kernel_constants
    if tuple(getattr(kernel, "hypers", ())) != ("lengthscale", "variance") or not hasattr(kernel, "get_hypers"):
        return None
    try:
        ell, var = kernel.get_hypers()
        kc = kernel_constants(kernel, ell, var)
    except Exception:
        return None
    return None if kc is None else (kc, float(ell), float(var))


def _jacobi_diag(ws, v, sig):
    """The Jacobi diagonal v[0] |ws|^2 + sigma^2 (:128-133) from the launch every solve of a model takes it from
    (efgp_gradient_prepare): a diagonal that differs in the last bit sends a CG run that ends at its iteration cap (ill-conditioned
    D T D) to a visibly different iterate.  Callers that also need rhs = D F*y make their one `gradient_prepare` call themselves."""
    cidx = _center_flat(v)
    return gradient_prepare(ws, None, v.reshape(-1)[cidx:cidx + 1], sig, want_diag=True, want_rhs=False)[0]


def _variance_hyper(kernel, variance_idx):
    """Host value of the kernel's `variance` hyper-parameter; 1.0 for a kernel that has none (variance_idx None)."""
    if variance_idx is None:
        return 1.0
    if hasattr(kernel, "get_hypers"):
        return dict(zip(kernel.hypers, kernel.get_hypers()))["variance"]
    return float(kernel.get_hyper("variance"))


class _StageClock:
    """Host clock of a gradient step's stages, under the reference's stage names and their roctx ranges: `lap(name, ...)` ends the
    named stages.  sync (do_profiling): the device is synchronised at every stage boundary, which makes the times device-accurate
    and is not free."""

    __slots__ = ("dev", "sync", "stages", "_tic", "_ranges")          # a step laps ten times and is bound by host time

    def __init__(self, dev, sync):
        self.dev, self.sync, self.stages = dev, sync, {}
        self._tic = time.perf_counter()
        self._ranges = _StageRanges("efgpnd_gradient_batched", "0_book_keeping")

    def __call__(self, *names):
        stages, ranges = self.stages, self._ranges
        for name in names:
            if self.sync:
                torch.cuda.synchronize(self.dev)
            now = time.perf_counter()
            stages[name] = stages.get(name, 0.0) + (now - self._tic)
            self._tic = now
            if ranges.enabled:
                ranges.lap(name)

    def close(self):
        if self.sync:
            print("\n===== stage timings for efgpnd_gradient_batched (seconds) =====")
            for name, sec in self.stages.items():
                print(f"  {name:28s} {sec:.6f}")
        self._ranges.close()


class _TailResult(NamedTuple):
    """What steps 4-8 of a gradient step hand to `_gradient_finish`, whichever tail ran them."""
    out_vec: Optional[torch.Tensor]     # grad | term1 | term2 | y.alpha in ONE device vector (the next four are views of it), or None
    grad: torch.Tensor
    term1: torch.Tensor
    term2: torch.Tensor
    y_alpha: object                     # 0-dim device tensor or host float
    beta: torch.Tensor                  # the mean solve's solution: the next step's warm start
    mean_iters: object                  # iteration counts: they stay on the device until somebody reads them
    trace_iters: object
    n_rhs: int
    warm: bool

    @classmethod
    def of_vector(cls, out, nh, *rest):
        """From the output vector of efgp_gradient_assemble / efgp_gradient_step over nh = H + 1 parameters."""
        return cls(out, out[:nh], out[nh:2 * nh], out[2 * nh:3 * nh], out[3 * nh], *rest)


_NO_ONE_CALL_STEP = set()          # (device, d, mtot) whose solves are not single launches: efgp_gradient_step said so once


def _gradient_one_call(kernel, grid, xd, yd, points, sig, N, cg_tol, early_stopping, mean_cg_init, use_mean_pc, use_trace_pc, tight,
                       nufft_eps, T, trace_idx, variance_idx, probe_seed, y_norm_sq, dev):
    """The whole adjoint-estimator step in one library call (efgp_hip.gradient_step) when it applies: built-in kernel, one GPU,
    generated probes, a circulant grid whose solves are single launches.  Returns a `_TailResult` as `_gradient_tail_native` does,
    or None (nothing enqueued that matters) and the caller drives the entry points itself."""
    if grid.ard:                       # the one-call step evaluates the isotropic weights itself
        return None
    key = (dev.index, grid.d, grid.mtot)
    F = 1 << (2 * grid.mtot - 2).bit_length()
    if key in _NO_ONE_CALL_STEP or F ** grid.d > 4096 or os.environ.get("EFGP_NO_GRADIENT_STEP") or os.environ.get("EFGP_NO_NATIVE_GRID"):
        return None
    kc = _builtin_kernel_constants(kernel)
    if kc is None or variance_idx != 1 or trace_idx != [0] or T < 1:
        return None
    from efgp_hip.ops import gradient_step
    warm = mean_cg_init is not None and tuple(mean_cg_init.shape) == (grid.M,)
    # the same draws from torch's generator, in the same order, as the entry-by-entry sequence
    if probe_seed is None:
        probe_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    v_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    yy = float(y_norm_sq) if y_norm_sq is not None else float(vdot_real(yd, yd))
    res = gradient_step(xd, yd, points, h=grid.h, mtot=grid.mtot, kconst=kc[0], lengthscale=kc[1], variance=kc[2], sigmasq=sig,
                        tol_pair=tight, tol_probe=max(tight, float(nufft_eps)) if nufft_eps else tight, cg_tol=cg_tol,
                        early_stop=early_stopping, nprobes=T, probe_seed=probe_seed, v_seed=v_seed, use_mean_pc=use_mean_pc,
                        use_trace_pc=use_trace_pc, variance_idx=variance_idx, trace_idx=trace_idx,
                        beta0=mean_cg_init.detach() if warm else None, n_obs=N, yy=yy)
    if res is None:
        _NO_ONE_CALL_STEP.add(key)
        return None
    out, beta, mean_iters, trace_iters = res
    return _TailResult.of_vector(out, 3, beta, mean_iters, trace_iters, 2 * T, warm)


def _domain_length(xd: torch.Tensor, shards: PointShards) -> float:
    lo, hi = torch.aminmax(xd, dim=0)
    lo, hi = shards.minmax(lo, hi)
    return float((hi - lo).max())


def _domain_sides(xd: torch.Tensor, shards: PointShards):
    """Side of the bounding box per axis (the per-axis grids of the ARD kernels), from the same all-reduced min / max."""
    lo, hi = torch.aminmax(xd, dim=0)
    lo, hi = shards.minmax(lo, hi)
    return [float(v) for v in (hi - lo).tolist()]


def _box_L(sides, ard):
    """What a `_Grid` takes as L, from the sides of the bounding box: every side for the per-axis grid of an ARD kernel, the longest
    otherwise; a box without extent counts as 1."""
    def clamp(v):
        return v if v > 1e-9 else 1.0
    return [clamp(float(v)) for v in sides] if ard else clamp(max(sides))


def _points_box(xd, shards, ard):
    """`_box_L` of a model's points.  On a sharded model the longest side is all-reduced first and, for an ARD kernel, the sides
    after it: every rank goes through the same collectives in this order."""
    L = _box_L([_domain_length(xd, shards)], False)
    return _box_L(_domain_sides(xd, shards), True) if ard else L


def _kernel_by_name(name, dimension):
    """The built-in kernel a model's `kernel` string names (case-insensitive)."""
    from kernels.matern import Matern
    from kernels.squared_exponential import SquaredExponential
    key = name.lower()
    if key in ("squaredexponential", "se"):
        return SquaredExponential(dimension=dimension)
    if key in ("matern12", "matern32", "matern52"):
        return Matern(dimension=dimension, nu={"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[key])
    raise ValueError(f"Unknown kernel type: {name}")


def _normal_equations(plan: NufftPlan, yd, grid: _Grid, shards: PointShards):
    """(F*y (M,), Toeplitz vector v ((4m+1,)*d)) in one pass over the points, all-reduced over shards."""
    Fy, v = plan.type1_pair(yd, grid.shape, tuple(2 * n - 1 for n in grid.shape))      # 2 n - 1 = 4 m + 1 lags per axis
    shards.sum_many_([Fy, v])
    return Fy.reshape(-1), v


def _center_value(v: torch.Tensor) -> torch.Tensor:
    return v[tuple((s - 1) // 2 for s in v.shape)].real


def _center_flat(v: torch.Tensor) -> int:
    idx = 0
    for s in v.shape:
        idx = idx * s + (s - 1) // 2
    return idx


# ======================================================================================
# hyper-parameter gradient (reference: efgpnd.py:17-317)
# ======================================================================================
def efgpnd_gradient_batched(
        x, y, sigmasq, kernel, eps, trace_samples, x0=None, x1=None,
        *, nufft_eps=6e-8, cg_tol=None, early_stopping=True, device=None,
        do_profiling=False, compute_log_marginal=False,
        noise_floor: Optional[float] = None,
        stats_out: Optional[Dict[str, float]] = None,
        mean_cg_init: Optional[torch.Tensor] = None, mean_cg_init_shape=None,
        use_mean_cg_preconditioner: bool = True,
        use_trace_cg_preconditioner: bool = True,
        log_marginal_probes=100, log_marginal_steps=25,
        probes_Z: Optional[torch.Tensor] = None, probes_V: Optional[torch.Tensor] = None,
        shards: Optional[PointShards] = None, trace_mode: str = "adjoint", probe_seed: Optional[int] = None,
        domain_length: Optional[float] = None, y_norm_sq: Optional[float] = None, points: Optional[PointSet] = None,
        log_marginal_probe_vectors: Optional[torch.Tensor] = None, pointwise_alpha: bool = False, raster=None):
    """d(negative log marginal likelihood)/d(kernel hypers..., sigma^2) = (term1 - term2)/2 with
    Hutchinson trace estimates (data-space probes Z for non-variance kernel hypers, feature-space
    probes V for the noise) and CG solves.  ``x0, x1`` are ignored as in the reference (:72-73).

    Extra keyword arguments (not in the reference): ``probes_Z`` (T,N) / ``probes_V`` (T,M) inject the
    +-1 probes (the reference draws them from torch's generator at :179-182 and :199-202), and
    ``shards`` sums the gridded partials / N-length scalars over point shards; ``domain_length`` passes the box
    length max_a(max x_a - min x_a) when the caller already knows it (EFGPND caches it: the two N-length min/max
    reductions cost 6.6 ms per step at N = 5e6, d = 3); ``y_norm_sq`` likewise the global sum of y^2.  In the
    adjoint mode nothing is read back to the host before the gradient is complete (solves through the asynchronous
    entry points, scalars kept as 0-dim device tensors).
    Stage timers (seconds) are written to ``stats_out['stage_sec']`` with the reference's stage names (host
    clock; with ``do_profiling=True`` the device is synchronised at every stage boundary so they are exact).

    ``trace_mode``:
      * ``"adjoint"`` (default) evaluates every N-length inner product of the reference in feature space
        through the adjoint identity  sum_n z_n (F g)_n = <F* z, g>  and  |F g|^2 = <g, T g>:
        sum_n Z (rhs - F(ws beta))/sigma^2 = Re<F*Z, D'F*Z - ws beta>/sigma^2,  y.z = Re<F*y, g>,  |z|^2 = Re<g, T g>
        (g = ws beta, z = F g).  Same estimator, same probes, but NO type-2 pass over the N points (the
        reference spends 1 + 2T of them, :149, :189, :234) and, without injected probes, the +-1 draws are
        generated inside the spread kernel (``probe_seed``) so Z never exists in memory.  Agrees with the
        literal sequence to the NUFFT tolerance.
      * ``"reference"`` follows the reference's operation sequence literally (type-2 passes included).

    ``pointwise_alpha`` (adjoint mode only): the adjoint form obtains |y - F g|^2 as yy - 2 Re<F*y, g> + <g, T g>, i.e. by
    cancellation: the 6e-8 transform error is amplified by yy / |y - F g|^2 (the reference's pointwise alpha only by the
    square root of that).  For high-SNR data (sigma^2 << signal variance) set it to get alpha = (y - F g)/sigma^2 from ONE
    real type-2 pass and the two N-length reductions of the reference (:163, :170); everything else stays adjoint.

    ``raster`` (set by a gridded model, `EFGPND.from_grid`): ``(axes, mask, n_observed)`` -- the observations lie on the
    rectilinear raster axes[0] x .. x axes[d-1]; ``x`` is ignored, ``y`` holds the raster's values in row-major order, ``mask``
    (float64 0/1 of the raster's size, or None) its observed cells.  Every pass over the observations is then an exact
    `RasterPlan` transform; adjoint estimator only, ``domain_length`` required.
    """
    if trace_mode not in ("adjoint", "reference"):
        raise ValueError(f"trace_mode must be 'adjoint' or 'reference', got {trace_mode!r}")
    adjoint = trace_mode == "adjoint"
    if cg_tol is None:
        cg_tol = eps

    # 0) book keeping -------------------------------------------------------------------------
    out_device = device or x.device
    dev = compute_device(y if raster is not None else x, device=device)
    lap = _StageClock(dev, do_profiling)
    shards = shards or PointShards(enabled=False)
    yd = y.detach().to(device=dev, dtype=torch.float64).contiguous()
    if raster is not None:
        if not adjoint or pointwise_alpha:
            raise NotImplementedError("a gridded model (EFGPND.from_grid) supports the adjoint gradient estimator only: the literal "
                                      "and pointwise_alpha modes need a complex type-2 transform onto the raster")
        if shards.active or domain_length is None:
            raise NotImplementedError("a gridded model (EFGPND.from_grid) runs on one device and passes its domain_length")
        xd, yd = None, yd.reshape(-1)
        N_local, d = int(raster[2]), len(raster[0])
        N = N_local
    else:
        xd = _dev_points(x, dev)
        N_local, d = xd.shape
        N = int(shards.sum_scalars([N_local], dev)[0]) if shards.active else N_local
    if hasattr(kernel, "ard_kind"):
        L = _box_L(domain_length if domain_length is not None else _domain_sides(xd, shards), True)
    else:
        L = float(domain_length) if domain_length is not None else _domain_length(xd, shards)
    sig = float(sigmasq.detach()) if torch.is_tensor(sigmasq) else float(sigmasq)
    if noise_floor is not None:
        sig = max(sig, float(noise_floor))
    kernel_hypers = list(getattr(kernel, "hypers", []))
    variance_idx = kernel_hypers.index("variance") if "variance" in kernel_hypers else None
    kernel_hyper_count = kernel.num_hypers - 1
    trace_idx = [i for i in range(kernel_hyper_count) if i != variance_idx]
    T = int(trace_samples)
    echo = (T, bool(use_mean_cg_preconditioner), bool(use_trace_cg_preconditioner))          # what the statistics repeat
    lap("0_book_keeping")

    # 1) frequency grid -----------------------------------------------------------------------
    grid = _Grid(kernel, eps, L, d, dev, want_grad=True, defer_weights=True)
    if mean_cg_init_shape is not None and tuple(mean_cg_init_shape) != tuple(grid.shape):
        mean_cg_init = None                   # a start vector of another block with the same mode count is no warm start
    lap("1_frequency_grid_setup")

    # 2) NUFFT plan ---------------------------------------------------------------------------
    # The Toeplitz vector is always computed to 6e-8 (:1418) and F*y rides in that pass; the probe transforms only
    # need the caller's nufft_eps (:186-189), i.e. a narrower window: a second plan over the same points (W^d LDS
    # operations per point: 3-D, eps 1e-4 vs 6e-8 is 216 vs 512 per channel).
    tight = min(float(nufft_eps), _CONV_TOL) if nufft_eps else _CONV_TOL
    if points is not None and (raster is not None or points.x.data_ptr() != xd.data_ptr() or points.npts != N_local):
        points = None
    # Everything from here to the assembled gradient in ONE library call when the step is the common one (adjoint estimator, built-in
    # kernel, one GPU, generated probes, single-launch solves): the ~15 entry points cost more host time driven from Python than
    # their kernels take on the device (csrc/gradient_step.cpp).  Stage timers then carry the whole call under "4_solve_cg".
    res = None
    if (raster is None and adjoint and not pointwise_alpha and not shards.active and probes_Z is None and probes_V is None and not do_profiling
            and not compute_log_marginal and os.environ.get("EFGP_NO_FUSED_GRADIENT") is None and dev.type == "cuda"):
        res = _gradient_one_call(kernel, grid, xd, yd, points, sig, N, cg_tol, early_stopping, mean_cg_init,
                                 use_mean_cg_preconditioner, use_trace_cg_preconditioner, tight, nufft_eps, T, trace_idx, variance_idx,
                                 probe_seed, y_norm_sq, dev)
    if res is not None:
        lap("2_nufft_setup", "3_toeplitz_setup", "4_solve_cg", "5_compute_term2", "6_monte_carlo_trace", "7_batch_cg_solve",
            "7.5_compute_alpha", "8_gradient_calculation")
        return _gradient_finish(res, grid, lap, stats_out, echo, out_device, x.dtype)
    if raster is not None:               # exact transforms: one plan serves the pair and the probes
        plan = plan_p = RasterPlan(raster[0], grid.plan_h, cell_scale=raster[1], _scale_checked=True)
    else:
        plan = NufftPlan(xd, grid.plan_h, tight, points=points)
        plan_p = plan if (not nufft_eps or float(nufft_eps) <= tight) else NufftPlan(xd, grid.plan_h, float(nufft_eps), points=points)
    lap("2_nufft_setup")

    # 3) Toeplitz operator, Jacobi diagonal (F*y rides in the same pass over the points) --------
    Fy, v = _normal_equations(plan, yd, grid, shards)
    grid.make_weights()                      # behind the pass over the points: the device is busy while the host sets them up
    Dp = grid.dprime
    top = ToeplitzOp(v)
    # The M-scale tail in native launches when the estimator is the adjoint one: prepare | solve | T g | probes, two scaled
    # Toeplitz products | batched solve | assemble -- about 35 launches per step instead of 118 (the step was bound by the host
    # enqueueing 3 us torch kernels on 529-element vectors).  The literal / pointwise modes keep the torch sequence.
    native = (adjoint and not pointwise_alpha and kernel_hyper_count <= 4 and Dp is not None and Dp.ndim == 2
              and Dp.shape[1] == kernel_hyper_count and os.environ.get("EFGP_NO_FUSED_GRADIENT") is None)
    tail = _gradient_tail_native if native else partial(_gradient_tail_torch, adjoint=adjoint, pointwise_alpha=pointwise_alpha)
    res = tail(kernel, grid, top, Fy, v, sig, N, N_local, cg_tol, early_stopping, mean_cg_init, use_mean_cg_preconditioner,
               use_trace_cg_preconditioner, plan_p, shards, dev, T, trace_idx, variance_idx, probes_Z, probes_V, probe_seed, y_norm_sq,
               yd, lap)
    logdet = None
    if compute_log_marginal:
        logdet = partial(logdet_slq, grid.ws, sig, top, probes=log_marginal_probes, steps=log_marginal_steps, dtype=torch.float64,
                         device=dev, n=N, probe_vectors=log_marginal_probe_vectors)
    return _gradient_finish(res, grid, lap, stats_out, echo, out_device, x.dtype, N, logdet)


def _gradient_finish(res, grid, lap, stats_out, echo, out_device, rdtype, N=None, logdet=None):
    """Diagnostics, the optional log marginal likelihood and the returned gradient of a step whose tail returned `res`.  `echo`: the
    settings of the step that its statistics repeat (trace samples, mean and trace solves preconditioned); `logdet`: the call that
    gives log det(K + sigma^2 I) when the log marginal likelihood of the N observations is wanted, else None."""
    if stats_out is not None:
        stats_out.update({
            # iteration counts of the asynchronous solves stay on the device until somebody reads them (int(...), comparison,
            # formatting all do): two blocking device-to-host copies per step otherwise
            "mean_cg_iters": res.mean_iters,
            "trace_cg_iters": res.trace_iters,
            "trace_num_rhs": int(res.n_rhs),
            "feature_count": int(grid.M),
            **({} if grid.ard else {"mtot": grid.mtot}),
            "shape": tuple(grid.shape),
            "hs": tuple(grid.hs),
            "trace_samples": echo[0],
            "mean_cg_warm_start_used": bool(res.warm),
            "mean_cg_preconditioned": echo[1],
            "trace_cg_preconditioned": echo[2],
            "stage_sec": dict(lap.stages),
        })
        stats_out["mean_beta"] = res.beta.to(out_device)
        if res.out_vec is not None:
            # grad | term1 | term2 | y.alpha live in one device vector: ONE read-back serves the diagnostics and the caller's
            # host copy of the gradient (EFGPND.compute_gradients)
            nh = int(res.term1.numel())
            host_out = res.out_vec.cpu()
            stats_out["term1"] = host_out[nh:2 * nh].clone()
            stats_out["term2"] = host_out[2 * nh:3 * nh].clone()
            stats_out["grad_host"] = host_out[:nh].clone()
        else:
            stats_out["term1"] = res.term1.detach().cpu()
            stats_out["term2"] = res.term2.detach().cpu()
    log_marginal = None
    if logdet is not None:
        log_marginal = torch.tensor(-0.5 * float(res.y_alpha) - 0.5 * logdet() - 0.5 * N * math.log(TWO_PI), dtype=rdtype)
        lap("9_log_marginal_likelihood")
    lap.close()
    g_out = res.grad.to(device=out_device, dtype=rdtype)
    return g_out if logdet is None else (g_out, log_marginal)


def _gradient_tail_torch(kernel, grid, top, Fy, v, sig, N, N_local, cg_tol, early_stopping, mean_cg_init, use_mean_pc, use_trace_pc,
                         plan_p, shards, dev, T, trace_idx, variance_idx, probes_Z, probes_V, probe_seed, y_norm_sq, yd, lap, *,
                         adjoint, pointwise_alpha):
    """Steps 4-8 of efgpnd_gradient_batched as the reference's own sequence of torch operations: the tests' yardstick, and the only
    path of trace_mode="reference", of `pointwise_alpha`, and of kernels with more than four hyper-parameters or no `spectral_grad`
    matrix.  Arguments as `_gradient_tail_native`; the result carries no output vector."""
    ws, Dp, M = grid.ws, grid.dprime, grid.M
    num_hypers = kernel.num_hypers
    kernel_hyper_count = num_hypers - 1
    diag = _jacobi_diag(ws, v, sig)          # from the launch the native tail takes it from
    lap("3_toeplitz_setup")

    # 4) mean solve ---------------------------------------------------------------------------
    rhs = ws * Fy
    warm = mean_cg_init is not None and tuple(mean_cg_init.shape) == tuple(rhs.shape)
    b0 = mean_cg_init.detach().to(device=dev, dtype=torch.complex128) if warm else None          # None: the solver starts from zeros it allocates itself (no copy)
    # rhs = D F*y of the real y (and a warm start from an earlier solve of the same kind): coefficients of real functions
    beta, mean_iters = cg_solve_lazy(top, ws, sig, 0, rhs, b0, cg_tol, early_stop=early_stopping,
                                     diag=diag if use_mean_pc else None, batched=False, hermitian=True)
    mean_iters.settle()
    beta_raw = beta.clone()
    beta_s = ws * beta                                        # g = D beta
    Tg = top.apply(beta_s)
    if not adjoint:
        z = plan_p.type2(beta_s, grid.shape)                 # F g, complex (N,)
        alpha = (yd - z) / sig
    lap("4_solve_cg")

    # 5) term 2 -------------------------------------------------------------------------------
    fadj_alpha = (Fy - Tg) / sig                               # = F* alpha without another pass over N
    term2_kernel = torch.stack([vdot_m(fadj_alpha, Dp[:, i] * fadj_alpha) for i in range(kernel_hyper_count)]) \
        if kernel_hyper_count else torch.zeros(0, dtype=torch.float64, device=dev)
    if adjoint:
        yy = float(y_norm_sq) if y_norm_sq is not None else shards.sum_scalars([vdot_real(yd, yd)], dev)[0]
        y_z = vdot_m(Fy, beta_s)                               # Re sum_n y_n z_n          (0-dim device tensors:
        z_z = vdot_m(beta_s, Tg)                               # |F g|^2 = <g, T g>         no host round trip)
        if pointwise_alpha:
            zr = plan_p.type2(beta_s, grid.shape, real_only=True)          # Re F g at the N points: one real gather
            alpha_r = (yd - zr) / sig
            a_norm, y_alpha = shards.sum_scalars([vdot_real(alpha_r, alpha_r), vdot_real(yd, alpha_r)], dev)
        else:
            a_norm = (yy - 2.0 * y_z + z_z) / (sig * sig)
            y_alpha = (yy - y_z) / sig
    else:
        a_norm, y_alpha = shards.sum_scalars([vdot_real(alpha, alpha), vdot_real(yd, alpha)], dev)
    variance = _variance_hyper(kernel, variance_idx)
    if variance_idx is not None:
        term2_kernel[variance_idx] = (y_alpha - sig * a_norm) / variance
    term2 = torch.cat((term2_kernel, torch.as_tensor(a_norm, dtype=torch.float64, device=dev).reshape(1)))
    lap("5_compute_term2")

    # 6) Monte-Carlo trace probes ---------------------------------------------------------------
    K = len(trace_idx)
    Z = None
    rhs_k = None
    if K > 0:
        if probes_Z is not None:
            Z = probes_Z.detach().to(device=dev, dtype=torch.float64).contiguous()
            FZ = plan_p.type1(Z, grid.shape).reshape(T, M)                            # real rows, two per pass
        elif adjoint:
            if probe_seed is None:
                probe_seed = shards.shared_seed(dev)              # one draw on rank 0: all shards use one Z stream
            offset = shards.exclusive_offset(N_local, dev)
            FZ = plan_p.type1_rademacher(probe_seed, T, grid.shape, index_offset=offset).reshape(T, M)
        elif shards.active:
            # sharded literal mode: Z[t, n] from (seed, t, GLOBAL index n) so the shards hold slices of one global
            # probe matrix (per-rank torch generators would repeat or decorrelate blocks depending on their seeds)
            if probe_seed is None:
                probe_seed = shards.shared_seed(dev)
            Z = rademacher_fill(dev, probe_seed, T, N_local, index_offset=shards.exclusive_offset(N_local, dev))
            FZ = plan_p.type1(Z, grid.shape).reshape(T, M)
        else:
            Z = torch.empty((T, N_local), device=dev, dtype=torch.float64).bernoulli_(0.5).mul_(2).sub_(1)
            FZ = plan_p.type1(Z, grid.shape).reshape(T, M)
        shards.sum_(FZ)
        DFZ = torch.stack([Dp[:, i] * FZ for i in trace_idx], dim=0).reshape(K * T, M)
        if not adjoint:
            rhs_k = plan_p.type2(DFZ, grid.shape, batched=True)                       # (K*T, N) complex
        B_k = ws * top.apply(DFZ)
    else:
        DFZ = torch.empty((0, M), dtype=torch.complex128, device=dev)
        B_k = torch.empty((0, M), dtype=torch.complex128, device=dev)
    if probes_V is not None:
        V = probes_V.detach().to(device=dev, dtype=torch.float64).contiguous()
    else:
        V = torch.empty((T, M), device=dev, dtype=torch.float64).bernoulli_(0.5).mul_(2).sub_(1)
        shards.broadcast_(V)                                      # replicated solves need ONE draw (rank 0's)
    Vc = V.to(torch.complex128)
    B_n = ws * top.apply(ws * Vc)
    B_all = torch.cat((B_k, B_n), dim=0)
    lap("6_monte_carlo_trace")

    # 7) batched CG -----------------------------------------------------------------------------
    Beta_all, trace_iters = _solve_batched(shards, top, ws, sig, 0, B_all, cg_tol, early_stop=early_stopping,
                                           diag=diag if use_trace_pc else None)
    lap("7_batch_cg_solve")

    # 7.5) term 1 -------------------------------------------------------------------------------
    term1 = torch.empty(num_hypers, dtype=torch.float64, device=dev)
    Beta_k, Beta_n = Beta_all[:K * T], Beta_all[K * T:]
    if K > 0:
        if adjoint:
            # sum_n Z (F(D'F*Z) - F(ws beta))/sigma^2 = Re <F*Z, D'F*Z - ws beta> / sigma^2   (F*Z is already global)
            diff = (DFZ - ws * Beta_k).reshape(K, T, M)
            sums = [(FZ.conj() * diff[slot]).sum().real / sig for slot in range(K)]
        else:
            fwdB = plan_p.type2(ws * Beta_k, grid.shape, batched=True)
            Alpha = (rhs_k - fwdB) / sig                                            # (K*T, N)
            sums = [vdot_real(Z, Alpha[s_ * T:(s_ + 1) * T]) for s_ in range(K)]    # sum_t sum_n Z*Alpha
            sums = shards.sum_scalars(sums, dev)
        for slot, ki in enumerate(trace_idx):
            term1[ki] = sums[slot] / T
    t1_noise = N / sig - ((Vc.conj() * Beta_n).sum(dim=1).real / sig).mean()
    if variance_idx is not None:
        term1[variance_idx] = (N - sig * t1_noise) / variance
    term1[-1] = t1_noise
    lap("7.5_compute_alpha")

    grad = 0.5 * (term1 - term2)
    lap("8_gradient_calculation")

    return _TailResult(None, grad, term1, term2, y_alpha, beta_raw, mean_iters, trace_iters, int(B_all.shape[0]), warm)


def _gradient_tail_native(kernel, grid, top, Fy, v, sig, N, N_local, cg_tol, early_stopping, mean_cg_init, use_mean_pc, use_trace_pc,
                          plan_p, shards, dev, T, trace_idx, variance_idx, probes_Z, probes_V, probe_seed, y_norm_sq, yd, lap):
    """Steps 4-8 of efgpnd_gradient_batched (adjoint estimator) in native launches; same quantities, same stage names.
    Returns a `_TailResult` whose output vector is grad | term1 | term2 | y.alpha of efgp_gradient_assemble."""
    ws, Dp, M = grid.ws, grid.dprime, grid.M
    lap("3_toeplitz_setup")
    # 4) mean solve (reference :128-153): Jacobi diagonal and rhs = D F*y in one launch, solve, T g
    cidx = _center_flat(v)
    diag, rhs = gradient_prepare(ws, Fy, v.reshape(-1)[cidx:cidx + 1], sig, want_diag=use_mean_pc or use_trace_pc)
    warm = mean_cg_init is not None and tuple(mean_cg_init.shape) == tuple(rhs.shape)
    b0 = mean_cg_init.detach().to(device=dev, dtype=torch.complex128) if warm else None
    beta, mean_iters = cg_solve_lazy(top, ws, sig, 0, rhs, b0, cg_tol, early_stop=early_stopping,
                                     diag=diag if use_mean_pc else None, batched=False, hermitian=True)
    Tg = top.apply_scaled(beta, pre=ws)                         # T (D beta)
    lap("4_solve_cg")
    lap("5_compute_term2")                                      # term 2 is part of the assemble launch below

    # 6, 7) probes, the right-hand sides of the trace systems and their batched solve
    FZ, V, Beta_all, trace_iters = _trace_systems(grid, top, plan_p, sig, cg_tol, early_stopping, diag if use_trace_pc else None, T,
                                                  trace_idx, shards, N_local, dev, probes_Z, probes_V, probe_seed, lap)
    # the mean solve is settled only here, where the batched solve has made the host wait already; a re-solved beta needs T g again
    if mean_iters.settle():
        Tg = top.apply_scaled(beta, pre=ws)
    lap("7_batch_cg_solve")

    # 7.5 / 8) every inner product of terms 1 and 2 and the final algebra: two launches, nothing read back
    yy = float(y_norm_sq) if y_norm_sq is not None else float(shards.sum_scalars([vdot_real(yd, yd)], dev)[0])
    out = gradient_assemble(Fy, Tg, ws, beta, Dp, FZ, V, Beta_all.reshape(-1, M), variance_idx=variance_idx, trace_idx=trace_idx,
                            sigmasq=sig, n_obs=N, yy=yy, variance=_variance_hyper(kernel, variance_idx))
    lap("7.5_compute_alpha", "8_gradient_calculation")
    return _TailResult.of_vector(out, Dp.shape[1] + 1, beta, mean_iters, trace_iters, Beta_all.shape[0], warm)


def _trace_systems(grid, top, plan_p, sig, cg_tol, early_stopping, diag, T, trace_idx, shards, N_local, dev, probes_Z=None,
                   probes_V=None, probe_seed=None, lap=None):
    """The trace block of the adjoint estimator, which depends on the points and the hyper-parameters only: T data-space probes Z
    through F* (for the traced hypers `trace_idx`), T feature-space probes V (for the noise), the (len(trace_idx) + 1) T
    right-hand sides and their batched solve from zero -> (F*Z (T, M) or None, V (T, M), solutions ((K + 1) T, M), iteration
    counts).  Draws from torch's generator, in this order: the seed of Z, only when none was given and a hyper is traced; then
    the seed of V (its T x M entries on a sharded model).  `lap` ends stage 6 between the right-hand sides and the solve."""
    ws, Dp, M, K = grid.ws, grid.dprime, grid.M, len(trace_idx)
    # 6) probes and the right-hand sides of the trace systems (reference :179-203)
    B_all = torch.empty(((K + 1) * T, M), dtype=torch.complex128, device=dev)
    FZ = None
    if K > 0:
        if probes_Z is not None:
            Z = probes_Z.detach().to(device=dev, dtype=torch.float64).contiguous()
            FZ = plan_p.type1(Z, grid.shape).reshape(T, M)
        else:
            if probe_seed is None:
                probe_seed = shards.shared_seed(dev)            # one draw on rank 0: all shards use one Z stream
            FZ = plan_p.type1_rademacher(probe_seed, T, grid.shape, index_offset=shards.exclusive_offset(N_local, dev)).reshape(T, M)
        shards.sum_(FZ)
        for slot, ki in enumerate(trace_idx):                   # D ws-scaled T (D'_i F*Z): D'_i rides in the pad, ws in the crop
            top.apply_scaled(FZ, pre=Dp[:, ki].contiguous(), post=ws, out=B_all[slot * T:(slot + 1) * T])
    if probes_V is not None:
        V = probes_V.detach().to(device=dev, dtype=torch.float64).contiguous()
    elif shards.active:
        V = torch.empty((T, M), device=dev, dtype=torch.float64).bernoulli_(0.5).mul_(2).sub_(1)
        shards.broadcast_(V)                                    # replicated solves need ONE draw (rank 0's)
    else:
        V = rademacher_fill(dev, int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()), T, M)
    top.apply_scaled(V, pre=ws, post=ws, out=B_all[K * T:])
    if lap is not None:
        lap("6_monte_carlo_trace")
    # 7) batched CG from zero (reference :205-236)
    Beta_all, trace_iters = _solve_batched(shards, top, ws, sig, 0, B_all, cg_tol, early_stop=early_stopping, diag=diag)
    return FZ, V, Beta_all, trace_iters


def _rows_over_ranks(shards, top, R):
    """Should the R independent systems of a batched solve be split over the ranks?  On the 64 x 64 grid every system is ONE
    workgroup on one CU and up to num_CU of them run side by side on a GPU: splitting pays from more rows than CUs on.  Larger
    grids take many CUs per system (cooperative launch, multi-kernel 3-D iteration) and go through the rows in slabs:
    splitting pays as soon as every rank gets a row.  opts / env EFGP_SHARD_ROWS=0 keeps every solve replicated."""
    if shards is None or not shards.active or R < shards.world_size:
        return False
    if os.environ.get("EFGP_SHARD_ROWS", "1") == "0":
        split = False
    elif top.one_workgroup_per_system:
        split = R > torch.cuda.get_device_properties(top.dev).multi_processor_count
    else:
        split = True
    # the decision selects the collectives that follow: it must be identical on all ranks (checked once per shape)
    return shards.agree(("rows_over_ranks", top.fft_cells, R), split, top.dev)


def _solve_batched(shards, top, ws, sig, variant, B_all, tol, *, early_stop, diag, max_iter=None, hermitian=False):
    """The batched solves of the gradient and of the variance: asynchronous persistent / cooperative kernels where the grid
    allows, the multi-launch solver otherwise; rows split over the ranks when that pays (`_rows_over_ranks`).  Returns
    (X (R, M), iteration count: int-like)."""
    from efgp_hip.ops import LazyIterations
    from efgp_hip.dist import solve_rows_sharded

    def solve(block):
        x, its = cg_solve_lazy(top, ws, sig, variant, block, None, tol, max_iter=max_iter, early_stop=early_stop, diag=diag,
                               batched=True, hermitian=hermitian)
        its.settle()           # nobody downstream reads the counts before using the solutions (diag_sums_nd, the assemble launch)
        return x, its.rows_tensor

    R = B_all.shape[0]
    if _rows_over_ranks(shards, top, R):
        X, rows = solve_rows_sharded(shards, B_all.reshape(R, -1), solve)
        X = X.reshape(B_all.shape)
    else:
        X, rows = solve(B_all)
    return X, LazyIterations(rows, True, int(max_iter) if max_iter is not None else 2 * top.size)


def vdot_m(a, b):
    """Re<a,b> for M-length device vectors, kept on the device (glue on tiny vectors)."""
    return (a.conj() * b).sum().real


# ======================================================================================
# variance helpers (reference: efgpnd.py:1634-1679, 1761-1841) and SLQ log-det (:1686-1759)
# ======================================================================================
def _unwrap_operator(A_apply):
    if isinstance(A_apply, _FeatureOperator) and A_apply._efgp_fusable:
        return A_apply
    raise TypeError("expected an operator made by create_A_mean / create_A_var")


def _hutchinson_solves(A_apply, J, xis_flat, max_cg_iter, cg_tol, ws, probes, shards, shape):
    """The probes of the stochastic variance and their solves u_j = A^-1 (ws eta_j), which depend on the hyper-parameters only: what
    `diag_sums_nd` and `diag_sums_gradient_nd` share.  -> (ws on the device, us (J, M), etas (J, M), mode count(s), d)."""
    if shape is not None:
        m_loc, d_loc, Mtot = tuple(int(n) for n in shape), len(shape), prod(shape)
    else:
        Mtot, d_loc = xis_flat.shape
        m_loc = round(Mtot ** (1 / d_loc))
        assert m_loc ** d_loc == Mtot, "xis must lie on tensor grid"
    op = _unwrap_operator(A_apply)
    dev = op.toeplitz._dev
    if probes is None:
        etas = (torch.randint(0, 2, (J, Mtot), device=dev) * 2 - 1).to(torch.float64)
    else:
        etas = probes.detach().to(device=dev, dtype=torch.float64)
    wsd = ws.to(device=dev, dtype=torch.complex128)
    rhs = wsd[None, :] * etas
    us, _ = _solve_batched(shards, op.toeplitz._op, wsd, op.sigmasq, op.variant, rhs, cg_tol, early_stop=True, diag=None,
                           max_iter=max_cg_iter)
    return wsd, us, etas, m_loc, d_loc


def diag_sums_nd(A_apply, J, xis_flat, max_cg_iter, cg_tol, ws, probes: Optional[torch.Tensor] = None, shards=None, shape=None):
    """Hutchinson estimate of the lag sums c[r] = sum_{k-l=r} (A^-1)_{kl}-weighted products used by the
    stochastic variance (reference: efgpnd.py:1634-1664).  ``probes`` (J,M) of +-1 may be injected;
    otherwise they are drawn with torch.randint as in the reference (:1644).  ``shards`` (a PointShards of a multi-GPU
    model; the probes must then be identical on all ranks): the J systems are split by rows over the ranks.  ``shape``: the mode
    count per axis of a per-axis grid (then ``xis_flat`` is not looked at); the lag box is (2 n_a - 1) per axis."""
    wsd, us, etas, m_loc, d_loc = _hutchinson_solves(A_apply, J, xis_flat, max_cg_iter, cg_tol, ws, probes, shards, shape)
    # zero-padded correlation of every probe pair and the mean over probes (:1660-1664): hipFFT + three small kernels
    return lag_sums(wsd[None, :] * us, etas, m_loc, d_loc)


def diag_sums_gradient_nd(A_apply, J, xis_flat, max_cg_iter, cg_tol, ws, xi_axes, probes: Optional[torch.Tensor] = None, shards=None,
                          shape=None):
    """The lag sums of the variance of every partial derivative, from the solves of `diag_sums_nd` (same probe handling): with
    C = D A^-1 D, Var[d_a f(x)] = sum_kl (2 pi)^2 xi_ka xi_la f_k(x) C_kl conj f_l(x), so axis a takes the frequency-weighted sums
    2 pi lag_sums((2 pi xi_a) ws u, xi_a eta).  xi_axes: d device vectors (M,), xi_a of every mode.  -> list of d lag boxes."""
    wsd, us, etas, m_loc, d_loc = _hutchinson_solves(A_apply, J, xis_flat, max_cg_iter, cg_tol, ws, probes, shards, shape)
    g = wsd[None, :] * us
    return [TWO_PI * lag_sums((TWO_PI * xi)[None, :] * g, xi[None, :] * etas, m_loc, d_loc) for xi in xi_axes]


def nufft_var_est_nd(est_sums, h_val, x_center, pts, eps_val):
    """s^2(x*) = Re sum_r c[r] exp(2 pi i h r.x*), lags in FFT order (reference: efgpnd.py:1666-1679)."""
    B_loc, d_loc = pts.shape
    if est_sums.ndim != d_loc:
        raise ValueError("est_sums wrong dimensionality")
    op = NUFFT(pts, x_center, h_val, eps=eps_val)
    out = op._type2_dev(est_sums.detach(), tuple(est_sums.shape), modeord=1, real_only=True, batched=False)
    return out.to(device=pts.device, dtype=pts.dtype)


@torch.no_grad()
def logdet_slq(ws, sigma2, toeplitz, *, probes=1000, steps=100, dtype=torch.float64, device="cpu", eps=1e-18, n=None,
               probe_vectors: Optional[torch.Tensor] = None):
    """Stochastic Lanczos quadrature estimate of log det(sigma^2 I + D T D) restricted to feature space,
    i.e. log det(I + D T D / sigma^2) + n log sigma^2 (reference: efgpnd.py:1686-1759).

    All probes run their Lanczos recurrences inside ONE launch (`efgp_lanczos`: one workgroup per probe, alpha / beta
    stay on the device); grids beyond the single-launch kernel run the same recurrence for all probes at once as batched
    device operations.  Either way nothing is read back before the tridiagonal eigen-problems (one batched `eigh` of
    (probes, steps, steps) at the end): the reference's loop structure costs two host reads per Lanczos step.
    ``probe_vectors`` (probes, M) of +-1 may be injected; otherwise they are drawn as the reference does (:1716-1717)."""
    if n is None:
        raise ValueError("logdet_slq needs n (number of observations)")
    top = toeplitz._op if isinstance(toeplitz, ToeplitzND) else toeplitz
    dev = top.dev
    w = ws.real.to(device=dev, dtype=torch.float64)
    wc = w.to(torch.complex128)
    m = w.numel()
    s2 = float(sigma2)
    if probe_vectors is None:
        zs = torch.empty((int(probes), m), dtype=torch.float64, device=dev).bernoulli_(0.5).mul_(2).sub_(1)
    else:
        zs = probe_vectors.detach().to(device=dev, dtype=torch.float64).reshape(-1, m)
    P, K = zs.shape[0], int(steps)
    res = lanczos(top, wc, s2, 1, zs, K)
    if res is not None:
        alphas, betas, norm2, taken = res
        k_idx = torch.arange(K, device=dev)[None, :]
        live = k_idx < taken[:, None]                               # steps actually taken per probe
    else:
        q = (zs / zs.norm(dim=1, keepdim=True)).to(torch.complex128)
        norm2 = (zs * zs).sum(dim=1)
        q_prev = torch.zeros_like(q)
        beta_prev = torch.zeros(P, dtype=torch.float64, device=dev)
        alive = torch.ones(P, dtype=torch.bool, device=dev)
        a_list, b_list, l_list = [], [], []
        for _ in range(K):
            vv = q + (wc * top.apply(wc * q)) / s2 - beta_prev[:, None] * q_prev
            a = (q.conj() * vv).sum(dim=1).real
            vv = vv - a[:, None] * q
            b = vv.norm(dim=1)
            a_list.append(a)
            b_list.append(b)
            l_list.append(alive)
            nxt = alive & (b >= 1e-12)                               # the reference breaks after recording this step (:1733)
            safe = torch.where(nxt, b, torch.ones_like(b))
            q_prev = torch.where(nxt[:, None], q, q_prev)
            q = torch.where(nxt[:, None], vv / safe[:, None], q)
            beta_prev = torch.where(nxt, b, beta_prev)
            alive = nxt
        alphas, betas, live = torch.stack(a_list, 1), torch.stack(b_list, 1), torch.stack(l_list, 1)
    # tridiagonal matrices, padded with decoupled unit diagonal entries behind the steps taken (log 1 = 0, zero weight)
    alphas = torch.where(live, alphas, torch.ones_like(alphas))
    off = torch.where(live[:, 1:], betas[:, :-1], torch.zeros_like(betas[:, :-1]))      # beta_i couples steps i and i+1
    Tm = torch.diag_embed(alphas) + torch.diag_embed(off, offset=1) + torch.diag_embed(off, offset=-1)
    evals, evecs = torch.linalg.eigh(Tm.cpu())                       # (P, K, K) tiny: one transfer, LAPACK on the host
    evals = evals.clamp_min(eps)
    quad = ((evecs[:, 0, :] ** 2) * torch.log(evals)).sum(dim=1) * norm2.cpu()
    return float(quad.sum() / P) + n * math.log(s2)


def compute_prediction_variance(x_new, xis, ws, A_var, cg_tol, max_cg_iter, variance_method, h, xcen,
                                hutchinson_probes, nufft_eps, device, rdtype, cdtype, probes=None, shards=None, shape=None):
    """Latent posterior variance at x_new: 'regular' (one CG solve per point, microbatched) or
    'stochastic' (Hutchinson lag sums + FFT-ordered type-2).  Reference: efgpnd.py:1761-1841.
    ``shape`` with ``h`` a sequence: the per-axis grid of an ARD kernel (mode count and spacing per axis)."""
    method = variance_method.lower()
    if method == "regular":
        op = _unwrap_operator(A_var)
        dev = op.toeplitz._dev
        wsd = ws.to(device=dev, dtype=torch.complex128)
        xn = x_new.to(device=dev, dtype=torch.float64)
        M_loc = wsd.numel()
        if shape is not None:
            mtot_loc, hval = tuple(int(n) for n in shape), tuple(float(v) for v in h)
            assert prod(mtot_loc) == M_loc, "ws must lie on the per-axis grid"
        else:
            mtot_loc = round(M_loc ** (1.0 / xn.shape[1]))
            assert mtot_loc ** xn.shape[1] == M_loc, "ws must lie on the tensor grid"
            hval = float(h)
        out = []
        for xb in torch.split(xn, 8192, dim=0):
            rhs = variance_rhs(xb, hval, mtot_loc, wsd)                  # ws * conj(f(x*)): explicit feature rows (b, M)
            gamma, _, _ = cg_solve(op.toeplitz._op, wsd, op.sigmasq, op.variant, rhs, None, cg_tol,
                                   max_iter=max_cg_iter, early_stop=True, diag=None, batched=True,
                                   hermitian=True)     # feature rows of real points: conjugate-even
            out.append(variance_contract(xb, hval, mtot_loc, wsd, gamma))
        return torch.cat(out, dim=0).to(device=device, dtype=rdtype)
    if method == "stochastic":
        t1 = time.time()
        est = diag_sums_nd(A_var, hutchinson_probes, xis, max_cg_iter, cg_tol, ws, probes=probes, shards=shards, shape=shape)
        print(f"Time to compute diag sums: {time.time() - t1:.4f} seconds")
        return nufft_var_est_nd(est, h, xcen, x_new, nufft_eps).to(device=device, dtype=rdtype)
    raise ValueError(f"Variance method '{variance_method}' not implemented. Choose 'regular' or 'stochastic'.")


def gradient_variance_regular(x_new, xi_axes, ws, A_var, cg_tol, max_cg_iter, h, shape=None):
    """'regular' variance of the d partial derivatives of the latent function at x_new -> (B, d) float64 on the compute device.
    The feature row of the partial along axis a is 2 pi i xi_a f(x*): per block of 8192 points the right-hand sides of the value
    (`variance_rhs`: ws conj f) are multiplied by -2 pi i xi_a -- they stay conjugate-even -- and solved by the Hermitian batched
    CG; Var = max(0, Re sum_k conj(rhs_k) gamma_k), the contraction of `variance_contract` with the derivative row.
    xi_axes: d device vectors (M,); ``shape`` with ``h`` a sequence: a per-axis grid, as in `compute_prediction_variance`."""
    op = _unwrap_operator(A_var)
    dev = op.toeplitz._dev
    wsd = ws.to(device=dev, dtype=torch.complex128)
    xn = x_new.to(device=dev, dtype=torch.float64)
    M_loc = wsd.numel()
    if shape is not None:
        mtot_loc, hval = tuple(int(n) for n in shape), tuple(float(v) for v in h)
        assert prod(mtot_loc) == M_loc, "ws must lie on the per-axis grid"
    else:
        mtot_loc = round(M_loc ** (1.0 / xn.shape[1]))
        assert mtot_loc ** xn.shape[1] == M_loc, "ws must lie on the tensor grid"
        hval = float(h)
    factors = [torch.complex(torch.zeros_like(xi), -TWO_PI * xi) for xi in xi_axes]
    out = []
    for xb in torch.split(xn, 8192, dim=0):
        rhs = variance_rhs(xb, hval, mtot_loc, wsd)
        cols = []
        for fac in factors:
            ra = rhs * fac[None, :]
            gamma, _, _ = cg_solve(op.toeplitz._op, wsd, op.sigmasq, op.variant, ra, None, cg_tol, max_iter=max_cg_iter,
                                   early_stop=True, diag=None, batched=True, hermitian=True)
            cols.append((ra.conj() * gamma.reshape(ra.shape)).sum(dim=1).real.clamp_min(0.0))
        out.append(torch.stack(cols, dim=1))
    return torch.cat(out, dim=0)


def _raster_cell_blocks(ax, n_axis, dev, block=8192):
    """The coordinates of the raster's cells in row-major order, `block` cells at a time: no (prod n, d) tensor."""
    cells = prod(n_axis)
    for lo in range(0, cells, block):
        idx = torch.arange(lo, min(cells, lo + block), device=dev)
        cols = []
        for a in reversed(range(len(ax))):
            cols.append(ax[a][idx % n_axis[a]])
            idx = idx // n_axis[a]
        yield torch.stack(cols[::-1], dim=1)


# ======================================================================================
# the model (reference: efgpnd.py:336-1226)
# ======================================================================================
# Rows per batched pass of EFGPND.sample_paths (even: normals come in pairs).  A pass holds one complex fine grid and one int64
# accumulator pair per TWO rows plus the CG vectors of every row: 64 rows keep that below ~100 MB on the 2-D grids (up to
# 512 x 512 fine cells) and fill the batched CG; the 3-D fine grids (128^3 and beyond) are 100x larger per row.
# The table is efgp_hip.ops._SAMPLE_BLOCK = {1: 64, 2: 64, 3: 8} (imported above): NufftPlan.type2_jet feeds its rows by it too.


def _derive_seed(seed: int, stream: int) -> int:
    """Seed of noise stream `stream` of a draw: the splitmix64 finaliser of (seed, stream) -- e1 and e2 never share a counter."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(stream) + 1)) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return z ^ (z >> 31)


def _check_axes(axes, d_model, what):
    """The d_model coordinate vectors of a rectilinear raster as float64 tensors (where the caller has them); ValueError for a
    wrong count, an axis that is not 1-D or is empty, and non-finite coordinates."""
    if axes is None:
        raise ValueError(f"axes must be provided for {what}")
    if torch.is_tensor(axes) or isinstance(axes, np.ndarray):
        axes = [axes] if (d_model == 1 and axes.ndim == 1) else list(axes)
    axes = [torch.as_tensor(a).to(torch.float64) for a in axes]
    if len(axes) != d_model:
        raise ValueError(f"{what}: {len(axes)} axes given, the model was built on {d_model} dimensions")
    for a, ax in enumerate(axes):
        if ax.ndim != 1:
            raise ValueError(f"{what}: axes[{a}] must be 1-D (got shape {tuple(ax.shape)})")
        if ax.numel() == 0:
            raise ValueError(f"{what}: axes[{a}] is empty")
    fin = [torch.isfinite(ax).all() for ax in axes]
    for a, ok in enumerate(torch.stack([f.to(fin[0].device) for f in fin]).tolist()):       # one read-back for all axes
        if not ok:
            raise ValueError(f"{what}: axes[{a}] has non-finite coordinates")
    return axes


class EFGPND(nn.Module):
    """Equispaced-Fourier GP regression in d dimensions.

    ``EFGPND(x, y, kernel, sigmasq=None, eps=1e-2, nufft_eps=1e-4, opts=None, estimate_params=True)``
    with ``kernel`` a kernel object or one of "SquaredExponential"/"SE"/"Matern12"/"Matern32"/"Matern52"
    (case-insensitive).  Recognised ``opts``: cg_tolerance (1e-4), max_cg_iterations (1000),
    mean_cg_preconditioner (True), trace_cg_preconditioner (True), mean_cg_warm_start (True),
    noise_floor, log_marginal_probes (100), log_marginal_steps (25); additionally
    ``shard_points`` (bool): x, y hold THIS rank's block of the observations and gridded partial
    sums are all-reduced over the default process group (one process per GPU); ``point_layout``
    ("auto" | True | False): when the model builds its sorted point layout (see ``_layout``).
    """

    def __init__(self, x, y, kernel, sigmasq: float = None, eps: float = 1e-2, nufft_eps: float = 1e-4,
                 opts: Optional[Dict] = None, estimate_params: bool = True):
        super().__init__()
        self.x = x
        self.y = y
        self.device = x.device
        self.eps = eps
        self.nufft_eps = nufft_eps
        self.opts = {} if opts is None else opts.copy()
        dimension = 1 if x.ndim == 1 else x.shape[1]

        if isinstance(kernel, str):
            kernel = _kernel_by_name(kernel, dimension)
        self.kernel = kernel

        if estimate_params:
            try:
                ls, var, noise = kernel.estimate_hyperparameters(x, y)
                if hasattr(kernel, "set_hyper"):
                    kernel.set_hyper("lengthscale", ls)
                    kernel.set_hyper("variance", var)
                else:
                    print(f"Warning: Could not set hyperparameters on kernel of type {type(kernel)}")
                if sigmasq is None:
                    sigmasq = noise
            except Exception as e:   # same forgiving behaviour as the reference (:437-441)
                print(f"Warning: Failed to estimate hyperparameters: {e}")
                if sigmasq is None:
                    sigmasq = 0.1

        # hyper-parameters live in log space in the data's dtype (reference :444-457)
        prev = torch.get_default_dtype()
        try:
            torch.set_default_dtype(x.dtype)
            self._gp_params = GPParams(kernel=kernel, init_sig2=(sigmasq or 0.1))
            self.register_parameter("gp_params", self._gp_params.raw)
            if hasattr(self.kernel, "_gp_params_ref") and self.kernel._gp_params_ref is None:
                self.kernel._gp_params_ref = self._gp_params
        finally:
            torch.set_default_dtype(prev)

        self._beta = None
        self._xis = None
        self._ws = None
        self._toeplitz = None
        self._fitted = False
        self._cached_params = {}
        self._registered_optimizers = []
        self._last_gradient_stats = {}
        self._last_gradient_beta = None
        self._last_fit_stats = {}
        self._devdata = None
        self._fit_state = None
        self._predict_plan = None
        self._sample_plan = None
        self._last_sample_stats = {}
        self._nan_scalar = None
        self._raster = None                      # set by from_grid: the observations lie on a rectilinear raster
        # shard_points: True = torch.distributed default group; an efgp_hip.RcclComm = the library's own RCCL communicator
        sp = self.opts.get("shard_points", False)
        self._shards = PointShards(comm=sp) if (sp is not None and not isinstance(sp, bool)) else PointShards(enabled=bool(sp))
        self._update_param_cache()

    @classmethod
    def from_grid(cls, axes, Y, kernel, *, mask=None, sigmasq: float = None, eps: float = 1e-2, nufft_eps: float = 1e-4,
                  opts: Optional[Dict] = None, estimate_params: bool = True):
        """A model of observations that lie on the rectilinear raster axes[0] x .. x axes[d-1] ("ij" order): `Y` of shape
        (n_0, .., n_{d-1}), `axes` d one-dimensional coordinate tensors (any spacing, any order; checked as `predict_grid` checks
        its axes), `mask` a bool tensor of Y's shape, True = observed (None: the finite cells of Y are the observations).

        Such a gridded model never holds the (N, d) coordinate tensor and builds no point layout: every pass over the observations
        (F* y, the Toeplitz vector, the trace probes, the sampler's noise transform) is an exact separable sum on the raster
        (`efgp_hip.RasterPlan`: `raster_type1` / `raster_type2`, no spreading window, `nufft_eps` plays no part in them).  `fit`,
        `predict`, `predict_grid`, `sample_paths`, `sample_paths_grid`, `sample_posterior(method="efgp")`, `compute_gradients`
        (adjoint estimator), `compute_log_marginal` and `optimize_hyperparameters` work as on a point model;
        `last_fit_stats["route"]` is "raster".  Refused: opts["shard_points"], the literal and `pointwise_alpha` gradient modes,
        `sample_posterior(method="dense")`.

        N is the number of observed cells; the domain length (or sides, for an ARD kernel) comes from the axes' extremes; the
        initial hyper-parameter estimate runs on the coordinates of at most 4096 observed cells taken at a fixed stride."""
        if opts and opts.get("shard_points", False):
            raise NotImplementedError("a gridded model (EFGPND.from_grid) does not support opts['shard_points']: the raster is "
                                      "transformed on one device")
        Y = torch.as_tensor(Y)
        if not Y.is_floating_point():
            Y = Y.to(torch.float64)
        if Y.ndim < 1 or Y.ndim > 3:
            raise ValueError(f"from_grid: Y must have 1, 2 or 3 dimensions (got shape {tuple(Y.shape)})")
        axes = _check_axes(axes, Y.ndim, "from_grid")
        n_axis = tuple(int(a.numel()) for a in axes)
        if tuple(Y.shape) != n_axis:
            raise ValueError(f"from_grid: Y has shape {tuple(Y.shape)}, the axes span {n_axis}")
        if mask is None:
            obs = torch.isfinite(Y)
        else:
            obs = torch.as_tensor(mask)
            if obs.dtype != torch.bool or tuple(obs.shape) != n_axis:
                raise ValueError(f"from_grid: mask must be a bool tensor of Y's shape {n_axis}")
            obs = obs.to(Y.device)
            if not bool(torch.isfinite(Y[obs]).all()):
                raise ValueError("from_grid: Y is not finite in every observed cell")
        n_obs = int(obs.sum())
        if n_obs == 0:
            raise ValueError("from_grid: the raster has no observed cell")
        # at most 4096 observed cells at a fixed stride through the row-major raster, the stride coprime to the cell count so
        # that it walks across every axis
        cells = prod(n_axis)
        step = -(-cells // 4096)
        while math.gcd(step, cells) != 1:
            step += 1
        idx = torch.arange(0, cells, step, device=Y.device)
        idx = idx[obs.reshape(-1)[idx]]
        if idx.numel() == 0:
            idx = obs.reshape(-1).nonzero().reshape(-1)[:4096]
        y_sub = Y.reshape(-1)[idx]
        cols = []
        for a in reversed(range(len(axes))):
            cols.append(axes[a].to(device=Y.device, dtype=Y.dtype)[idx % n_axis[a]])
            idx = idx // n_axis[a]
        model = cls(torch.stack(cols[::-1], dim=1), y_sub, kernel, sigmasq=sigmasq, eps=eps, nufft_eps=nufft_eps, opts=opts,
                    estimate_params=estimate_params)
        model._raster = dict(axes=axes, Y=Y, obs=obs, N=n_obs, n_axis=n_axis)
        return model

    # -- parameter bookkeeping ------------------------------------------------------------------
    def register_optimizer(self, optimizer):
        """Wrap optimizer.step so the hyper-parameter cache is refreshed after every step."""
        if optimizer in self._registered_optimizers:
            return optimizer
        inner = optimizer.step

        def step_and_sync(*a, **k):
            res = inner(*a, **k)
            self._update_param_cache()
            return res

        optimizer.step = step_and_sync
        self._registered_optimizers.append(optimizer)
        return optimizer

    @property
    def sigmasq(self) -> torch.Tensor:
        return self._gp_params.sig2

    @property
    def last_gradient_stats(self) -> Dict:
        """Diagnostics of the last gradient step (reading them waits for its asynchronous solves)."""
        st = self._last_gradient_stats
        for key in ("mean_cg_iters", "trace_cg_iters"):
            if key in st and not isinstance(st[key], int):
                st[key] = int(st[key])
        return st

    @property
    def last_fit_stats(self) -> Dict:
        """Diagnostics of the last fit (reading them waits for an asynchronous solve to finish)."""
        st = dict(self._last_fit_stats)
        if "mean_cg_iters" in st:
            st["mean_cg_iters"] = int(st["mean_cg_iters"])
        return st

    def _current_hypers(self):
        vals = {name: float(self.kernel.get_hyper(name)) for name in getattr(self.kernel, "hypers", [])}
        vals["sigmasq"] = float(self.sigmasq.detach())
        return vals

    def _update_param_cache(self):
        if isinstance(self.kernel, str):
            self._cached_params["kernel_type"] = str(type(self.kernel))
        else:
            for name, value in self.kernel.iter_hypers():
                self._cached_params[name] = float(value)
        self._cached_params["sigmasq"] = self._gp_params.host_pos()[-1]
        return self

    def _params_changed(self):
        if not self._cached_params:
            return True
        try:
            for name, value in self.kernel.iter_hypers():
                if name not in self._cached_params or abs(self._cached_params[name] - float(value)) > 1e-8:
                    return True
        except (AttributeError, TypeError):
            if self._cached_params.get("kernel_type") != str(type(self.kernel)):
                return True
        if "sigmasq" not in self._cached_params or \
                abs(self._cached_params["sigmasq"] - float(self.sigmasq.detach())) > 1e-8:
            return True
        # the fit itself remembers the hyper-parameters it was computed with
        if self._fit_state is not None:
            now = self._current_hypers()
            then = self._fit_state["hypers"]
            return any(abs(now[k] - then.get(k, float("nan"))) > 1e-8 for k in now)
        return False

    # -- device data ------------------------------------------------------------------------------
    def _device_data(self):
        if self._devdata is None and self._raster is not None:
            r = self._raster
            dev = compute_device(r["Y"])
            ax = [a.to(device=dev, dtype=torch.float64).contiguous() for a in r["axes"]]
            obs = r["obs"].to(dev)
            yd = torch.where(obs, r["Y"].detach().to(device=dev, dtype=torch.float64), 0.0).reshape(-1).contiguous()
            mask = None if r["N"] == obs.numel() else obs.to(torch.float64).reshape(-1).contiguous()
            sides = torch.stack([a.max() - a.min() for a in ax]).tolist()          # the axes' extremes, one read-back
            L = _box_L(sides, hasattr(self.kernel, "ard_kind"))
            yy = self._shards.sum_scalars([vdot_real(yd, yd)], dev)[0]
            self._devdata = dict(dev=dev, x=None, y=yd, L=L, N=r["N"], yy=yy, points=None, passes=0, axes=ax, mask=mask)
        if self._devdata is None:
            dev = compute_device(self.x)
            xd = _dev_points(self.x, dev)
            yd = self.y.detach().to(device=dev, dtype=torch.float64).contiguous()
            L = _points_box(xd, self._shards, hasattr(self.kernel, "ard_kind"))
            n_glob = int(self._shards.sum_scalars([xd.shape[0]], dev)[0]) if self._shards.active else xd.shape[0]
            yy = self._shards.sum_scalars([vdot_real(yd, yd)], dev)[0]          # global sum of y^2 (gradient, once)
            self._devdata = dict(dev=dev, x=xd, y=yd, L=L, N=n_glob, yy=yy, points=None, passes=0, layout_values=yd)
        return self._devdata

    def _layout(self):
        """The model's point layout (grid-independent sorted copies for the type-1 pass, bounding box, max|y| once per model), or
        None while it is not worth building.  opts["point_layout"]: "auto" (default) -- from the SECOND pass over the points
        on: a model that is fitted once (efgp_nd, predict-only use; efgpnd_variance_shootout.py:129-137) never pays the sort
        (bounding box + key + radix sort + two gathers: 0.5 ms at N = 1e6, 8-13 ms at 1e7), a training loop pays it at its second
        step and streams the sorted copies from then on; True -- from the first pass; False -- never."""
        dd = self._device_data()
        if self._raster is not None:              # a gridded model has no point layout
            return None
        want = self.opts.get("point_layout", "auto")
        dd["passes"] += 1
        if want is False or dd["x"].shape[0] == 0 or (want == "auto" and dd["passes"] < 2):
            return None
        if dd["points"] is None:
            dd["points"] = PointSet(dd["x"], values=dd["layout_values"])
        return dd["points"]

    # -- gradient -----------------------------------------------------------------------------------
    def compute_gradients(self, *, trace_samples: int = 10, do_profiling: bool = False,
                          nufft_eps: Optional[float] = None, cg_tol: Optional[float] = None,
                          noise_floor: Optional[float] = None, apply_gradients: bool = True,
                          compute_log_marginal: bool = False, log_marginal_probes: int = 100,
                          log_marginal_steps: int = 25, verbose: bool = False, **kwargs):
        """Gradient of the negative log marginal likelihood w.r.t. the log-space parameters
        (kernel hypers..., sigma^2); written to ``self._gp_params.raw.grad`` when apply_gradients."""
        self._update_param_cache()
        if nufft_eps is None:
            nufft_eps = self.eps * 0.1
        if noise_floor is None:
            noise_floor = self.opts.get("noise_floor")
        if cg_tol is None:
            cg_tol = 0.1 * self.eps
        warm = self.opts.get("mean_cg_warm_start", True)
        stats: Dict = {}
        dd = self._device_data()
        if self._raster is not None:
            if kwargs.get("trace_mode", "adjoint") != "adjoint" or kwargs.get("pointwise_alpha", False):
                raise NotImplementedError("a gridded model (EFGPND.from_grid) supports the adjoint gradient estimator only: the "
                                          "literal and pointwise_alpha modes need a complex type-2 transform onto the raster")
            kwargs["raster"] = (dd["axes"], dd["mask"], dd["N"])
        res = efgpnd_gradient_batched(
            self.x if self._raster is not None else dd["x"], dd["y"], sigmasq=self._gp_params.host_pos()[-1], kernel=self.kernel, eps=self.eps,
            trace_samples=trace_samples, do_profiling=do_profiling, nufft_eps=nufft_eps, cg_tol=cg_tol,
            noise_floor=noise_floor, stats_out=stats,
            mean_cg_init=self._last_gradient_beta if warm else None, mean_cg_init_shape=getattr(self, "_last_gradient_shape", None),
            use_mean_cg_preconditioner=self.opts.get("mean_cg_preconditioner", True),
            use_trace_cg_preconditioner=self.opts.get("trace_cg_preconditioner", True),
            compute_log_marginal=compute_log_marginal, log_marginal_probes=log_marginal_probes,
            log_marginal_steps=log_marginal_steps, shards=self._shards, domain_length=dd["L"], y_norm_sq=dd["yy"],
            points=self._layout(), **kwargs)
        self._last_gradient_beta = stats.pop("mean_beta", None)
        self._last_gradient_shape = tuple(stats["shape"]) if "shape" in stats else None
        grad_host = stats.pop("grad_host", None)       # the native tail reads grad | term1 | term2 back in one copy
        self._last_gradient_stats = stats
        grads, log_marginal = res if compute_log_marginal else (res, None)
        if grads.ndim == 0:
            grads = grads.unsqueeze(0)
        raw = self._gp_params.raw
        pos = raw.detach().exp()                         # = pos, without recording the exp for autograd
        if grad_host is not None and raw.device.type == "cpu":
            grads = grad_host
        raw_grad = grads.detach().to(device=raw.device, dtype=raw.dtype) * pos               # chain rule d/dlog
        if apply_gradients:
            with torch.no_grad():
                raw.grad = raw_grad.detach().clone()
        return (raw_grad, log_marginal) if compute_log_marginal else raw_grad

    # -- fit -----------------------------------------------------------------------------------------
    def _compute_common_parameters(self, force_recompute: bool = False, nufft_eps: Optional[float] = None) -> None:
        """Fit: grid, one fused pass over the points for (F*y, Toeplitz vector), Jacobi-PCG for beta."""
        self._update_param_cache()
        if self._fitted and not force_recompute and not self._params_changed():
            return
        if nufft_eps is None:
            nufft_eps = self.nufft_eps
        dd = self._device_data()
        dev, xd, yd = dd["dev"], dd["x"], dd["y"]
        d = xd.shape[1] if self._raster is None else len(dd["axes"])
        sig = self._gp_params.host_pos()[-1]
        rdtype = self.x.dtype
        cdtype = _cmplx(rdtype)

        grid = _Grid(self.kernel, self.eps, dd["L"], d, dev, defer_weights=True)
        warm = self.opts.get("mean_cg_warm_start", True) and self._beta is not None and tuple(self._beta.shape) == (grid.M,) \
            and (self._fit_state is None or tuple(self._fit_state["shape"]) == tuple(grid.shape))      # same block, not just the same M
        # Cold start of a built-in kernel on a 2-D grid: the weights may be made inside the mean solve (below); elsewhere they are
        # made now, ahead of the pass over the points
        bk = _builtin_kernel_constants(self.kernel) if (d == 2 and not warm and dev.type == "cuda" and
                                                        not os.environ.get("EFGP_NO_NATIVE_GRID")) else None
        if bk is None:
            grid.make_weights()
        if self._raster is not None:            # exact separable sums on the raster: no coordinates, no layout, no window
            plan = RasterPlan(dd["axes"], grid.plan_h, cell_scale=dd["mask"], _scale_checked=True)
        else:
            plan = NufftPlan(xd, grid.plan_h, min(float(nufft_eps), _CONV_TOL), points=self._layout())
        Fy, v = _normal_equations(plan, yd, grid, self._shards)
        Fy_rhs, rescale = Fy, None
        if self._raster is not None:
            # The CG kernels guard <r, z> and <p, A p> with an absolute 1e-16 (as the reference's loop does), which stalls them
            # near |r| = 1e-8 whatever the tolerance: for data of order one a cg_tolerance below ~1e-9 is never met and the
            # solve runs to its cap.  beta is linear in y, so the gridded fit solves for 2^k y with |2^k y| near 2^40 and
            # scales beta back -- both exact -- which makes the tolerance asked for reachable in any units of y.
            k = max(-900, min(900, 40 - math.frexp(math.sqrt(float(dd["yy"])) or 1.0)[1]))
            Fy_rhs, rescale = Fy * (2.0 ** k), 2.0 ** -k
        # deferred: on the 48 x 48 Hermitian grids the operator launches nothing; the fused solve makes its spectrum
        toeplitz = ToeplitzND(v, force_pow2=True, defer_spectra=bk is not None)
        use_precond = self.opts.get("mean_cg_preconditioner", True)
        tol = self.opts.get("cg_tolerance", 1e-4)
        # Cold start on a grid that fits the single-launch kernel: rhs = ws*F*y (:792), the Jacobi diagonal
        # v[0]|ws|^2 + sigma^2 (:795-799) and beta_0 = 0 are formed inside the solve kernel -- one launch, no host
        # synchronisation (the iteration count stays on the device until somebody reads last_fit_stats).  On the 48 x 48 grids
        # of a built-in kernel that launch also evaluates ws and makes the operator's spectrum (efgp_cg_solve_mean_fused).
        res = None
        if bk is not None:
            (kind, nu, c0), ell, _var = bk
            fused = cg_solve_mean_fused(toeplitz._op, kind, nu, c0, ell, grid.h, grid.mtot, sig,
                                        _center_value(v) if use_precond else None, Fy_rhs, tol, early_stop=True)
            if fused is not None:
                beta_f, grid.ws, iters_f = fused
                res = (beta_f, iters_f)
        grid.make_weights()                        # no-op when the fused solve made them
        if res is None and not warm:
            res = cg_solve_mean_async(toeplitz._op, grid.ws, sig, _center_value(v) if use_precond else None, Fy_rhs, tol,
                                      early_stop=True)
        if res is None:
            # rhs = D F*y (:792) and the Jacobi diagonal (:795-799) in one native launch (four torch launches otherwise, whose first
            # use in a process costs 0.3 s of torch's own lazy kernel loading)
            cidx = _center_flat(v)
            diag, rhs = gradient_prepare(grid.ws, Fy_rhs, v.reshape(-1)[cidx:cidx + 1], sig, want_diag=use_precond)
            b0 = self._beta.detach().to(device=dev, dtype=torch.complex128) if warm else None
            if warm and rescale is not None:
                b0 = b0 / rescale
            res = cg_solve_lazy(toeplitz._op, grid.ws, sig, 0, rhs, b0, tol, early_stop=True, diag=diag, batched=False,
                                hermitian=True)         # 3-D grids: the planes k0 >= 0 only (efgp_cg_solve_hermitian)
        beta, iters = res
        if rescale is not None:
            iters.settle()                         # a re-solve writes into the scaled vector: before it is scaled back
            beta = beta * rescale
        self._beta = beta.to(cdtype) if cdtype != torch.complex128 else beta
        self._xis = (grid, rdtype)                 # the (M, d) node tensor is built when somebody asks for it (property below)
        self._ws = grid.ws.to(cdtype) if cdtype != torch.complex128 else grid.ws
        self._toeplitz = toeplitz
        # h, mtot: the scalars of an isotropic grid (None for an ARD kernel); hs, shape, plan_h describe every grid
        self._fit_state = dict(h=grid.h, mtot=grid.mtot, d=d, sig=sig, ws=grid.ws, beta=beta,
                               hypers=self._current_hypers(), Fy=Fy, v=v, shape=grid.shape, hs=grid.hs, plan_h=grid.plan_h, ard=grid.ard)
        if grid.ard:
            self._last_fit_stats = dict(mean_cg_iters=iters, feature_count=grid.M, hs=grid.hs, shape=grid.shape)
        else:
            self._last_fit_stats = dict(mean_cg_iters=iters, mtot=grid.mtot, feature_count=grid.M, h=grid.h)
        if self._raster is not None:
            self._last_fit_stats["route"] = "raster"
        self._fitted = True
        self._update_param_cache()
        # Nothing downstream reads the count before using beta: a solve that may hold a dead system is settled HERE -- last, behind
        # the host's own bookkeeping, which thereby still overlaps the solve.  beta and the count are repaired in place.
        if iters.settle() and cdtype != torch.complex128:
            self._beta = beta.to(cdtype)

    @property
    def _xis(self):
        """(M, d) frequency nodes of the last fit (reference attribute `_xis`, efgpnd.py:816), materialised on first access."""
        src = self.__dict__.get("_xis_src")
        if src is None:
            return None
        if not torch.is_tensor(src):
            grid, rdtype = src
            xis = grid.xis.to(dtype=rdtype)
            if not grid.ard:
                xis.h_float = grid.h
            self.__dict__["_xis_src"] = src = xis
        return src

    @_xis.setter
    def _xis(self, value):
        self.__dict__["_xis_src"] = value

    def fit(self, force_recompute: bool = True):
        """Convenience: run the fit now (the reference fits lazily inside predict)."""
        self._compute_common_parameters(force_recompute=force_recompute)
        return self

    # -- predict ---------------------------------------------------------------------------------------
    def _plan_at(self, xn, nufft_eps):
        """The plan over the new points `xn`, kept while the same tensor (same storage, same version) comes back with the same
        grid: predicting at the training points after every refit is the reference's own usage (efgpnd_ex.ipynb cell 23)."""
        st = self._fit_state
        pkey = (xn.data_ptr(), tuple(xn.shape), xn._version, st["plan_h"], float(nufft_eps))
        if self._predict_plan is None or self._predict_plan[0] != pkey:
            self._predict_plan = (pkey, NufftPlan(xn, st["plan_h"], float(nufft_eps)))
        return self._predict_plan[1]

    def _nan_like(self, shape):
        """NaN of `shape`, where no variance was asked for.  The reference fills a (B,) tensor with NaN (efgpnd.py:947): same values
        as a stride-0 view of ONE NaN, made once per model, without writing 8 B bytes per call (16 us and 80 MB of traffic per
        predict at N = 1e7)."""
        rdtype = self.x.dtype
        if self._nan_scalar is None or self._nan_scalar.device != self.device or self._nan_scalar.dtype != rdtype:
            self._nan_scalar = torch.full((1,), float("nan"), device=self.device, dtype=rdtype)
        return self._nan_scalar.expand(shape)

    # What a subclass with other coefficients supplies (EFGPNDMulti): the two means and the log marginal that `predict` appends
    def _mean_at(self, plan):
        st = self._fit_state          # the shape is carried explicitly (the reference re-derives it, :908)
        return plan.type2(st["beta"], st["shape"], real_only=True, mode_scale=st["ws"])     # F (ws * beta), efgpnd.py:919-922

    def _mean_on_raster(self, ax):
        st = self._fit_state
        return raster_type2(ax, st["plan_h"], st["shape"], st["beta"], mode_scale=st["ws"])        # F (ws * beta) on the raster

    def _predict_log_marginal(self):
        st = self._fit_state
        return self._compute_log_marginal(beta=st["beta"], ws=st["ws"], sigmasq=st["sig"], toeplitz=self._toeplitz,
                                          device=self._devdata["dev"], rdtype=self.x.dtype, n=self._devdata["N"])

    def _variance_at(self, xn, variance_method, hutchinson_probes, nufft_eps, variance_probes):
        """The latent variance at the points `xn` (on the compute device); it depends on the points and the hyper-parameters only."""
        st = self._fit_state
        rdtype = self.x.dtype
        if variance_probes is None and self._shards.active and variance_method.lower() == "stochastic":
            # replicas must estimate the SAME lag sums: rank 0's draw (reference draw: efgpnd.py:1644)
            variance_probes = (torch.randint(0, 2, (hutchinson_probes, st["ws"].numel()), device=xn.device) * 2 - 1).to(torch.float64)
            self._shards.broadcast_(variance_probes)
        A_var = create_A_var(st["ws"], self._toeplitz, st["sig"], torch.complex128)
        return compute_prediction_variance(
            x_new=xn, xis=self._xis.to(torch.float64), ws=st["ws"], A_var=A_var,
            cg_tol=self.opts.get("cg_tolerance", 1e-4), max_cg_iter=self.opts.get("max_cg_iterations", 1000),
            variance_method=variance_method, h=st["plan_h"], xcen=torch.zeros(xn.shape[1], dtype=torch.float64),
            hutchinson_probes=hutchinson_probes, nufft_eps=nufft_eps, device=self.device, rdtype=rdtype,
            cdtype=_cmplx(rdtype), probes=variance_probes, shards=self._shards if self._shards.active else None,
            shape=st["shape"] if st["ard"] else None)

    def predict(self, x_new: torch.Tensor, *, return_variance: bool = True, variance_method: str = "stochastic",
                hutchinson_probes: int = 1_000, compute_log_marginal: bool = False, force_recompute: bool = False,
                do_profiling: bool = False, nufft_eps: Optional[float] = None, variance_probes: Optional[torch.Tensor] = None):
        """Posterior mean (and latent variance) at x_new -> (mean, var[, log_marginal])."""
        if x_new is None:
            raise ValueError("x_new must be provided for prediction")
        self._compute_common_parameters(force_recompute=force_recompute, nufft_eps=nufft_eps)
        st = self._fit_state
        if nufft_eps is None:
            nufft_eps = self.nufft_eps
        dev = self._devdata["dev"]
        xn = _dev_points(x_new, dev)
        B, d = xn.shape
        if d != st["d"]:
            raise ValueError(f"x_new has {d} columns, the model was built on {st['d']}")
        t0 = time.perf_counter()
        ranges = _StageRanges(f"{type(self).__name__}.predict", "predict_mean")
        out_mean = self._mean_at(self._plan_at(xn, nufft_eps)).to(device=self.device, dtype=self.x.dtype)
        t1 = time.perf_counter()
        if return_variance:
            ranges.stage("compute_variance")
            var = self._variance_at(xn, variance_method, hutchinson_probes, nufft_eps, variance_probes)
        else:
            var = self._nan_like((B,))
        t2 = time.perf_counter()
        ranges.close()
        if do_profiling:
            torch.cuda.synchronize(dev)
            print(f"predict_mean {t1 - t0:.6f}s  compute_variance {t2 - t1:.6f}s")
        return (out_mean, var, self._predict_log_marginal()) if compute_log_marginal else (out_mean, var)

    # -- posterior gradients ---------------------------------------------------------------------------
    # The fitted model is a finite trigonometric sum, so its partial derivatives are exact in the same feature space: mode k of the
    # partial along axis a is 2 pi i xi_ka times mode k of the mean (efgp_hip.mode_jet_rows), through the transforms of the mean.
    def _xi_axes(self):
        """xi_a of every mode, a = 0 .. d - 1: d device vectors (M,) in the row-major order of the mode box, kept with the fit."""
        st = self._fit_state
        if "xi_axes" not in st:
            dev = st["ws"].device
            shape = tuple(int(n) for n in st["shape"])
            cols = []
            for a, (n, h) in enumerate(zip(shape, st["hs"])):
                k = torch.arange(-(n // 2), (n - 1) // 2 + 1, dtype=torch.float64, device=dev) * float(h)
                view = [1] * len(shape)
                view[a] = n
                cols.append(k.view(view).expand(shape).reshape(-1))
            st["xi_axes"] = cols
        return st["xi_axes"]

    # What a subclass with other coefficients supplies (EFGPNDMulti): value and gradient of the mean from ONE pass
    def _jet_at(self, plan):
        """-> (mean (N*,), grad (N*, d)) on the compute device."""
        st = self._fit_state
        jet = plan.type2_jet(st["beta"], st["shape"], mode_scale=st["ws"])[0]
        return jet[0], jet[1:].T

    def _jet_on_raster(self, ax):
        """-> (mean (n_0, ..), grad (d, n_0, ..)) on the compute device."""
        st = self._fit_state
        jet = raster_type2_jet(ax, st["plan_h"], st["shape"], st["beta"], mode_scale=st["ws"])[0]
        return jet[0], jet[1:]

    def _gradient_lag_sums(self, hutchinson_probes, variance_probes):
        """The d lag boxes of the stochastic variance of the partials, stacked (d, 2 n_0 - 1, ..)."""
        st = self._fit_state
        A_var = create_A_var(st["ws"], self._toeplitz, st["sig"], torch.complex128)
        ests = diag_sums_gradient_nd(A_var, hutchinson_probes, self._xis.to(torch.float64), self.opts.get("max_cg_iterations", 1000),
                                     self.opts.get("cg_tolerance", 1e-4), st["ws"], self._xi_axes(), probes=variance_probes,
                                     shape=st["shape"] if st["ard"] else None)
        return torch.stack(ests)

    def _gradient_variance_regular(self, xb):
        st = self._fit_state
        A_var = create_A_var(st["ws"], self._toeplitz, st["sig"], torch.complex128)
        return gradient_variance_regular(xb, self._xi_axes(), st["ws"], A_var, self.opts.get("cg_tolerance", 1e-4),
                                         self.opts.get("max_cg_iterations", 1000), st["plan_h"], shape=st["shape"] if st["ard"] else None)

    def _gradient_refusals(self, what, return_variance, variance_method):
        if self.opts.get("shard_points", False):
            raise NotImplementedError(f"{what} does not support opts['shard_points']: the jets are transformed on one device")
        if return_variance and variance_method.lower() not in ("regular", "stochastic"):
            raise ValueError(f"Variance method '{variance_method}' not implemented. Choose 'regular' or 'stochastic'.")

    def predict_gradient(self, x_new: torch.Tensor, *, return_variance: bool = True, variance_method: str = "stochastic",
                         hutchinson_probes: int = 1_000, variance_probes: Optional[torch.Tensor] = None,
                         nufft_eps: Optional[float] = None, return_mean: bool = False, force_recompute: bool = False):
        """Gradient of the posterior mean at x_new and the latent variance of every partial -> (grad (N*, d), grad_var (N*, d));
        return_mean=True: (mean (N*,), grad, grad_var), the mean out of the same pass over the points.

        Nothing is approximated beyond what `predict` approximates: the partial along axis a multiplies mode k by 2 pi i xi_ka
        (`efgp_hip.mode_jet_rows`), and the 1 + d real-only rows ride two per complex fine grid through the type 2 of `predict`.
        "stochastic": the Hutchinson solves of `predict` (same probe handling: `variance_probes` (J, M) of +-1 may be injected)
        with frequency-weighted lag sums per axis; "regular": the per-point solves of `predict` with the derivative rows, 8192
        points at a time.  return_variance=False returns NaN of the gradient's shape as a stride-0 view."""
        self._gradient_refusals("predict_gradient", return_variance, variance_method)
        if x_new is None:
            raise ValueError("x_new must be provided for prediction")
        self._compute_common_parameters(force_recompute=force_recompute, nufft_eps=nufft_eps)
        st = self._fit_state
        if nufft_eps is None:
            nufft_eps = self.nufft_eps
        dev = self._devdata["dev"]
        xn = _dev_points(x_new, dev)
        B, d = xn.shape
        if d != st["d"]:
            raise ValueError(f"x_new has {d} columns, the model was built on {st['d']}")
        plan = self._plan_at(xn, nufft_eps)
        mean, grad = self._jet_at(plan)
        if not return_variance:
            var = self._nan_like((B, d))
        else:
            if variance_method.lower() == "stochastic":
                ests = self._gradient_lag_sums(hutchinson_probes, variance_probes)
                var = plan.type2(ests, tuple(ests.shape[1:]), modeord=1, real_only=True, batched=True).T
            else:
                var = self._gradient_variance_regular(xn)
            var = var.to(device=self.device, dtype=self.x.dtype)
        grad = grad.to(device=self.device, dtype=self.x.dtype)
        return (mean.to(device=self.device, dtype=self.x.dtype), grad, var) if return_mean else (grad, var)

    def predict_gradient_grid(self, axes, *, return_variance: bool = True, variance_method: str = "stochastic",
                              hutchinson_probes: int = 1_000, variance_probes: Optional[torch.Tensor] = None, return_mean: bool = False,
                              force_recompute: bool = False):
        """`predict_gradient` on the rectilinear raster axes[0] x .. x axes[d-1] -> (grad (d, n_0, .., n_{d-1}), grad_var of the same
        shape), return_mean=True prepends the mean map: the jets through the exact raster transform of `predict_grid` (arguments
        as there); the "regular" variance is fed 8192 raster cells at a time in row-major order."""
        self._gradient_refusals("predict_gradient_grid", return_variance, variance_method)
        axes = self._grid_axes(axes, "predict_gradient_grid")
        self._compute_common_parameters(force_recompute=force_recompute)
        st = self._fit_state
        dev = self._devdata["dev"]
        ax = [a.to(dev) for a in axes]
        n_axis = tuple(int(a.numel()) for a in ax)
        d = len(ax)
        mean, grad = self._jet_on_raster(ax)
        if not return_variance:
            var = self._nan_like((d,) + n_axis)
        else:
            if variance_method.lower() == "stochastic":
                ests = self._gradient_lag_sums(hutchinson_probes, variance_probes)
                var = raster_type2(ax, st["plan_h"], tuple(ests.shape[1:]), ests, modeord=1, batched=True)
            else:
                var = torch.cat([self._gradient_variance_regular(xb) for xb in _raster_cell_blocks(ax, n_axis, dev)]).T.reshape((d,) + n_axis)
            var = var.to(device=self.device, dtype=self.x.dtype)
        grad = grad.to(device=self.device, dtype=self.x.dtype)
        return (mean.to(device=self.device, dtype=self.x.dtype), grad, var) if return_mean else (grad, var)

    # -- function draws ----------------------------------------------------------------------------------
    @property
    def last_sample_stats(self) -> Dict:
        """Seed, row count and per-row CG iteration counts of the last `sample_paths` call (reading them waits for its solves);
        `cg_capped` lists the rows that reached `cg_max_iterations` without meeting the tolerance."""
        st = dict(self._last_sample_stats)
        if "cg_iters" in st:
            st["cg_iters"] = [int(v) for its in st["cg_iters"] for v in its.rows]
            st["cg_capped"] = [i for i, v in enumerate(st["cg_iters"]) if v >= st["cg_max_iterations"]]
        return st

    def _draw_weight_blocks(self, nsamples, prior, seed, cg_tolerance, keep, transform):
        """The weight draws of `sample_paths` and `sample_paths_grid`, in blocks of `_SAMPLE_BLOCK` rows: w (nb, M) of every block
        goes through `transform` (the type-2 of the caller's points) -> (list of its outputs, max_iter, tol); the last two are None
        for the prior.  `keep`: None or the lists of `return_state`.  Sets `_last_sample_stats`."""
        st = self._fit_state
        dev = self._devdata["dev"]
        d, M = st["d"], st["ws"].numel()
        shape = st["shape"]
        max_iter = tol = None
        seed_e1, seed_e2 = _derive_seed(seed, 1), _derive_seed(seed, 2)
        block = _SAMPLE_BLOCK[d]
        sig = st["sig"]
        sols = []
        if not prior:
            tol = float(cg_tolerance) if cg_tolerance is not None else self.opts.get("cg_tolerance", 1e-4)
            points = self._layout()
            # kept while the grid spacing, the tolerance and the layout object stay what the plan was made with (a refit
            # replaces _fit_state; what the plan depends on is h)
            tol1 = min(float(self.nufft_eps), _CONV_TOL)
            sp = self._sample_plan
            if self._raster is not None and (sp is None or sp[0] != (st["plan_h"], tol1)):
                self._sample_plan = sp = ((st["plan_h"], tol1), RasterPlan(self._devdata["axes"], st["plan_h"],
                                                                          cell_scale=self._devdata["mask"], _scale_checked=True), None)
            elif sp is None or sp[0] != (st["plan_h"], tol1) or sp[2] is not points:
                self._sample_plan = sp = ((st["plan_h"], tol1), NufftPlan(self._devdata["x"], st["plan_h"], tol1, points=points), points)
            plan_x = sp[1]
            max_iter = int(self.opts.get("max_cg_iterations", 1000))
            diag = _jacobi_diag(st["ws"], st["v"], sig) if self.opts.get("mean_cg_preconditioner", True) else None
            sroot = math.sqrt(sig)
        outs = []
        for r0 in range(0, nsamples, block):
            nb = min(block, nsamples - r0)
            if prior:
                w = hermitian_normal_rows(dev, seed_e2, nb, M, a=0.0, b=1.0, index_offset=normal_row_offset(2 * r0))
            else:
                fz = plan_x.type1_normal(seed_e1, nb, shape, index_offset=normal_row_offset(r0)).reshape(nb, M)
                rhs = hermitian_normal_rows(dev, seed_e2, nb, M, a=sroot, ws=st["ws"], fz=fz, b=sig,
                                            index_offset=normal_row_offset(2 * r0))
                delta, its = cg_solve_lazy(self._toeplitz._op, st["ws"], sig, 0, rhs, None, tol,
                                           max_iter=max_iter, early_stop=True, diag=diag,
                                           batched=True, hermitian=True)
                its.settle()                         # reads the counts only where the solve may hold dead rows
                sols.append(its)
                # The solution of a conjugate-even system is conjugate-even.  The Hermitian kernels iterate on the full vector
                # and control only its even part: over the ~1000 iterations these broad-spectrum right-hand sides take at
                # N = 1e6 the odd part grows from rounding to 1e-5..1e-3 of the solution (the fit's 10-300 iterations never
                # show it).  It drops out of Re F(ws w) anyway; projecting it out makes delta and the weights what they mean.
                delta = delta.reshape(nb, M)
                delta = 0.5 * (delta + delta.flip(1).conj())
                w = delta + st["beta"].reshape(1, M)
                if keep is not None:
                    keep["delta"].append(delta)
                    keep["rhs"].append(rhs)
            if keep is not None:
                keep["weights"].append(w)
            outs.append(transform(w))
        self._last_sample_stats = dict(seed=seed, nsamples=nsamples, prior=bool(prior), blocks=-(-nsamples // block))
        if not prior:
            self._last_sample_stats["cg_iters"] = sols
            self._last_sample_stats["cg_max_iterations"] = max_iter
        return outs, max_iter, tol

    def sample_paths(self, x_new: torch.Tensor, nsamples: int, *, prior: bool = False, seed: Optional[int] = None,
                     cg_tolerance: Optional[float] = None, return_state: bool = False, gradient: bool = False):
        """Draws of the latent function at x_new -> (nsamples, B), from the posterior (default) or the prior, in the weight space
        of the equispaced features: with D = diag(ws), A = D F*F D + sigma^2 I and the weights' prior N(0, I),

            w = beta + A^-1 (sigma D F* e1 + sigma^2 e2),   f(x*) = Re F_new (ws * w),

        e1 ~ N(0, I_N) real and e2 a conjugate-even standard complex normal on the mode grid (the bracket has covariance
        sigma^2 A, so w ~ N(beta, sigma^2 A^-1), the posterior of the weights).  One draw costs one type-1 transform of a noise
        row generated inside the spreader (e1 never exists in memory), one Hermitian CG solve with the fit's operator and one
        type-2 transform, all batched over blocks of `_SAMPLE_BLOCK` rows.  prior=True draws w = e2 alone: no pass over the
        training points, no solve.

        seed=None takes a 63-bit seed from torch's default generator (`torch.manual_seed` governs reproducibility); an integer
        makes the call a pure function of (model, x_new, nsamples, seed).  Rows are numbered across blocks: the first k rows of a
        larger call are the draws of a k-row call (to rounding).  return_state=True also returns a dict with `seed`, `weights`
        (nsamples, M), `delta`, `rhs`, `cg_iters`, `cg_max_iterations` and `cg_capped` (posterior; None for the prior).

        The noise right-hand sides excite every mode, not only the smooth ones of the data term, so their solves take about
        sqrt(cond A) ln(2 / tol) / 2 iterations at worst (785-1104 measured at N = 1e6, tolerance 1e-4, where the fit takes 15):
        opts["max_cg_iterations"] (default 1000) caps them.  Rows that reach the cap are returned as they stand; their indices
        are in `last_sample_stats["cg_capped"]` (read on request: no synchronisation in the call) and in the state, and a
        return_state=True call, which reads the counts anyway, warns about them.  The pass over the training points counts as
        one for opts["point_layout"] = "auto": a first sample_paths call after a single fit builds the sorted layout.

        gradient=True returns (draws (nsamples, B), grads (nsamples, B, d)[, state]): the same weight draws under the same seed
        through `NufftPlan.type2_jet` -- every draw with its exact spatial gradient out of one pass over x_new."""
        nsamples = int(nsamples)
        if nsamples < 1:
            raise ValueError(f"nsamples must be at least 1 (got {nsamples})")
        if self.opts.get("shard_points", False):
            raise NotImplementedError("sample_paths does not support opts['shard_points']: the sharded sampler needs an all-reduce "
                                      "of the noise transform F* e1 over the ranks")
        if x_new is None:
            raise ValueError("x_new must be provided for sampling")
        d_model = 1 if self.x.ndim == 1 else self.x.shape[1]
        d_new = 1 if x_new.ndim == 1 else x_new.shape[1]
        if d_new != d_model:
            raise ValueError(f"x_new has {d_new} columns, the model was built on {d_model}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed = int(seed)
        self._compute_common_parameters()
        st = self._fit_state
        rdtype = self.x.dtype
        dev = self._devdata["dev"]
        xn = _dev_points(x_new, dev)
        shape = st["shape"]
        plan_new = self._plan_at(xn, self.nufft_eps)
        keep =dict(weights=[], delta=[], rhs=[]) if return_state else None
        if gradient:
            transform = lambda w: plan_new.type2_jet(w, shape, mode_scale=st["ws"])        # (nb, 1 + d, B)
        else:
            transform = lambda w: plan_new.type2(w, shape, real_only=True, batched=True, mode_scale=st["ws"])
        outs, max_iter, tol = self._draw_weight_blocks(nsamples, prior, seed, cg_tolerance, keep, transform)
        out = outs[0] if len(outs) == 1 else torch.cat(outs)       # one block: the transform's own output, no copy
        if gradient:
            res = (out[:, 0].to(device=self.device, dtype=rdtype), out[:, 1:].permute(0, 2, 1).to(device=self.device, dtype=rdtype))
        else:
            res = out.to(device=self.device, dtype=rdtype)
        if not return_state:
            return res
        state = dict(seed=seed, weights=torch.cat(keep["weights"]),
                     delta=torch.cat(keep["delta"]) if not prior else None,
                     rhs=torch.cat(keep["rhs"]) if not prior else None,
                     cg_iters=None, cg_max_iterations=None, cg_capped=None)
        if not prior:
            stats = self.last_sample_stats
            state.update(cg_iters=stats["cg_iters"], cg_max_iterations=max_iter, cg_capped=stats["cg_capped"])
            if stats["cg_capped"]:
                warnings.warn(f"sample_paths: {len(stats['cg_capped'])} of {nsamples} solves reached max_cg_iterations = {max_iter} "
                              f"without meeting the tolerance {tol:g}; raise opts['max_cg_iterations']", RuntimeWarning, stacklevel=2)
        return res + (state,) if gradient else (res, state)

    # -- maps on rectilinear grids ---------------------------------------------------------------------
    def _grid_axes(self, axes, what):
        """The d coordinate vectors of a rectilinear raster as float64 tensors (where the caller has them); ValueError for a wrong
        count, an axis that is not 1-D or is empty, and non-finite coordinates."""
        if self.opts.get("shard_points", False):
            raise NotImplementedError(f"{what} does not support opts['shard_points']: the raster is evaluated on one device")
        return _check_axes(axes, 1 if self.x.ndim == 1 else self.x.shape[1], what)

    def predict_grid(self, axes, *, return_variance: bool = True, variance_method: str = "stochastic", hutchinson_probes: int = 1_000,
                     variance_probes: Optional[torch.Tensor] = None, force_recompute: bool = False):
        """Posterior mean and latent variance on the rectilinear raster axes[0] x .. x axes[d-1] -> (mean, var), both of shape
        (n_0, .., n_{d-1}) in "ij" order: what `predict` gives at `meshgrid(*axes, indexing="ij")`, without the (prod n, d)
        coordinate tensor, the plan over it and the spreading window.  On a tensor product of coordinates the transform
        separates per axis (`efgp_hip.raster_type2`: phase tables, a contraction per leading axis, a real GEMM on the f64 matrix
        cores), so the map is exact to rounding -- `nufft_eps` plays no part in it.

        axes: d one-dimensional tensors or arrays (any spacing, any order); a single tensor for a 1-D model.  "stochastic" variance:
        the Hutchinson lag sums of `predict` (same probe handling: `variance_probes` (J, M) of +-1 may be injected), evaluated on
        the raster in FFT order; "regular": the per-point solves of `predict`, fed 8192 raster cells at a time in row-major order.
        return_variance=False returns NaN of the raster's shape as a stride-0 view."""
        axes = self._grid_axes(axes, "predict_grid")
        self._compute_common_parameters(force_recompute=force_recompute)
        ax = [a.to(self._devdata["dev"]) for a in axes]
        n_axis = tuple(int(a.numel()) for a in ax)
        out_mean = self._mean_on_raster(ax).to(device=self.device, dtype=self.x.dtype)
        if not return_variance:
            return out_mean, self._nan_like(n_axis)
        return out_mean, self._variance_on_raster(ax, n_axis, variance_method, hutchinson_probes, variance_probes)

    def _variance_on_raster(self, ax, n_axis, variance_method, hutchinson_probes, variance_probes):
        """The latent variance map of `predict_grid` on the raster of the device axes `ax` (n_axis cells per axis)."""
        st = self._fit_state
        dev = self._devdata["dev"]
        A_var = create_A_var(st["ws"], self._toeplitz, st["sig"], torch.complex128)
        cg_tol, max_it = self.opts.get("cg_tolerance", 1e-4), self.opts.get("max_cg_iterations", 1000)
        shape = st["shape"] if st["ard"] else None
        method = variance_method.lower()
        if method == "stochastic":
            est = diag_sums_nd(A_var, hutchinson_probes, self._xis.to(torch.float64), max_it, cg_tol, st["ws"], probes=variance_probes,
                               shape=shape)
            var = raster_type2(ax, st["plan_h"], tuple(est.shape), est.detach(), modeord=1)
        elif method == "regular":
            parts = []
            for xb in _raster_cell_blocks(ax, n_axis, dev):      # the coordinates of 8192 cells at a time
                parts.append(compute_prediction_variance(
                    x_new=xb, xis=None, ws=st["ws"], A_var=A_var, cg_tol=cg_tol, max_cg_iter=max_it, variance_method="regular",
                    h=st["plan_h"], xcen=None, hutchinson_probes=hutchinson_probes, nufft_eps=self.nufft_eps, device=dev,
                    rdtype=torch.float64, cdtype=torch.complex128, shape=shape))
            var = torch.cat(parts).reshape(n_axis)
        else:
            raise ValueError(f"Variance method '{variance_method}' not implemented. Choose 'regular' or 'stochastic'.")
        return var.to(device=self.device, dtype=self.x.dtype)

    def sample_paths_grid(self, axes, nsamples: int, *, prior: bool = False, seed: Optional[int] = None,
                          cg_tolerance: Optional[float] = None, gradient: bool = False):
        """Draws of the latent function on the rectilinear raster axes[0] x .. x axes[d-1] -> (nsamples, n_0, .., n_{d-1}): the
        weight draws of `sample_paths` (same seed, same weights), evaluated by the exact raster transform of `predict_grid`
        instead of a type-2 NUFFT over materialised points.  Arguments as in `sample_paths`; `last_sample_stats` is set alike.
        gradient=True returns (draws, grads (nsamples, d, n_0, .., n_{d-1})) through `raster_type2_jet`."""
        nsamples = int(nsamples)
        if nsamples < 1:
            raise ValueError(f"nsamples must be at least 1 (got {nsamples})")
        axes = self._grid_axes(axes, "sample_paths_grid")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed = int(seed)
        self._compute_common_parameters()
        st = self._fit_state
        dev = self._devdata["dev"]
        ax = [a.to(dev) for a in axes]
        if gradient:
            transform = lambda w: raster_type2_jet(ax, st["plan_h"], st["shape"], w, mode_scale=st["ws"])      # (nb, 1 + d, n_0, ..)
        else:
            transform = lambda w: raster_type2(ax, st["plan_h"], st["shape"], w, batched=True, mode_scale=st["ws"])
        outs, _, _ = self._draw_weight_blocks(nsamples, prior, seed, cg_tolerance, None, transform)
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        if gradient:
            return out[:, 0].to(device=self.device, dtype=self.x.dtype), out[:, 1:].to(device=self.device, dtype=self.x.dtype)
        return out.to(device=self.device, dtype=self.x.dtype)

    def sample_posterior(self, x_new: torch.Tensor, nsamples: int, method: str = "dense", seed: Optional[int] = None):
        """Posterior samples at x_new as a numpy array (B, nsamples).  method="dense": the O(N^3) sampler of the reference
        (small N only; efgpnd.py:974-1022), drawing from torch's default generator; method="efgp": `sample_paths`, which
        scales like the fit (`seed` as there)."""
        if method == "efgp":
            return self.sample_paths(x_new, nsamples, seed=seed).T.detach().cpu().numpy()
        if method != "dense":
            raise ValueError(f"unknown sampling method {method!r}: 'dense' or 'efgp'")
        if self._raster is not None:
            raise NotImplementedError("a gridded model (EFGPND.from_grid) holds no coordinate tensor for the dense sampler: use "
                                      "method='efgp'")
        x = _as2d(self.x)
        xn = _as2d(x_new)
        if hasattr(self.kernel, "ard_kind"):            # a function of the coordinate differences, not of the distance
            km = self.kernel.kernel_matrix
        else:
            k = self.kernel.kernel
            km = lambda a, b: k(torch.cdist(a, b, p=2))
        sig = self.sigmasq.detach()
        K_no = km(xn, x)
        K_oo = km(x, x) + sig * torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
        K_nn = km(xn, xn)
        cov = K_nn - K_no @ torch.linalg.solve(K_oo, K_no.T)
        cov = cov + 1e-10 * torch.eye(xn.shape[0], dtype=xn.dtype, device=xn.device)
        chol = torch.linalg.cholesky(cov)
        Zs = torch.randn(xn.shape[0], nsamples, dtype=x.dtype, device=x.device)
        mean, _ = self.predict(xn, return_variance=False)
        return (mean.unsqueeze(1) + chol @ Zs).detach().cpu().numpy()

    def _compute_log_marginal(self, beta, ws, sigmasq, toeplitz, device, rdtype, n):
        """-(logdet + sum |ws| |beta|^2)/2, the `predict`-path formula of the reference (:1050-1066)."""
        log_det = logdet_slq(ws=ws, sigma2=sigmasq, toeplitz=toeplitz, probes=self.opts.get("log_marginal_probes", 100),
                             steps=self.opts.get("log_marginal_steps", 25), dtype=rdtype, device=device, n=n,
                             probe_vectors=self.opts.get("log_marginal_probe_vectors"))
        data_fit = float((ws.abs() * (beta.abs() ** 2)).sum().real)
        return -0.5 * (log_det + data_fit)

    # -- training loop -------------------------------------------------------------------------------------
    def optimize_hyperparameters(self, *, optimizer="Adam", lr: Optional[float] = 0.1, max_iters: int = 50,
                                 min_lengthscale: float = 5e-3, log_interval: int = 10,
                                 compute_log_marginal: bool = False, verbose: bool = False,
                                 trace_samples: int = 10, **gkwargs):
        """Adam (or a supplied optimizer) on the log-space parameters using `compute_gradients`;
        history is left in ``self.training_log``.  Reference: efgpnd.py:1068-1226."""
        if isinstance(optimizer, str):
            if optimizer.lower() != "adam":
                raise ValueError(f"Unsupported optimizer string: {optimizer}. Currently supporting: 'adam'")
            opt = Adam(self._gp_params.parameters(), lr=lr)
        else:
            opt = optimizer
        hist = {"log_marginal": [], "gradients": [], "mean_cg_iters": [], "trace_cg_iters": []}

        def record():
            for name, value in self.kernel.iter_hypers():
                hist.setdefault(name, []).append(float(self.kernel.get_hyper(name)))
            hist.setdefault("sigmasq", []).append(float(self.sigmasq.detach()))

        record()
        t_start = time.time()
        print(f"Optimizing hyperparameters using {optimizer if isinstance(optimizer, str) else type(optimizer).__name__}")
        for it in range(max_iters):
            record()
            opt.zero_grad()
            want_lm = compute_log_marginal and (it % log_interval == 0 or it == max_iters - 1)
            res = self.compute_gradients(trace_samples=trace_samples, nufft_eps=self.nufft_eps, apply_gradients=True,
                                         compute_log_marginal=want_lm, verbose=verbose, **gkwargs)
            if want_lm:
                grad, lm = res
                hist["log_marginal"].append(float(lm))
            else:
                grad = res
            hist["gradients"].append([float(g) for g in grad])
            hist["mean_cg_iters"].append(self.last_gradient_stats.get("mean_cg_iters"))
            hist["trace_cg_iters"].append(self.last_gradient_stats.get("trace_cg_iters"))
            if verbose:
                print(f"  Iter {it}: Gradients = {hist['gradients'][-1]}")
            opt.step()
            with torch.no_grad():
                try:
                    names = self._gp_params.hypers_names
                    floor = torch.tensor(min_lengthscale, device=self._gp_params.raw.device, dtype=self._gp_params.raw.dtype)
                    for idx in [i for i, nm in enumerate(names) if nm.startswith("lengthscale_")] or [names.index("lengthscale")]:
                        if torch.exp(self._gp_params.raw[idx]) < floor:
                            self._gp_params.raw[idx].copy_(torch.log(floor))
                except (ValueError, IndexError) as e:
                    if verbose:
                        print(f"Note: Could not apply lengthscale constraint: {e}")
            if it % log_interval == 0 or it == max_iters - 1:
                parts = [f"iter {it}/{max_iters}"]
                for name, values in hist.items():
                    if not values or name == "gradients" or (name == "log_marginal" and not compute_log_marginal):
                        continue
                    if values[-1] is not None:
                        parts.append(f"{name}={values[-1]:.6g}")
                print(", ".join(parts))
        self._fitted = False
        self._cached_params = {}
        self._compute_common_parameters(force_recompute=True)
        print(f"Optimization complete after {time.time() - t_start:.2f} seconds")
        print("\nFinal hyperparameters:")
        for name, _ in self.kernel.iter_hypers():
            print(f"{name} = {float(self.kernel.get_hyper(name)):.6g}")
        print(f"sigmasq = {float(self.sigmasq.detach()):.6g}")
        self.training_log = hist
        return self


# ======================================================================================
# legacy functional entry point (signature from efgpnd_variance_shootout.py:129-137)
# ======================================================================================
def efgp_nd(x, y, sigmasq, kernel, eps, x_new, nufft_eps=1e-4, opts=None, do_profiling=False):
    """One-shot fit + predict -> (beta, xis, ytrg{'mean','var'[,'log_marginal']}, ws, toeplitz).

    ``opts``: cg_tolerance, early_stopping (ignored: the mean solve always stops early, as in the
    reference), estimate_variance, variance_method, hutchinson_probes, max_cg_iter, compute_log_marginal."""
    opts = dict(opts or {})
    mopts = {"cg_tolerance": opts.get("cg_tolerance", 1e-4), "mean_cg_warm_start": False}
    if "max_cg_iter" in opts:
        mopts["max_cg_iterations"] = opts["max_cg_iter"]
    model = EFGPND(_as2d(x), y, kernel, sigmasq=float(sigmasq), eps=eps, nufft_eps=nufft_eps, opts=mopts,
                   estimate_params=False)
    want_var = bool(opts.get("estimate_variance", False))
    res = model.predict(_as2d(x_new), return_variance=want_var,
                        variance_method=opts.get("variance_method", "stochastic"),
                        hutchinson_probes=opts.get("hutchinson_probes", 1000),
                        compute_log_marginal=bool(opts.get("compute_log_marginal", False)), do_profiling=do_profiling)
    ytrg = {"mean": res[0], "var": res[1]}
    if len(res) > 2:
        ytrg["log_marginal"] = res[2]
    return model._beta, model._xis, ytrg, model._ws, model._toeplitz
