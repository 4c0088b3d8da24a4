"""EFGPNDMulti: B outputs observed at the SAME points under one kernel and one noise level, fitted in one batched pass.

Everything that depends on the points only -- the point layout and the NUFFT plan, the Toeplitz vector and operator, the spectral
weights and the Jacobi diagonal, the predictive variance, the trace term of the hyper-gradient, the SLQ log-determinant -- is
computed once; everything that depends on the data is a row of a batched call of libefgp_hip: `efgp_nufft_type1` with B real rows,
the Hermitian CG with B systems (one workgroup each on the single-launch grids: B compute units instead of one),
`efgp_nufft_type2_scaled` / `efgp_raster_type2` with B rows, and `efgp_gradient_assemble_multi` for the data terms of the joint
gradient.  The model is the sum of B independent single-output models with shared hyper-parameters: its objective is the sum of
their negative log marginal likelihoods.

Rows are stored in units of an exact power of two each (`2^e_b`, e_b the frexp exponent of max|y_b|): the type-1 transform pairs
real rows two per complex grid, so the smaller row of a pair inherits 1e-16 times the magnitude ratio, and the CG kernels guard
<r, z> with an absolute 1e-16 (efgpnd.py, `_compute_common_parameters`).  Coefficients, means and the data terms are scaled back
exactly.

Out of scope: per-output missing data or noise levels, gridded and sharded multi-output models, function draws.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from efgp_hip import NufftPlan, cg_solve_lazy, compute_device, gradient_assemble_multi, raster_type2, raster_type2_jet
from efgpnd import (EFGPND, ToeplitzND, _CONV_TOL, _Grid, _SAMPLE_BLOCK, _dev_points, _jacobi_diag, _kernel_by_name, _points_box,
                    _trace_systems, _variance_hyper, logdet_slq)

TWO_PI = 2.0 * math.pi
_ESTIMATE_COLUMNS = 8          # columns the initial hyper-parameter estimate looks at


class _RowIterations:
    """Per-row iteration counts of a fit's block solves; reading them waits for the solves.  Rows that held no data (an all-zero
    column, solved with a stand-in right-hand side) count 0."""

    def __init__(self, blocks, zero_rows):
        self._blocks, self._zero, self._rows = blocks, zero_rows, None

    @property
    def rows(self):
        if self._rows is None:
            rows = [int(v) for its in self._blocks for v in its.rows]
            self._rows = [0 if z else v for v, z in zip(rows, self._zero)]
        return self._rows

    def __int__(self):
        return max(self.rows)


class EFGPNDMulti(EFGPND):
    """``EFGPNDMulti(x, Y, kernel, sigmasq=None, eps=1e-2, nufft_eps=1e-4, opts=None, estimate_params=True)``: x (N, d), d in
    {1, 2, 3}; Y (N, B), B >= 1, finite.  One kernel object, one noise variance and one `GPParams` for all outputs; `kernel` and
    `opts` as `EFGPND` takes them (built-in and ARD kernels).  Refused: opts["shard_points"], a non-finite entry of Y (per-output
    missing data would break the shared operator), Y that is not 2-D.

    `fit`, `predict` -> (mean (N*, B), variance (N*,)), `predict_grid` -> (mean (B, n_0, ..), variance map), `compute_gradients`
    (gradient of the joint negative log marginal, adjoint estimator), `optimize_hyperparameters`, `register_optimizer` and
    `log_marginal` -> (B,).  The initial hyper-parameter estimate is `kernel.estimate_hyperparameters` on at most 8 columns at a
    fixed stride, combined by the geometric mean."""

    def __init__(self, x, Y, kernel, sigmasq: float = None, eps: float = 1e-2, nufft_eps: float = 1e-4,
                 opts: Optional[Dict] = None, estimate_params: bool = True):
        if opts and opts.get("shard_points", False):
            raise NotImplementedError("EFGPNDMulti does not support opts['shard_points']: the batched rows are transformed and "
                                      "solved on one device")
        if not torch.is_tensor(Y):
            Y = torch.as_tensor(Y)
        if Y.ndim != 2:
            raise ValueError(f"Y must be 2-D, (N, B) with one column per output (got shape {tuple(Y.shape)}); a single output is "
                             "Y[:, None] or an EFGPND model")
        if not Y.is_floating_point():
            Y = Y.to(torch.float64)
        n_pts = x.shape[0]
        if Y.shape[0] != n_pts or Y.shape[1] < 1:
            raise ValueError(f"Y has shape {tuple(Y.shape)}: it needs one row per point of x ({n_pts}) and at least one column")
        if not bool(torch.isfinite(Y).all()):
            raise ValueError("Y has non-finite entries: every output must be observed at every point (per-output missing data "
                             "would break the operator the outputs share)")
        dimension = 1 if x.ndim == 1 else x.shape[1]
        if isinstance(kernel, str):
            kernel = _kernel_by_name(kernel, dimension)
        if estimate_params:
            try:
                ls, var, noise = self._estimate(kernel, x, Y)
                kernel.set_hyper("lengthscale", ls)
                kernel.set_hyper("variance", var)
                if sigmasq is None:
                    sigmasq = noise
            except Exception as e:          # as forgiving as EFGPND
                print(f"Warning: Failed to estimate hyperparameters: {e}")
                if sigmasq is None:
                    sigmasq = 0.1
        super().__init__(x, Y[:, 0], kernel, sigmasq=sigmasq, eps=eps, nufft_eps=nufft_eps, opts=opts, estimate_params=False)
        self.y = Y
        self.Y = Y
        self.n_outputs = int(Y.shape[1])
        self._last_gradient_beta = None
        self._rows_out = None

    @staticmethod
    def _estimate(kernel, x, Y):
        """Geometric mean of kernel.estimate_hyperparameters over at most 8 columns at a fixed stride (columns whose estimate is
        not positive and finite -- a constant column -- are left out)."""
        B = Y.shape[1]
        step = -(-B // _ESTIMATE_COLUMNS)
        logs = []
        for c in range(0, B, step):
            ls, var, noise = kernel.estimate_hyperparameters(x, Y[:, c])
            flat = [float(v) for v in (ls if isinstance(ls, (tuple, list)) else [ls])] + [float(var), float(noise)]
            if all(math.isfinite(v) and v > 0.0 for v in flat):
                logs.append([math.log(v) for v in flat])
        if not logs:
            raise ValueError("no column of Y gives a positive, finite estimate")
        mean = [math.exp(sum(col) / len(logs)) for col in zip(*logs)]
        ls = mean[0] if len(mean) == 3 else tuple(mean[:-2])
        return ls, mean[-2], mean[-1]

    # -- what EFGPND offers and a multi-output model does not ---------------------------------------------------------------------
    @classmethod
    def from_grid(cls, *args, **kwargs):
        raise NotImplementedError("EFGPNDMulti.from_grid: gridded multi-output models are not supported")

    def sample_paths(self, *args, **kwargs):
        raise NotImplementedError("EFGPNDMulti.sample_paths: function draws per output are not supported")

    def sample_paths_grid(self, *args, **kwargs):
        raise NotImplementedError("EFGPNDMulti.sample_paths_grid: function draws per output are not supported")

    def sample_posterior(self, *args, **kwargs):
        raise NotImplementedError("EFGPNDMulti.sample_posterior: function draws per output are not supported")

    # -- device data ----------------------------------------------------------------------------------------------------------------
    def _device_data(self):
        """Points, the (B, N) rows in units of 2^e_b each, the scales and |row|^2, the box: made once per model.  The point layout
        (`EFGPND._layout`) carries no target values: the rows go through `type1`, which takes them in point order."""
        if self._devdata is None:
            dev = compute_device(self.x)
            xd = _dev_points(self.x, dev)
            Yd = self.Y.detach().to(device=dev, dtype=torch.float64)
            amax = Yd.abs().amax(dim=0)                                   # (B,)
            expo = torch.frexp(amax.cpu())[1].clamp(-1021, 1023)          # B numbers, once per model: on the host
            scale = torch.ldexp(torch.ones(expo.shape, dtype=torch.float64), expo).to(dev)      # 2^e_b > max|y_b| (1 for a zero column)
            rows = (Yd / scale[None, :]).T.contiguous()                   # division by a power of two: exact
            L = _points_box(xd, self._shards, hasattr(self.kernel, "ard_kind"))
            zero = (amax == 0)
            self._devdata = dict(dev=dev, x=xd, y=rows, scale=scale.contiguous(), yy=(rows * rows).sum(dim=1).contiguous(), L=L,
                                 N=xd.shape[0], points=None, passes=0, layout_values=None, zero=zero,
                                 zero_host=[bool(z) for z in zero.tolist()])
        return self._devdata

    # -- the batched pieces -----------------------------------------------------------------------------------------------------------
    def _shared_operator(self, grid, sig, nufft_eps, want_diag, probe_plan=False):
        """What depends on x only, once for all outputs: the plan at the Toeplitz vector's tolerance (and, with probe_plan, the one
        at nufft_eps for the trace probes when that is looser), the Toeplitz vector from a ones-only pass, the operator and the
        Jacobi diagonal.  Counts as a pass over the points (`_layout`).  -> (plan, plan_p, v, toeplitz, diag)"""
        xd = self._device_data()["x"]
        tight = min(float(nufft_eps), _CONV_TOL) if nufft_eps else _CONV_TOL
        points = self._layout()
        plan = plan_p = NufftPlan(xd, grid.plan_h, tight, points=points)
        if probe_plan and nufft_eps and float(nufft_eps) > tight:
            plan_p = NufftPlan(xd, grid.plan_h, float(nufft_eps), points=points)
        v = plan.type1_ones(tuple(2 * n - 1 for n in grid.shape))
        toeplitz = ToeplitzND(v, force_pow2=True)
        return plan, plan_p, v, toeplitz, _jacobi_diag(grid.ws, v, sig) if want_diag else None

    def _solve_rows(self, plan, grid, top, diag, sig, tol, warm_rows):
        """F* of every row and the B mean systems, `_SAMPLE_BLOCK` rows at a time (a pass holds a complex fine grid per two rows and
        the CG vectors of every row).  -> (FY (B, M), beta (B, M), list of the blocks' LazyIterations); rows in their own units."""
        dd = self._device_data()
        rows, zero = dd["y"], dd["zero"]
        B, M, ws = rows.shape[0], grid.M, grid.ws
        any_zero = any(dd["zero_host"])
        block = _SAMPLE_BLOCK[grid.d]
        FY = torch.empty((B, M), dtype=torch.complex128, device=dd["dev"])
        beta = torch.empty((B, M), dtype=torch.complex128, device=dd["dev"])
        its_all = []
        for r0 in range(0, B, block):
            r1 = min(B, r0 + block)
            FY[r0:r1] = plan.type1(rows[r0:r1], grid.shape).reshape(r1 - r0, M)
            rhs = ws[None, :] * FY[r0:r1]                                  # D F* y_b for the block
            if any_zero:
                # a right-hand side of zeros has no relative residual: such a row is solved for D 1 instead and set to zero after
                rhs = torch.where(zero[r0:r1, None], ws[None, :], rhs)
            b0 = warm_rows[r0:r1] if warm_rows is not None else None
            x, its = cg_solve_lazy(top, ws, sig, 0, rhs, b0, tol, early_stop=True, diag=diag, batched=True, hermitian=True)
            its.settle()                       # the rows a dead grid barrier left are solved again, as in efgpnd._solve_batched
            beta[r0:r1] = x.reshape(r1 - r0, M)
            its_all.append(its)
        if any_zero:
            beta = torch.where(zero[:, None], torch.zeros((), dtype=beta.dtype, device=beta.device), beta)
        return FY, beta, its_all

    # -- fit ------------------------------------------------------------------------------------------------------------------------
    def _compute_common_parameters(self, force_recompute: bool = False, nufft_eps: Optional[float] = None) -> None:
        """Fit: grid, one ones-only pass over the points for the Toeplitz vector, one batched real-row type 1 for F*Y, one operator,
        one Jacobi diagonal, one batched Hermitian solve (warm-started from the previous rows when opts["mean_cg_warm_start"])."""
        self._update_param_cache()
        if self._fitted and not force_recompute and not self._params_changed():
            return
        if nufft_eps is None:
            nufft_eps = self.nufft_eps
        dd = self._device_data()
        d = dd["x"].shape[1]
        sig = self._gp_params.host_pos()[-1]
        grid = _Grid(self.kernel, self.eps, dd["L"], d, dd["dev"])
        plan, _, v, toeplitz, diag = self._shared_operator(grid, sig, nufft_eps, self.opts.get("mean_cg_preconditioner", True))
        tol = self.opts.get("cg_tolerance", 1e-4)
        prev = self._fit_state
        warm = (self.opts.get("mean_cg_warm_start", True) and prev is not None and tuple(prev["shape"]) == tuple(grid.shape)
                and tuple(prev["beta_rows"].shape) == (self.n_outputs, grid.M))
        FY, beta, its = self._solve_rows(plan, grid, toeplitz._op, diag, sig, tol, prev["beta_rows"] if warm else None)
        rdtype = self.x.dtype
        self._beta = beta * dd["scale"][:, None]          # (B, M) in the units of Y: times a power of two, exact
        self._xis = (grid, rdtype)
        self._ws = grid.ws
        self._toeplitz = toeplitz
        self._fit_state = dict(h=grid.h, mtot=grid.mtot, d=d, sig=sig, ws=grid.ws, beta=self._beta, beta_rows=beta, Fy=FY, v=v,
                               hypers=self._current_hypers(), shape=grid.shape, hs=grid.hs, plan_h=grid.plan_h, ard=grid.ard)
        stats = dict(mean_cg_iters=_RowIterations(its, dd["zero_host"]), feature_count=grid.M, n_outputs=self.n_outputs,
                     row_block=_SAMPLE_BLOCK[d], mean_cg_warm_start_used=bool(warm), hs=grid.hs, shape=grid.shape)
        if not grid.ard:
            stats.update(mtot=grid.mtot, h=grid.h)
        self._last_fit_stats = stats
        self._rows_out = None
        self._fitted = True
        self._update_param_cache()

    @property
    def last_fit_stats(self) -> Dict:
        """Diagnostics of the last fit: the shared grid numbers, and `mean_cg_iters` as the list of per-row iteration counts
        (reading them waits for the solves)."""
        st = dict(self._last_fit_stats)
        if "mean_cg_iters" in st:
            st["mean_cg_iters"] = list(st["mean_cg_iters"].rows)
        return st

    # -- predict --------------------------------------------------------------------------------------------------------------------
    # `predict` -> (means (N*, B), latent variance (N*,)) and `predict_grid` -> (means (B, n_0, .., n_{d-1}), variance map) are
    # EFGPND's: the variance does not depend on Y and is computed once.  What differs is how the means are formed, and that
    # predict(compute_log_marginal=True) appends `log_marginal()` (B,) with opts["log_marginal_probes"] / ["log_marginal_steps"].
    def _row_blocks(self):
        block = _SAMPLE_BLOCK[self._fit_state["d"]]
        return [(r0, min(self.n_outputs, r0 + block)) for r0 in range(0, self.n_outputs, block)]

    def _mean_at(self, plan):
        st, dd = self._fit_state, self._devdata
        mean = torch.empty((self.n_outputs, plan.npts), dtype=torch.float64, device=dd["dev"])
        for r0, r1 in self._row_blocks():                    # F (ws * beta_b), a block of rows per gather
            mean[r0:r1] = plan.type2(st["beta_rows"][r0:r1], st["shape"], real_only=True, batched=True, mode_scale=st["ws"])
        return (mean * dd["scale"][:, None]).T

    def _mean_on_raster(self, ax):
        st, dd = self._fit_state, self._devdata
        n_axis = tuple(int(a.numel()) for a in ax)
        mean = torch.empty((self.n_outputs,) + n_axis, dtype=torch.float64, device=dd["dev"])
        for r0, r1 in self._row_blocks():                    # the batched exact raster transform
            raster_type2(ax, st["plan_h"], st["shape"], st["beta_rows"][r0:r1], batched=True, mode_scale=st["ws"], out=mean[r0:r1])
        return mean * dd["scale"].reshape((-1,) + (1,) * len(n_axis))

    # `predict_gradient` -> (grad (N*, B, d), variance of the partials (N*, d)) and `predict_gradient_grid` -> (grad (B, d, n_0, ..),
    # variance (d, n_0, ..)) are EFGPND's as well; return_mean=True prepends the means (N*, B) / (B, n_0, ..) of the same pass.
    def _jet_at(self, plan):
        st, dd = self._fit_state, self._devdata
        d = st["d"]
        jet = torch.empty((self.n_outputs, 1 + d, plan.npts), dtype=torch.float64, device=dd["dev"])
        for r0, r1 in self._row_blocks():                    # value and partials of F (ws * beta_b), a block of outputs per call
            jet[r0:r1] = plan.type2_jet(st["beta_rows"][r0:r1], st["shape"], mode_scale=st["ws"])
        jet = jet * dd["scale"][:, None, None]
        return jet[:, 0].T, jet[:, 1:].permute(2, 0, 1)

    def _jet_on_raster(self, ax):
        st, dd = self._fit_state, self._devdata
        jet = torch.cat([raster_type2_jet(ax, st["plan_h"], st["shape"], st["beta_rows"][r0:r1], mode_scale=st["ws"])
                         for r0, r1 in self._row_blocks()])
        jet = jet * dd["scale"].reshape((-1,) + (1,) * (jet.ndim - 1))
        return jet[:, 0], jet[:, 1:]

    def _predict_log_marginal(self):
        return self.log_marginal(self.opts.get("log_marginal_probes", 100), self.opts.get("log_marginal_steps", 25))

    # -- objective --------------------------------------------------------------------------------------------------------------------
    def log_marginal(self, probes: int = 100, steps: int = 25) -> torch.Tensor:
        """(B,) log marginal likelihoods at the current hyper-parameters: -(y_b . alpha_b + log det(K + sigma^2 I) + N log 2 pi) / 2
        with the data terms of the fit's rows (efgp_gradient_assemble_multi, `rows_out`) and ONE stochastic-Lanczos log-determinant
        (`logdet_slq`; its probes come from torch's generator, or opts["log_marginal_probe_vectors"])."""
        self._compute_common_parameters()
        st, dd = self._fit_state, self._devdata
        if self._rows_out is None:
            tg = self._toeplitz._op.apply_scaled(st["beta_rows"], pre=st["ws"])
            _, self._rows_out = gradient_assemble_multi(st["Fy"], tg, st["ws"], st["beta_rows"], None, None, None, None,
                                                        variance_idx=None, trace_idx=[], sigmasq=st["sig"], n_obs=dd["N"], yy=dd["yy"],
                                                        row_scale=dd["scale"], variance=1.0)
        det = logdet_slq(st["ws"], st["sig"], self._toeplitz, probes=probes, steps=steps, dtype=torch.float64, device=dd["dev"],
                         n=dd["N"], probe_vectors=self.opts.get("log_marginal_probe_vectors"))
        lm = -0.5 * self._rows_out[:, 2] - 0.5 * det - 0.5 * dd["N"] * math.log(TWO_PI)
        return lm.to(device=self.device, dtype=self.x.dtype)

    # -- gradient -------------------------------------------------------------------------------------------------------------------
    def compute_gradients(self, *, trace_samples: int = 10, do_profiling: bool = False, nufft_eps: Optional[float] = None,
                          cg_tol: Optional[float] = None, noise_floor: Optional[float] = None, apply_gradients: bool = True,
                          compute_log_marginal: bool = False, log_marginal_probes: int = 100, log_marginal_steps: int = 25,
                          verbose: bool = False, **kwargs):
        """Gradient of the JOINT negative log marginal likelihood (the sum over outputs) w.r.t. the log-space parameters (kernel
        hypers..., sigma^2), adjoint estimator; written to ``self._gp_params.raw.grad`` when apply_gradients.  The probes, their
        transforms and the (n_trace + 1) T trace solves run once and their terms count B times; the two probe seeds are drawn
        from torch's global generator as `efgpnd_gradient_batched` draws them (`torch.manual_seed` makes the step comparable
        with single-output steps).  compute_log_marginal=True also returns the joint log marginal, the sum of `log_marginal`'s."""
        if kwargs.get("trace_mode", "adjoint") != "adjoint" or kwargs.get("pointwise_alpha", False):
            raise NotImplementedError("EFGPNDMulti supports the adjoint gradient estimator only")
        unknown = set(kwargs) - {"trace_mode", "pointwise_alpha"}
        if unknown:
            raise TypeError(f"EFGPNDMulti.compute_gradients: unexpected arguments {sorted(unknown)}")
        self._update_param_cache()
        if nufft_eps is None:
            nufft_eps = self.eps * 0.1
        if noise_floor is None:
            noise_floor = self.opts.get("noise_floor")
        if cg_tol is None:
            cg_tol = 0.1 * self.eps
        dd = self._device_data()
        dev, N = dd["dev"], dd["N"]
        kernel = self.kernel
        sig = self._gp_params.host_pos()[-1]
        if noise_floor is not None:
            sig = max(sig, float(noise_floor))
        hypers = list(getattr(kernel, "hypers", []))
        variance_idx = hypers.index("variance") if "variance" in hypers else None
        H = kernel.num_hypers - 1
        trace_idx = [i for i in range(H) if i != variance_idx]
        K, T = len(trace_idx), int(trace_samples)
        grid = _Grid(kernel, self.eps, dd["L"], dd["x"].shape[1], dev, want_grad=True)
        ws, Dp, M = grid.ws, grid.dprime, grid.M
        if H > 4 or Dp is None or Dp.ndim != 2 or Dp.shape[1] != H:
            raise NotImplementedError("EFGPNDMulti.compute_gradients needs a kernel with at most 4 hyper-parameters and a spectral_grad")
        use_mean_pc = self.opts.get("mean_cg_preconditioner", True)
        use_trace_pc = self.opts.get("trace_cg_preconditioner", True)
        plan, plan_p, _, toeplitz, diag = self._shared_operator(grid, sig, nufft_eps, use_mean_pc or use_trace_pc, probe_plan=True)
        top = toeplitz._op
        prev = self._last_gradient_beta
        warm = (self.opts.get("mean_cg_warm_start", True) and prev is not None and tuple(prev.shape) == (self.n_outputs, M)
                and getattr(self, "_last_gradient_shape", None) == tuple(grid.shape))
        FY, beta, mean_its = self._solve_rows(plan, grid, top, diag if use_mean_pc else None, sig, cg_tol, prev if warm else None)
        Tg = top.apply_scaled(beta, pre=ws)                                # T (D beta_b), every row in one call

        # probes, the right-hand sides of the trace systems and their solve: once for all outputs, on generated probes
        FZ, V, Beta_all, trace_iters = _trace_systems(grid, top, plan_p, sig, cg_tol, True, diag if use_trace_pc else None, T, trace_idx,
                                                      self._shards, N, dev)
        out, rows_out = gradient_assemble_multi(FY, Tg, ws, beta, Dp, FZ, V, Beta_all.reshape(-1, M), variance_idx=variance_idx,
                                                trace_idx=trace_idx, sigmasq=sig, n_obs=N, yy=dd["yy"], row_scale=dd["scale"],
                                                variance=_variance_hyper(kernel, variance_idx))
        nh = H + 1
        host = out.cpu()                                                   # ONE read-back: gradient and diagnostics
        self._last_gradient_beta = beta
        self._last_gradient_shape = tuple(grid.shape)
        self._last_gradient_stats = dict(
            mean_cg_iters=int(_RowIterations(mean_its, dd["zero_host"])), trace_cg_iters=trace_iters, trace_num_rhs=(K + 1) * T,
            feature_count=M, shape=tuple(grid.shape), hs=tuple(grid.hs), trace_samples=T, n_outputs=self.n_outputs,
            mean_cg_warm_start_used=bool(warm), term1=host[nh:2 * nh].clone(), term2=host[2 * nh:3 * nh].clone(), rows=rows_out,
            **({} if grid.ard else {"mtot": grid.mtot}))
        raw = self._gp_params.raw
        raw_grad = host[:nh].to(device=raw.device, dtype=raw.dtype) * raw.detach().exp()         # chain rule d/dlog
        if apply_gradients:
            with torch.no_grad():
                raw.grad = raw_grad.detach().clone()
        if not compute_log_marginal:
            return raw_grad
        det = logdet_slq(ws, sig, top, probes=log_marginal_probes, steps=log_marginal_steps, dtype=torch.float64, device=dev, n=N,
                         probe_vectors=self.opts.get("log_marginal_probe_vectors"))
        B = self.n_outputs
        lm = -0.5 * float(host[3 * nh]) - 0.5 * B * det - 0.5 * B * N * math.log(TWO_PI)
        return raw_grad, torch.tensor(lm, dtype=self.x.dtype)
