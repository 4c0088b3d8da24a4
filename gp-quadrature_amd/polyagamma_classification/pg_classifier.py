"""Polya-Gamma (PG) augmented GP estimators on the HIP EFGP operators (reference: polyagamma_classification/pg_classifier.py):
`PolyagammaGPClassifier` (Bernoulli likelihood with logistic link) and `PolyagammaGPNegativeBinomialRegressor` (counts,
y ~ NB(r, sigmoid(f)), optionally with a learnt r).  Both share one fit loop; the likelihood enters only through the PG
strength kappa, the PG shape b and the training metric.

Every solve of the model is the weighted feature-space system  (I + D T_w D) u = b,  T_w the Toeplitz operator of
F* diag(w) F for the PG weights w = delta, D = ws (E-step) or the clamped D_s (M-step, mean, prediction).  Here each of
them is ONE batched call of the fused device solver (efgp_cg_solve, variant 1 with sigma^2 = 1), the transforms are the
library's NUFFT plans on a per-fit point layout, and the N-scale pointwise work of the PG update and the M-step's trace
estimator are kernels of their own (efgp_pg_estep_update, efgp_pg_weight_rows, efgp_pg_mstep_terms; csrc/pg_ops.hip); the
negative-binomial E-step pass and the gradient of r are efgp_pg_nb_estep_update and efgp_pg_nb_total_count_grad.
torch carries allocations, the O(M) diagonal products around the solves and the O(#hypers) optimiser state.

Scope: SE kernel, float64, the constructor option predictive_variance_method="exact", a GPU device.  Anything else is refused with
an error that names the option.  The approximate variances are chosen per call on a fitted estimator: `predictive_variance(X,
method=...)` and the `variance_method=` keyword of `predict_response_mean` / `predict_proba` / `predict_mean_count` take "exact",
"stochastic" (alias "stochastic_diag_sums": Hutchinson probes on the mode grid, one cached batched solve, efgp_lag_sums, one
FFT-ordered type 2 per call) and "chebyshev" (the exact variance at n^d Chebyshev-Lobatto nodes of the test box, interpolated by
efgp_cheb_interp; csrc/cheb_interp.hip).  The product path does not import scikit-learn.
"""
from __future__ import annotations

import functools
import inspect
import math
import os
import sys
import warnings

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

__all__ = ["PolyagammaGPClassifier", "PolyagammaGPNegativeBinomialRegressor", "approximate_logistic_gaussian_prob",
           "negative_binomial_gaussian_mean", "_gauss_hermite_normal_rule", "_pg_omega_expectation"]

_SE_NAMES = ("squared_exponential", "se", "rbf")
_EXACT_VARIANCE = "exact"
_UNSUPPORTED_VARIANCE = ("stochastic", "stochastic_diag_sums", "chebyshev")
_VARIANCE_METHODS = ("exact", "stochastic", "stochastic_diag_sums", "chebyshev")      # the per-call keyword of the predictions
_CHEB_MAX_AXIS, _CHEB_MAX_BOX = 64, 4096                                              # efgp_cheb_interp


def approximate_logistic_gaussian_prob(mean: torch.Tensor, variance: torch.Tensor | None = None) -> torch.Tensor:
    """E[sigmoid(f)] for f ~ N(mean, variance) by the probit-style moment approximation
    sigmoid(mean / sqrt(1 + pi variance / 8)) (negative variances count as 0); sigmoid(mean) without a variance."""
    if variance is None:
        return torch.sigmoid(mean)
    scale = torch.sqrt(1.0 + (math.pi / 8.0) * variance.clamp_min(0.0))
    return torch.sigmoid(mean / scale)


def negative_binomial_gaussian_mean(mean: torch.Tensor, variance: torch.Tensor, *, total_count: float) -> torch.Tensor:
    """E[count] = r exp(mean + variance / 2) of y ~ NB(r, sigmoid(f)), f ~ N(mean, variance) (negative variances count as 0)."""
    return total_count * torch.exp(mean + 0.5 * variance.clamp_min(0.0))


@functools.lru_cache(maxsize=None)
def _gauss_hermite_normal_rule(num_nodes: int):
    """(nodes, weights) of the num_nodes-point Gauss-Hermite rule for E[g(X)], X ~ N(0, 1): numpy's hermgauss rule for the
    weight exp(-x^2), nodes scaled by sqrt(2) and weights by 1/sqrt(pi).  Read-only float64 arrays."""
    if num_nodes <= 0:
        raise ValueError("num_nodes must be positive.")
    x, w = np.polynomial.hermite.hermgauss(int(num_nodes))
    nodes, weights = (x * np.sqrt(2.0)).astype(np.float64), (w / np.sqrt(np.pi)).astype(np.float64)
    nodes.flags.writeable = weights.flags.writeable = False
    return nodes, weights


def _pg_omega_expectation(c: torch.Tensor, pg_b: torch.Tensor) -> torch.Tensor:
    """Mean of a PG(b, c) variable, b tanh(c/2) / (2 c), with its limit b / 4 for c <= 1e-8 (c is clamped at 1e-12 first)."""
    c_safe = c.clamp_min(1e-12)
    value = 0.5 * pg_b * torch.tanh(0.5 * c_safe) / c_safe
    return torch.where(c > 1e-8, value, 0.25 * pg_b)


def _sample_rademacher(shape, seed):
    """+-1 probes of the reference's seeded stream (host torch.Generator, float64 uniforms -> floor(2 u) * 2 - 1)."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    u = torch.rand(shape, generator=gen, dtype=torch.float64)
    return u.mul_(2.0).floor_().mul_(2.0).sub_(1.0)


def _check_X_y(X, y):
    X_arr = np.asarray(X, dtype=np.float64)
    if X_arr.ndim != 2:
        raise ValueError(f"X must be a 2-D array (n_samples, n_features), got shape {X_arr.shape}")
    y_arr = np.asarray(y)
    if y_arr.ndim == 2 and y_arr.shape[1] == 1:
        y_arr = y_arr[:, 0]
    if y_arr.ndim != 1 or y_arr.shape[0] != X_arr.shape[0]:
        raise ValueError(f"y must be a 1-D array with one label per row of X, got shape {y_arr.shape} for X {X_arr.shape}")
    if X_arr.shape[0] == 0 or not np.isfinite(X_arr).all():
        raise ValueError("X must be non-empty and finite")
    return np.ascontiguousarray(X_arr), y_arr


def _check_array(X, n_features):
    X_arr = np.asarray(X, dtype=np.float64)
    if X_arr.ndim != 2 or X_arr.shape[1] != n_features:
        raise ValueError(f"X must have shape (n_samples, {n_features}), got {X_arr.shape}")
    return np.ascontiguousarray(X_arr)


class _Spectral:
    """Quadrature grid, weights and NUFFT plan of one hyper-parameter setting (the reference's _SpectralState without the
    unweighted Toeplitz operator, which the PG model never applies)."""

    def __init__(self, kernel, points, xd, L, spectral_eps, trunc_eps, nufft_eps):
        from efgp_hip.ops import NufftPlan
        from efgpnd import _Grid
        d = xd.shape[1]
        self.grid = _Grid(kernel, spectral_eps, L, d, xd.device, want_grad=True, trunc_eps=trunc_eps)
        self.h, self.mtot, self.d = self.grid.h, self.grid.mtot, d
        self.shape = (self.mtot,) * d
        self.conv_shape = (2 * self.mtot - 1,) * d
        self.M = self.grid.M
        self.ws = self.grid.ws                                   # (M,) complex128, imaginary part 0
        self.dprime = self.grid.dprime                           # (M, 2) complex128: h^d (dS/dl, dS/dvariance)
        self.ws2 = self.ws * self.ws
        # the M-step / prediction scaling (pg_classifier.py:452-455): D_s = sqrt(clamp(ws^2, max(mean(ws^2) 1e-14, 1e-14)))
        d2 = self.ws2.real
        floor = max(float(d2.mean()) * 1e-14, 1e-14)
        ds = torch.sqrt(torch.clamp(d2, min=floor))
        self.ds = ds.to(torch.complex128)
        self.ds_inv = 1.0 / ds
        self.ws2_over_ds = self.ws2 / self.ds
        # NUFFT centre 0, as the reference (pg_classifier.py:347-354); the spreader folds the phases itself
        self.plan = NufftPlan(xd, self.h, nufft_eps, xcen=None, points=points)


class _BasePolyagammaGPEstimator:
    """The fit loop, solves and prediction shared by the PG estimators (the reference's _BasePolyagammaGPEstimator).  A
    subclass supplies the likelihood: `_prepare_targets` (checks, model targets), `_start_likelihood` (kappa, optimiser state),
    `_initial_delta`, `_estep_pass` (the N-scale E-step kernel and its metric), `_refresh_likelihood` / `_step_auxiliary` /
    `_final_record` (parameters of the likelihood learnt alongside the kernel's) and `_response_mean`."""

    _what = "the PG estimator"          # how option errors name the estimator
    _history_key = _history_label = _training_attr = None

    def __init__(self, *, kernel: str = "squared_exponential", lengthscale_init: float = 0.3, variance_init: float = 1.0,
                 max_iter: int = 50, e_step_iters: int = 1, final_e_step_iters: int = 1, e_step_tol: float = 1e-4, rho0: float = 0.7,
                 gamma: float = 1e-3, lr: float = 0.05, n_e_probes: int = 10, n_m_probes: int = 10, cg_tol: float = 1e-6,
                 nufft_eps: float = 1e-7, spectral_eps: float = 1e-4, trunc_eps: float = 1e-4, jitter: float = 1e-8,
                 use_exact_weighted_toeplitz_operator: bool = True, reuse_e_probes: bool = True,
                 prediction_batch_size: int | None = 64, predictive_variance_method: str = "exact",
                 predictive_variance_probes: int = 16, predictive_variance_chebyshev_nodes: int = 7, warm_start: bool = False,
                 random_state: int | None = None, device: str = "auto", dtype="float64", verbose: int = 0,
                 store_history: bool = False):
        self.kernel = kernel
        self.lengthscale_init = lengthscale_init
        self.variance_init = variance_init
        self.max_iter = max_iter
        self.e_step_iters = e_step_iters
        self.final_e_step_iters = final_e_step_iters
        self.e_step_tol = e_step_tol
        self.rho0 = rho0
        self.gamma = gamma
        self.lr = lr
        self.n_e_probes = n_e_probes
        self.n_m_probes = n_m_probes
        self.cg_tol = cg_tol
        self.nufft_eps = nufft_eps
        self.spectral_eps = spectral_eps
        self.trunc_eps = trunc_eps
        self.jitter = jitter
        self.use_exact_weighted_toeplitz_operator = use_exact_weighted_toeplitz_operator
        self.reuse_e_probes = reuse_e_probes
        self.prediction_batch_size = prediction_batch_size
        self.predictive_variance_method = predictive_variance_method
        self.predictive_variance_probes = predictive_variance_probes
        self.predictive_variance_chebyshev_nodes = predictive_variance_chebyshev_nodes
        self.warm_start = warm_start
        self.random_state = random_state
        self.device = device
        self.dtype = dtype
        self.verbose = verbose
        self.store_history = store_history

    # -- estimator protocol (duck-typed: no scikit-learn import) ---------------------------------------------------------------
    @classmethod
    def _param_names(cls):
        return [p.name for p in inspect.signature(cls.__init__).parameters.values() if p.kind == p.KEYWORD_ONLY]

    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._param_names()}

    def set_params(self, **params):
        valid = set(self._param_names())
        for key, value in params.items():
            if key not in valid:
                raise ValueError(f"invalid parameter {key!r} for {type(self).__name__}")
            setattr(self, key, value)
        return self

    # -- option checks ---------------------------------------------------------------------------------------------------
    def _validate_options(self):
        if str(self.kernel).lower() not in _SE_NAMES:
            raise ValueError(f"kernel={self.kernel!r}: only the squared exponential kernel is supported in v1 "
                             f"({', '.join(_SE_NAMES)})")
        dt = self.dtype
        if not (dt == "float64" or dt is torch.float64):
            raise ValueError(f"dtype={dt!r} is not supported: {self._what} runs in float64 only")
        method = str(self.predictive_variance_method).lower()
        if method in _UNSUPPORTED_VARIANCE:
            raise NotImplementedError(f"predictive_variance_method={self.predictive_variance_method!r} is not implemented; "
                                      "use 'exact'")
        if method != _EXACT_VARIANCE:
            raise ValueError(f"predictive_variance_method={self.predictive_variance_method!r}: must be one of "
                             "{'exact', 'stochastic', 'stochastic_diag_sums', 'chebyshev'}")
        dev = str(self.device)
        if dev == "cpu" or dev.startswith("cpu:"):
            raise ValueError(f"device={self.device!r} is not supported: {self._what} runs on the GPU only (HIP kernels, "
                             "no CPU path)")
        if dev != "auto" and not dev.startswith("cuda"):
            raise ValueError(f"device={self.device!r}: use 'auto', 'cuda' or 'cuda:<index>'")
        if self.n_e_probes < 0 or self.n_m_probes < 0:
            raise ValueError("n_e_probes and n_m_probes must be >= 0")

    def _resolve_device(self):
        from efgp_hip.ops import compute_device
        return compute_device(device=None if self.device == "auto" else self.device)

    # -- device plumbing ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _draw_seed():
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())

    def _feature_rows(self, spec, kappa_rows, kappa_first, probes, seed, J):
        """F* of [kappa; z_1..z_J] (kappa_first) or [z_1..z_J; kappa] -> (J + 1, M) complex.  `kappa_rows` is the (J + 1, N)
        buffer with kappa in its slot and the uploaded probes in the others (seeded mode) -- or None: device-hash probes."""
        from efgp_hip.lib import check, lib
        from efgp_hip.ops import _i64, _on, _ptr, _stream
        if probes is not None or J == 0:
            return spec.plan.type1(kappa_rows, spec.shape).reshape(J + 1, spec.M)
        dev = self._dev
        out = torch.empty((J + 1, spec.M), dtype=torch.complex128, device=dev)
        k_out = out[0] if kappa_first else out[J]
        z_out = out[1:] if kappa_first else out[:J]
        with _on(dev):
            check(lib().efgp_nufft_type1(spec.plan._h, _ptr(self._kappa), 0, 1, _i64(spec.shape), -1, 0, _ptr(k_out),
                                         _stream(dev)), "efgp_nufft_type1")
            check(lib().efgp_nufft_type1_rademacher(spec.plan._h, int(seed) & (2 ** 64 - 1), 0, J, _i64(spec.shape), 0, _ptr(z_out),
                                                    _stream(dev)), "efgp_nufft_type1_rademacher")
        return out

    def _weighted_operator(self, spec, delta):
        """Toeplitz operator of F* diag(delta) F: v = F*(delta) on the (2 mtot - 1)^d box (pg_classifier.py:377-384)."""
        from efgp_hip.ops import ToeplitzOp
        return ToeplitzOp(spec.plan.type1(delta, spec.conv_shape), force_pow2=True)

    def _solve(self, op, diag, rhs, batched, step, outer):
        """(I + diag T diag) u = rhs in the fused device solver, from zero (cg.py semantics of a 2-D / 1-D rhs)."""
        from efgp_hip.ops import cg_solve
        x, iters, rows = cg_solve(op, diag, 1.0, 1, rhs, None, self.cg_tol, max_iter=2000, early_stop=True, batched=batched)
        self.last_fit_stats["solves"].append({"step": step, "outer": outer, "entry": "efgp_cg_solve", "fused": True,
                                              "cg_iters": int(iters), "rows": list(rows)})
        return x, int(iters)

    # -- E-step (pg_classifier.py:507-582) ----------------------------------------------------------------------------------
    def _estep(self, spec, max_iters, seed, outer):
        J = int(self.n_e_probes)
        N = self._N
        op = self._weighted_operator(spec, self._delta)
        residual, metric, cg_iters = float("inf"), float("nan"), 0
        probes, pseed = None, 0
        for it in range(int(max_iters)):
            if J > 0 and (it == 0 or not self.reuse_e_probes):
                if seed is not None:
                    self._zbuf_e[1:].copy_(_sample_rademacher((J, N), seed + 17 * (it + 1)))
                    probes = self._zbuf_e[1:]
                else:
                    pseed = self._draw_seed()
            fz = self._feature_rows(spec, self._zbuf_e, True, probes if seed is not None else None, pseed, J)
            x, cg_iters = self._solve(op, spec.ws, fz * spec.ws, True, "estep", outer)
            S = spec.plan.type2(x, spec.shape, real_only=True, mode_scale=spec.ws, batched=True)
            rho = self.rho0 / (1.0 + self.gamma * it)
            self._mean, self._sigma_diag, residual, metric = self._estep_pass(S, rho, probes, pseed)
            if self.verbose > 1:
                print(f"E-step it {it:3d} rho={rho:.3f} max|Delta-Lambda|={residual:.3e} {self._history_label}={metric:.4f}")
            if residual < self.e_step_tol:
                break
        return {"residual": residual, "metric": metric, "cg_iters": float(cg_iters)}

    # -- M-step gradient (pg_classifier.py:585-631) ---------------------------------------------------------------------------
    def _mstep(self, spec, seed, outer):
        from efgp_hip.ops import pg_mstep_terms, pg_weight_rows
        J = int(self.n_m_probes)
        op = self._weighted_operator(spec, self._delta)
        probes, pseed = None, 0
        if J > 0:
            if seed is not None:
                self._zbuf_m[:J].copy_(_sample_rademacher((J, self._N), seed + 10_000))
                probes = self._zbuf_m[:J]
            else:
                pseed = self._draw_seed()
        Q = self._feature_rows(spec, self._zbuf_m, False, probes if seed is not None else None, pseed, J)
        y, cg_iters = self._solve(op, spec.ds, Q * spec.ds, True, "mstep", outer)
        beta = y * spec.ds_inv
        if J > 0:
            W = pg_weight_rows(self._delta, J, probes=probes, seed=pseed)
            R = spec.plan.type1(W, spec.shape).reshape(J, spec.M)
            out = pg_mstep_terms(beta[J], beta[:J], R, spec.dprime)
        else:
            out = pg_mstep_terms(beta[J], None, None, spec.dprime)
        P = spec.dprime.shape[1]
        return {"grad": out[2 * P:3 * P], "term1": out[:P], "term2": out[P:2 * P], "beta_mean": beta[J], "cg_iters": cg_iters}

    # -- fit (pg_classifier.py:1254-1433) --------------------------------------------------------------------------------------
    def fit(self, X, y):
        X_arr, y_arr = _check_X_y(X, y)
        values, metadata = self._prepare_targets(y_arr)
        self._validate_options()
        from efgp_hip.ops import PointSet
        from kernels.squared_exponential import SquaredExponential

        dev = self._resolve_device()
        self._dev = dev
        for key, value in metadata.items():
            setattr(self, key, value)
        self.n_features_in_ = X_arr.shape[1]
        self._X_train_np_ = X_arr.copy()
        N, d = X_arr.shape
        self._N = N
        self.last_fit_stats = {"solves": []}
        self._variance_sums_cache = self._last_variance_stats = None     # the stochastic variance's lag sums belong to one fit

        xd = torch.as_tensor(X_arr).to(dev).contiguous()
        targets = torch.as_tensor(values).to(dev).contiguous()
        self._xd, self._targets = xd, targets
        self._start_likelihood(targets)                                 # self._kappa, and the likelihood's own state
        self._points = PointSet(xd)
        lo, hi = self._points.bounds()
        L = max(h_ - l_ for l_, h_ in zip(lo, hi))
        # (J + 1, N) strength rows of the type-1 passes: kappa in row 0 (E-step) / row J (M-step), probes uploaded into the rest
        Je, Jm = int(self.n_e_probes), int(self.n_m_probes)
        self._zbuf_e = torch.empty((Je + 1, N), dtype=torch.float64, device=dev)
        self._zbuf_e[0].copy_(self._kappa)
        self._zbuf_m = torch.empty((Jm + 1, N), dtype=torch.float64, device=dev)
        self._zbuf_m[Jm].copy_(self._kappa)

        keep = self.warm_start and getattr(self, "_delta", None) is not None and self._delta.numel() == N \
            and getattr(self, "kernel_", None) is not None and self._delta.device == dev
        if not keep:
            self.kernel_ = SquaredExponential(dimension=d, init_lengthscale=self.lengthscale_init, init_variance=self.variance_init)
            self._delta = self._initial_delta(targets)                                  # 0.25 b
        self._mean = self._sigma_diag = None
        kernel = self.kernel_
        raw = kernel._gp_params_ref.raw
        optimizer = torch.optim.Adam(kernel._gp_params_ref.parameters(), lr=self.lr, maximize=True)
        spec_args = (self._points, xd, L, self.spectral_eps, self.trunc_eps, self.nufft_eps)
        rs = self.random_state
        history = []
        mstep = None
        for outer in range(int(self.max_iter)):
            self._refresh_likelihood()
            seed = None if rs is None else int(rs) + 1000 * outer
            spec = _Spectral(kernel, *spec_args)
            est = self._estep(spec, self.e_step_iters, seed, outer)
            mstep = self._mstep(spec, seed, outer)
            g = [float(v) for v in mstep["grad"].tolist()]
            ell, var = kernel.lengthscale, kernel.variance
            raw.grad = torch.stack([torch.tensor(g[0], dtype=torch.float64).to(raw.dtype) * ell,
                                    torch.tensor(g[1], dtype=torch.float64).to(raw.dtype) * var,
                                    torch.tensor(0.0, dtype=raw.dtype)])
            optimizer.step()
            optimizer.zero_grad(set_to_none=True)
            aux = self._step_auxiliary(outer)
            record = {"iter": float(outer), "lengthscale": float(kernel.lengthscale), "variance": float(kernel.variance),
                      "grad_lengthscale": g[0], "grad_variance": g[1], "e_residual": est["residual"], "e_cg_iters": est["cg_iters"],
                      "m_cg_iters": float(mstep["cg_iters"])}
            record.update(aux)
            record[self._history_key] = est["metric"]
            history.append(record)
            if self.verbose:
                print(f"outer {outer:3d} lengthscale={record['lengthscale']:.5f} variance={record['variance']:.5f} "
                      f"grad=({g[0]:+.3e}, {g[1]:+.3e}) {self._history_label}={est['metric']:.4f}")

        self._refresh_likelihood()
        spec = _Spectral(kernel, *spec_args)
        self._spec = spec
        fin = self._estep(spec, self.final_e_step_iters, None if rs is None else int(rs) + 999_999, int(self.max_iter))
        # the mean solve (pg_classifier.py:634-650): a single right-hand side -> cg.py's single-system semantics
        self._op_pred = self._weighted_operator(spec, self._delta)
        q = spec.plan.type1(self._kappa, spec.shape).reshape(-1)
        ysol, beta_iters = self._solve(self._op_pred, spec.ds, q * spec.ds, False, "mean", int(self.max_iter))
        self._beta_mean = (ysol * spec.ds_inv).contiguous()

        self.delta_ = self._delta.detach().cpu().numpy().copy()
        self.posterior_mean_ = self._mean.detach().cpu().numpy()
        self.posterior_var_diag_ = self._sigma_diag.detach().cpu().numpy()
        self.lengthscale_ = float(kernel.lengthscale)
        self.variance_ = float(kernel.variance)
        self.n_iter_ = self.max_iter
        self.training_metric_ = fin["metric"]
        setattr(self, self._training_attr, fin["metric"])
        self.m_step_gradient_ = mstep["grad"].detach().cpu().numpy() if mstep is not None else np.zeros(2)
        self.beta_mean_ = self._beta_mean.detach().cpu().numpy()
        self.history_ = history if self.store_history else []
        self.history_.append({"iter": float(self.max_iter), "lengthscale": self.lengthscale_, "variance": self.variance_,
                              "grad_lengthscale": float(self.m_step_gradient_[0]), "grad_variance": float(self.m_step_gradient_[1]),
                              "e_residual": fin["residual"], "e_cg_iters": fin["cg_iters"], "m_cg_iters": float(beta_iters)})
        self.history_[-1].update(self._final_record())
        self.history_[-1][self._history_key] = fin["metric"]
        return self

    # -- prediction (pg_classifier.py:653-739, 1442-1508) -----------------------------------------------------------------------
    def _check_fitted(self):
        if getattr(self, "_beta_mean", None) is None:
            raise RuntimeError(f"This {type(self).__name__} instance is not fitted yet: call fit(X, y) first")

    def _is_training_input(self, X_arr):
        return X_arr.shape == self._X_train_np_.shape and np.allclose(X_arr, self._X_train_np_)

    def _latent_mean(self, xn):
        from efgp_hip.ops import NufftPlan
        spec = self._spec
        plan = NufftPlan(xn, spec.h, self.nufft_eps)
        return plan.type2(self._beta_mean, spec.shape, real_only=True, mode_scale=spec.ws2)

    def _latent_variance(self, xn):
        """Exact variance: rhs = D_s conj(f(x*)) (efgp_variance_rhs) -> batched solve -> Re sum_k f_k (ws^2 / D_s)_k u_k
        (efgp_variance_contract), in blocks of prediction_batch_size points."""
        from efgp_hip.ops import cg_solve, variance_contract, variance_rhs
        spec = self._spec
        n = xn.shape[0]
        if n == 0:
            return torch.empty(0, dtype=torch.float64, device=xn.device)
        bs = n if self.prediction_batch_size is None else max(1, min(int(self.prediction_batch_size), n))
        parts = []
        for lo in range(0, n, bs):
            xb = xn[lo:lo + bs]
            rhs = variance_rhs(xb, spec.h, spec.mtot, spec.ds)
            u, _, _ = cg_solve(self._op_pred, spec.ds, 1.0, 1, rhs, None, self.cg_tol, max_iter=2000, early_stop=True, batched=True)
            parts.append(variance_contract(xb, spec.h, spec.mtot, spec.ws2_over_ds, u))
        return torch.cat(parts)

    def _device_points(self, X_arr):
        return torch.as_tensor(X_arr).to(self._dev).contiguous()

    def decision_function(self, X):
        """Posterior mean on the training inputs, the predictive latent mean elsewhere."""
        self._check_fitted()
        X_arr = _check_array(X, self.n_features_in_)
        if self._is_training_input(X_arr):
            return self.posterior_mean_.copy()
        return self._latent_mean(self._device_points(X_arr)).cpu().numpy()

    # -- approximate variances, chosen per call (pg_classifier.py:767-1009, 1128-1216) ---------------------------------------------
    @staticmethod
    def _variance_method(method):
        """The per-call keyword -> "exact" | "stochastic" | "chebyshev" (None is "exact", "stochastic_diag_sums" is "stochastic")."""
        if method is None:
            return _EXACT_VARIANCE
        name = str(method).lower()
        if name not in _VARIANCE_METHODS:
            raise ValueError(f"variance method {method!r}: must be one of {', '.join(repr(m) for m in _VARIANCE_METHODS)}")
        return "stochastic" if name == "stochastic_diag_sums" else name

    @property
    def last_variance_stats(self):
        """What the last off-training variance computed: `method`; for "stochastic" `n_probes`, `seed` (the host stream's seed, or
        the drawn device seed with random_state=None), `cached` (the lag sums came from the cache: no solve), `cg_iters` and the
        per-row counts `rows` of the probe solve that made the sums; for "chebyshev" `n_nodes_total`, the per-axis `nodes` and
        the `node_values` they were interpolated from (host arrays, at most 4096 doubles)."""
        return dict(getattr(self, "_last_variance_stats", None) or {})

    def _stochastic_variance_sums(self):
        """Lag sums c[r] = mean_j sum_{k - l = r} gamma_j[k] eta_j[l] of J Rademacher probes eta on the mode grid,
        gamma_j = (ws^2 / D_s) A^-1 D_s eta_j: one batched solve on the fit's operator and efgp_lag_sums, (2 mtot - 1)^d complex
        in FFT order.  With random_state set the probes are the reference's host stream (seed random_state + 2_000_000),
        otherwise device-hash probes of a drawn seed.  Kept under the key (J, seed or None) until the next fit: a later
        prediction does no solve, and with random_state=None the drawn probes stay fixed."""
        from efgp_hip.ops import cg_solve, lag_sums, rademacher_fill
        J = int(self.predictive_variance_probes)
        if J <= 0:
            raise ValueError(f"predictive_variance_probes={self.predictive_variance_probes!r}: must be positive for the stochastic "
                             "predictive variance")
        rs = self.random_state
        key = (J, None if rs is None else int(rs) + 2_000_000)
        cache = getattr(self, "_variance_sums_cache", None)
        if cache is not None and cache["key"] == key:
            return cache, True
        spec, dev = self._spec, self._dev
        if rs is not None:
            seed = key[1]
            eta = _sample_rademacher((J, spec.M), seed).to(dev)
        else:
            seed = self._draw_seed()
            eta = rademacher_fill(dev, seed, J, spec.M)
        # the probes are real, not conjugate-even: the general solver route
        y, iters, rows = cg_solve(self._op_pred, spec.ds, 1.0, 1, spec.ds * eta, None, self.cg_tol, max_iter=2000, early_stop=True,
                                  batched=True)
        gamma = spec.ws2_over_ds * y.reshape(J, spec.M)
        sums = lag_sums(gamma, eta, spec.mtot, spec.d)
        cache = {"key": key, "sums": sums, "seed": int(seed), "n_probes": J, "cg_iters": int(iters), "rows": [int(v) for v in rows]}
        self._variance_sums_cache = cache
        return cache, False

    def _stochastic_variance(self, xn):
        """Re sum_r c[r] exp(2 pi i h r . x*) of the cached lag sums: one FFT-ordered type-2 transform, clamped at 0."""
        from efgp_hip.ops import NufftPlan
        cache, cached = self._stochastic_variance_sums()
        spec = self._spec
        var = NufftPlan(xn, spec.h, self.nufft_eps).type2(cache["sums"], spec.conv_shape, modeord=1, real_only=True)
        self._last_variance_stats = dict(method="stochastic", n_probes=cache["n_probes"], seed=cache["seed"], cached=cached,
                                         cg_iters=cache["cg_iters"], rows=list(cache["rows"]))
        return var.reshape(-1).clamp_min(0.0)

    @staticmethod
    def _chebyshev_axis(lo, hi, n):
        """Ascending Chebyshev-Lobatto nodes mid + half cos(pi k / (n - 1)) of [lo, hi] and their barycentric weights (-1)^k, halved
        at both ends (the reference's common factor 2 / (hi - lo) cancels in the interpolation formula)."""
        k = np.arange(n, dtype=np.float64)
        nodes = 0.5 * (lo + hi) + 0.5 * (hi - lo) * np.cos(np.pi * k / (n - 1))
        weights = (-1.0) ** k
        weights[0] *= 0.5
        weights[-1] *= 0.5
        order = np.argsort(nodes)
        return nodes[order], weights[order]

    def _chebyshev_variance(self, xn):
        """The exact variance at the n^d Chebyshev-Lobatto nodes of the test points' bounding box (`_latent_variance`, in
        prediction_batch_size blocks), interpolated at every test point by efgp_cheb_interp and clamped at 0."""
        from efgp_hip.ops import cheb_interp
        n = int(self.predictive_variance_chebyshev_nodes)
        d = xn.shape[1]
        if n < 2:
            raise ValueError(f"predictive_variance_chebyshev_nodes={self.predictive_variance_chebyshev_nodes!r}: must be at least 2")
        if n > _CHEB_MAX_AXIS or n ** d > _CHEB_MAX_BOX:
            raise ValueError(f"predictive_variance_chebyshev_nodes={n} in {d} dimensions is {n ** d} node solves: at most "
                             f"{_CHEB_MAX_AXIS} nodes per axis and {_CHEB_MAX_BOX} nodes in all are supported")
        lo_t, hi_t = torch.aminmax(xn, dim=0)
        bounds = torch.stack([lo_t, hi_t]).cpu().numpy()
        nodes, weights = [], []
        for a in range(d):
            lo, hi = float(bounds[0, a]), float(bounds[1, a])
            if np.isclose(lo, hi):
                pad = max(abs(lo), 1.0) * 1e-6
                lo, hi = lo - pad, hi + pad
            nd, wt = self._chebyshev_axis(lo, hi, n)
            nodes.append(nd)
            weights.append(wt)
        mesh = np.meshgrid(*nodes, indexing="ij")
        node_points = np.stack([g.reshape(-1) for g in mesh], axis=1)
        node_values = self._latent_variance(self._device_points(node_points))
        out = cheb_interp(nodes, weights, node_values, xn, clamp=True)
        self._last_variance_stats = dict(method="chebyshev", n_nodes_total=int(node_points.shape[0]), nodes=[a.copy() for a in nodes],
                                         node_values=node_values.cpu().numpy().reshape((n,) * d))
        return out

    def _predictive_variance_at(self, xn, method):
        """Device variance at the rows of xn by the normalised method."""
        if xn.shape[0] == 0:
            return torch.empty(0, dtype=torch.float64, device=xn.device)
        if method == "stochastic":
            return self._stochastic_variance(xn)
        if method == "chebyshev":
            return self._chebyshev_variance(xn)
        self._last_variance_stats = dict(method=_EXACT_VARIANCE)
        return self._latent_variance(xn)

    def predictive_variance(self, X, *, method=None):
        """Latent predictive variance at the rows of X.  method None / "exact": one feature-space solve per point;
        "stochastic" (alias "stochastic_diag_sums"): `predictive_variance_probes` Hutchinson probes, solved once per fit and
        cached, then one type-2 transform per call; "chebyshev": the exact variance at `predictive_variance_chebyshev_nodes`^d
        nodes of X's bounding box, interpolated.  Both options are read at call time.  The training inputs return
        `posterior_var_diag_` whatever the method."""
        method = self._variance_method(method)
        self._check_fitted()
        X_arr = _check_array(X, self.n_features_in_)
        if self._is_training_input(X_arr):
            return self.posterior_var_diag_.copy()
        return self._predictive_variance_at(self._device_points(X_arr), method).cpu().numpy()

    def predict_response_mean(self, X, *, variance_method=None):
        method = self._variance_method(variance_method)
        self._check_fitted()
        X_arr = _check_array(X, self.n_features_in_)
        if X_arr.shape[0] == 0:
            return np.empty(0, dtype=np.float64)
        if self._is_training_input(X_arr):
            mean = torch.as_tensor(self.posterior_mean_, dtype=torch.float64)
            variance = torch.as_tensor(self.posterior_var_diag_, dtype=torch.float64)
        else:
            xn = self._device_points(X_arr)
            mean, variance = self._latent_mean(xn), self._predictive_variance_at(xn, method)
        return self._response_mean(mean, variance).cpu().numpy()

    # -- function draws ----------------------------------------------------------------------------------------------------
    @property
    def last_sample_stats(self):
        """Seed, row count and per-row CG iteration counts of the last `sample_latent` call (reading them waits for its solves);
        `cg_capped` lists the rows that reached `cg_max_iterations` without meeting the tolerance."""
        st = dict(getattr(self, "_last_sample_stats", None) or {})
        if "cg_iters" in st:
            st["cg_iters"] = [int(v) for its in st["cg_iters"] for v in its.rows]
            st["cg_capped"] = [i for i, v in enumerate(st["cg_iters"]) if v >= st["cg_max_iterations"]]
        return st

    def sample_latent(self, X, n_samples, *, seed=None, cg_tolerance=None, max_cg_iterations=2000, return_state=False):
        """Joint draws of the latent function at the rows of X from the fitted variational posterior -> float64 array
        (n_samples, n).  The weights' posterior is N(m, A^-1), A = I + D T_w D with D = diag(ws) and T_w the Toeplitz operator of
        F* diag(delta) F for the fitted PG expectation delta, so

            u = A^-1 (D F*(sqrt(delta) .* e1) + e2),   f(x*) = Re F_new(ws .* (ws .* beta_mean + u)),

        e1 ~ N(0, I_N) real and e2 a conjugate-even standard complex normal on the mode grid: the bracket has covariance A,
        u ~ N(0, A^-1), and the draws have mean `_latent_mean` and covariance Phi_new D A^-1 D Phi_new^H.  The draws use the
        E-step's scaling D = ws; the exact `predictive_variance` solves with the clamped D_s, which differs from D only on modes
        with ws^2 < 1e-14 mean(ws^2), far below the draws' own solve tolerance.

        Per call: sqrt(delta) once and one plan over X.  Per block of `efgpnd._SAMPLE_BLOCK[d]` rows: one type-1 transform of
        normals generated and scaled inside the spreader (`NufftPlan.type1_normal_scaled`; neither e1 nor sqrt(delta) .* e1
        exists in memory), one right-hand-side kernel (`hermitian_normal_rows`), one batched Hermitian CG solve from zero with
        the fit's operator `_op_pred` (no Jacobi diagonal: the E-step solves the same system without one) and one batched
        type 2.  The solutions are projected onto their conjugate-even part, as `EFGPND.sample_paths` does.

        seed=None takes a 63-bit seed from torch's default generator (`torch.manual_seed` governs reproducibility); an integer
        makes the call a pure function of (fit, X, n_samples, seed).  Rows are numbered across blocks: the first k rows of a
        larger call are the draws of a k-row call (to rounding).  cg_tolerance defaults to the estimator's `cg_tol`.  Rows that
        reach max_cg_iterations are returned as they stand; their indices are in `last_sample_stats["cg_capped"]` (read on
        request) and in the state, and a return_state=True call warns about them.  return_state=True also returns a dict of
        device tensors and counts: `seed`, `weights` (ws .* beta_mean + u), `delta` (u), `rhs`, `cg_iters`, `cg_max_iterations`,
        `cg_capped`.

        Training inputs get no special case: `decision_function` returns the E-step's stochastic `posterior_mean_` there, while
        the draws always go through `beta_mean` (their mean on the training inputs is the predictive latent mean).  No fitted
        attribute changes and nothing is refitted."""
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError(f"n_samples must be at least 1 (got {n_samples})")
        max_iter = int(max_cg_iterations)
        if max_iter < 1:
            raise ValueError(f"max_cg_iterations must be at least 1 (got {max_iter})")
        self._check_fitted()
        X_arr = _check_array(X, self.n_features_in_)
        import efgpnd
        from efgp_hip.ops import NufftPlan, cg_solve_lazy, hermitian_normal_rows, normal_row_offset
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed = int(seed)
        spec, dev = self._spec, self._dev
        M, shape = spec.M, spec.shape
        tol = float(self.cg_tol if cg_tolerance is None else cg_tolerance)
        xn = self._device_points(X_arr)
        n = xn.shape[0]
        plan_new = NufftPlan(xn, spec.h, self.nufft_eps) if n else None
        root = torch.sqrt(self._delta)
        mean_w = (spec.ws * self._beta_mean).reshape(1, M)
        seed_e1, seed_e2 = efgpnd._derive_seed(seed, 1), efgpnd._derive_seed(seed, 2)
        block = efgpnd._SAMPLE_BLOCK[spec.d]
        outs, sols = [], []
        keep = dict(weights=[], delta=[], rhs=[]) if return_state else None
        for r0 in range(0, n_samples, block):
            nb = min(block, n_samples - r0)
            fz = spec.plan.type1_normal_scaled(seed_e1, nb, shape, root, index_offset=normal_row_offset(r0)).reshape(nb, M)
            rhs = hermitian_normal_rows(dev, seed_e2, nb, M, a=1.0, ws=spec.ws, fz=fz, b=1.0, index_offset=normal_row_offset(2 * r0))
            u, its = cg_solve_lazy(self._op_pred, spec.ws, 1.0, 1, rhs, None, tol, max_iter=max_iter, early_stop=True, batched=True,
                                   hermitian=True)
            its.settle()                             # reads the counts only where the solve may hold dead rows
            sols.append(its)
            # the Hermitian kernels control only the even part of the iterate; the odd part that rounding grows over a long solve
            # drops out of Re F(ws w) anyway, projecting it out makes delta and the weights what they mean (EFGPND.sample_paths)
            u = u.reshape(nb, M)
            u = 0.5 * (u + u.flip(1).conj())
            w = u + mean_w
            if keep is not None:
                keep["weights"].append(w)
                keep["delta"].append(u)
                keep["rhs"].append(rhs)
            outs.append(plan_new.type2(w, shape, real_only=True, batched=True, mode_scale=spec.ws) if n
                        else torch.empty((nb, 0), dtype=torch.float64, device=dev))
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        self._last_sample_stats = dict(seed=seed, n_samples=n_samples, blocks=-(-n_samples // block), cg_iters=sols,
                                       cg_max_iterations=max_iter)
        res = out.reshape(n_samples, n).cpu().numpy()
        if not return_state:
            return res
        stats = self.last_sample_stats
        state = dict(seed=seed, weights=torch.cat(keep["weights"]), delta=torch.cat(keep["delta"]), rhs=torch.cat(keep["rhs"]),
                     cg_iters=stats["cg_iters"], cg_max_iterations=max_iter, cg_capped=stats["cg_capped"])
        if stats["cg_capped"]:
            warnings.warn(f"sample_latent: {len(stats['cg_capped'])} of {n_samples} solves reached max_cg_iterations = {max_iter} "
                          f"without meeting the tolerance {tol:g}; raise max_cg_iterations", RuntimeWarning, stacklevel=2)
        return res, state

    # -- likelihood hooks: the ones a likelihood without parameters of its own does not need ------------------------------------
    def _refresh_likelihood(self):
        pass

    def _step_auxiliary(self, outer):
        return {}

    def _final_record(self):
        return {}


class PolyagammaGPClassifier(_BasePolyagammaGPEstimator):
    """Scikit-learn style PG-augmented GP classifier (Bernoulli likelihood, logistic link) on the HIP EFGP operators.

    Constructor keywords and defaults are the reference's.  `fit` follows its loop: delta = b / 4; per outer iteration the
    spectral state is rebuilt, one E-step (`e_step_iters` damped updates with the weighted operator built from delta as it
    stands at the start) and one M-step gradient run, and Adam (maximize=True) steps the log hyper-parameters with the raw
    gradient (g_l l, g_var var, 0); then a final E-step (seed random_state + 999_999) and the mean solve.

    Solves: `use_exact_weighted_toeplitz_operator` True or False give the same matrix F* diag(delta) F up to `nufft_eps`, so
    both run the fused weighted Toeplitz operator (efgp_cg_solve).

    Probes: with `random_state` set, the probes are the reference's (drawn by torch.Generator on the host, seeds
    random_state + 1000 outer + 17 (it + 1) for the E-step and + 10_000 for the M-step) and uploaded -- 2 J N doubles per
    outer iteration (J = n_e_probes = n_m_probes = 10, N = 1e6: 160 MB of host generation and upload per iteration), so a
    seeded fit equals the reference's.  With random_state=None the reference promises no stream: one seed per E-step /
    M-step is drawn from torch's global generator and the +-1 probes are generated on the device by the counter hash of
    efgp_rademacher_fill / efgp_nufft_type1_rademacher; they never exist in memory.

    Supported: kernel "squared_exponential" (aliases "se", "rbf"), dtype float64, predictive_variance_method "exact", a
    GPU device ("auto", "cuda", "cuda:k").  Others raise ValueError / NotImplementedError naming the option.

    After `fit`, `last_fit_stats` lists every solve (step, outer iteration, solver entry, `fused`, CG count, rows).
    """

    _what = "the PG classifier"
    _history_key, _history_label, _training_attr = "approx_accuracy", "approx_acc", "training_accuracy_"

    def _prepare_targets(self, y_arr):
        classes = np.unique(y_arr)
        if classes.size != 2:
            raise ValueError("PolyagammaGPClassifier only supports binary classification.")
        return (y_arr == classes[1]).astype(np.float64), {"classes_": classes}

    def _start_likelihood(self, targets):
        self._kappa = (targets - 0.5).contiguous()                      # y - 1/2 (b = 1)

    def _initial_delta(self, targets):
        return torch.full((self._N,), 0.25, dtype=torch.float64, device=self._dev)

    def _estep_pass(self, S, rho, probes, pseed):
        from efgp_hip.ops import pg_estep_update
        mean, sdiag, resid, correct = pg_estep_update(S, self._delta, self._targets, rho, probes=probes, seed=pseed)
        residual = float(resid.item())
        # the reference's metric is a float32 mean of the per-point hits (pg_classifier.py:129-138)
        metric = float(np.float32(int(correct.item())) / np.float32(self._N))
        return mean, sdiag, residual, metric

    def _response_mean(self, mean, variance):
        return approximate_logistic_gaussian_prob(mean, variance)

    def predict_proba(self, X, *, variance_method=None):
        p1 = np.clip(self.predict_response_mean(X, variance_method=variance_method), 1e-8, 1.0 - 1e-8)
        return np.column_stack([1.0 - p1, p1])

    def sample_proba(self, X, n_samples, *, seed=None):
        """sigmoid(f) of every draw of `sample_latent(X, n_samples, seed=seed)` -> (n_samples, n): joint draws of the probability
        of `classes_[1]`."""
        f = torch.from_numpy(self.sample_latent(X, n_samples, seed=seed))
        return torch.sigmoid(f).numpy()

    def predict(self, X):
        self._check_fitted()
        return self.classes_[(self.predict_proba(X)[:, 1] >= 0.5).astype(int)]

    def score(self, X, y):
        return float(np.mean(self.predict(X) == np.asarray(y)))


class PolyagammaGPNegativeBinomialRegressor(_BasePolyagammaGPEstimator):
    """PG-augmented GP regressor for counts: y ~ NB(r, sigmoid(f)), r = `total_count`, on the HIP EFGP operators.

    The fit loop is the classifier's with kappa = (y - r) / 2 and b = y + r.  With `learn_total_count=True`, log r is a float64
    parameter kept on the host and stepped by its own Adam (maximize=True, lr `total_count_lr` or `lr`) every
    `total_count_update_frequency`-th outer iteration, after the kernel's step, with the gradient taken from the E-step's
    marginals at the r that E-step used:  d/dr = sum_n [digamma(y_n + r) - digamma(r) + E log sigmoid(-f_n)],  the expectation
    by the `total_count_quadrature_nodes`-point Gauss-Hermite rule (efgp_pg_nb_total_count_grad, one scalar read back).  kappa
    is refreshed in the strength rows only when r has changed.  The final E-step and the mean solve use the last r.

    The training metric (efgp_pg_nb_estep_update) is the mean absolute error of the predicted mean count
    r exp(mean + var / 2); `predict`, `predict_mean_count` and `predict_response_mean` return that mean count, `score` is R^2.
    Supported options and refusals are the classifier's; at most 128 quadrature nodes when r is learnt.
    """

    _what = "the PG negative-binomial regressor"
    _history_key, _history_label, _training_attr = "mean_count_mae", "count_mae", "training_mean_absolute_error_"

    def __init__(self, *, total_count: float = 1.0, learn_total_count: bool = False, total_count_lr: float | None = None,
                 total_count_update_frequency: int = 5, total_count_quadrature_nodes: int = 12,
                 kernel: str = "squared_exponential", lengthscale_init: float = 0.3, variance_init: float = 1.0,
                 max_iter: int = 50, e_step_iters: int = 1, final_e_step_iters: int = 1, e_step_tol: float = 1e-4, rho0: float = 0.7,
                 gamma: float = 1e-3, lr: float = 0.05, n_e_probes: int = 10, n_m_probes: int = 10, cg_tol: float = 1e-6,
                 nufft_eps: float = 1e-7, spectral_eps: float = 1e-4, trunc_eps: float = 1e-4, jitter: float = 1e-8,
                 use_exact_weighted_toeplitz_operator: bool = True, reuse_e_probes: bool = True,
                 prediction_batch_size: int | None = 64, predictive_variance_method: str = "exact",
                 predictive_variance_probes: int = 16, predictive_variance_chebyshev_nodes: int = 7, warm_start: bool = False,
                 random_state: int | None = None, device: str = "auto", dtype="float64", verbose: int = 0,
                 store_history: bool = False):
        super().__init__(kernel=kernel, lengthscale_init=lengthscale_init, variance_init=variance_init, max_iter=max_iter,
                         e_step_iters=e_step_iters, final_e_step_iters=final_e_step_iters, e_step_tol=e_step_tol, rho0=rho0,
                         gamma=gamma, lr=lr, n_e_probes=n_e_probes, n_m_probes=n_m_probes, cg_tol=cg_tol, nufft_eps=nufft_eps,
                         spectral_eps=spectral_eps, trunc_eps=trunc_eps, jitter=jitter,
                         use_exact_weighted_toeplitz_operator=use_exact_weighted_toeplitz_operator, reuse_e_probes=reuse_e_probes,
                         prediction_batch_size=prediction_batch_size, predictive_variance_method=predictive_variance_method,
                         predictive_variance_probes=predictive_variance_probes,
                         predictive_variance_chebyshev_nodes=predictive_variance_chebyshev_nodes, warm_start=warm_start,
                         random_state=random_state, device=device, dtype=dtype, verbose=verbose, store_history=store_history)
        self.total_count = total_count
        self.learn_total_count = learn_total_count
        self.total_count_lr = total_count_lr
        self.total_count_update_frequency = total_count_update_frequency
        self.total_count_quadrature_nodes = total_count_quadrature_nodes

    _MAX_QUADRATURE_NODES = 128          # efgp_pg_nb_total_count_grad

    # -- likelihood (pg_classifier.py:142-171, 1558-1671) ------------------------------------------------------------------------
    def _prepare_targets(self, y_arr):
        if self.total_count <= 0:
            raise ValueError("total_count must be positive.")
        y = np.asarray(y_arr, dtype=np.float64)
        if np.any(y < 0):
            raise ValueError("Negative binomial targets must be nonnegative.")
        if not np.isfinite(y).all() or not np.allclose(y, np.round(y)):
            raise ValueError("Negative binomial targets must be integer-valued.")
        if self.total_count_update_frequency <= 0:
            raise ValueError("total_count_update_frequency must be positive.")
        if self.total_count_quadrature_nodes <= 0:
            raise ValueError("total_count_quadrature_nodes must be positive.")
        if self.learn_total_count and self.total_count_quadrature_nodes > self._MAX_QUADRATURE_NODES:
            raise ValueError(f"total_count_quadrature_nodes={self.total_count_quadrature_nodes}: at most "
                             f"{self._MAX_QUADRATURE_NODES} nodes are supported when learn_total_count=True")
        return np.round(y).astype(np.float64), {}

    def _current_total_count(self):
        raw = getattr(self, "_raw_total_count_", None)
        return float(torch.exp(raw).detach().item()) if raw is not None else float(self.total_count)

    def _start_likelihood(self, targets):
        """log r as a host float64 parameter with its own Adam (kept under warm_start), the quadrature rule on the device, and
        kappa = (y - r) / 2 at the starting r."""
        dev = self._dev
        if self.learn_total_count:
            prev = getattr(self, "_raw_total_count_", None)
            start = prev.detach().to(torch.float64) if (self.warm_start and prev is not None) \
                else torch.tensor(math.log(float(self.total_count)), dtype=torch.float64)
            self._raw_total_count_ = torch.nn.Parameter(start)
            lr = self.lr if self.total_count_lr is None else self.total_count_lr
            self._total_count_optimizer_ = torch.optim.Adam([self._raw_total_count_], lr=lr, maximize=True)
            nodes, weights = _gauss_hermite_normal_rule(int(self.total_count_quadrature_nodes))
            self._gh_nodes = torch.from_numpy(nodes.copy()).to(dev)
            self._gh_weights = torch.from_numpy(weights.copy()).to(dev)
            self._grad_r = torch.empty(1, dtype=torch.float64, device=dev)
        else:
            self._raw_total_count_ = self._total_count_optimizer_ = None
        self._escalars = torch.empty(2, dtype=torch.float64, device=dev)       # [residual, sum |mean count - y|]
        self._r = self._current_total_count()
        self._kappa = (0.5 * (targets - self._r)).contiguous()
        self._kappa_r = self._r

    def _initial_delta(self, targets):
        return 0.25 * (targets + self._r)

    def _refresh_likelihood(self):
        """kappa = (y - r) / 2 into _kappa and the E-step / M-step strength rows, when r has moved since they were written."""
        if self._r == self._kappa_r:
            return
        torch.sub(self._targets, self._r, out=self._kappa).mul_(0.5)
        self._zbuf_e[0].copy_(self._kappa)
        self._zbuf_m[int(self.n_m_probes)].copy_(self._kappa)
        self._kappa_r = self._r

    def _estep_pass(self, S, rho, probes, pseed):
        from efgp_hip.ops import pg_nb_estep_update
        mean, sdiag, scalars = pg_nb_estep_update(S, self._delta, self._targets, self._r, rho, probes=probes, seed=pseed,
                                                  out=self._escalars)
        residual, abs_err = scalars.tolist()
        return mean, sdiag, residual, abs_err / self._N

    def _step_auxiliary(self, outer):
        """The r gradient at the r of this iteration's E-step, from its marginals; an Adam step of log r on every
        total_count_update_frequency-th iteration (pg_classifier.py:1625-1662)."""
        record = {"total_count": self._r, "grad_total_count": 0.0, "total_count_updated": 0.0}
        if not self.learn_total_count:
            return record
        from efgp_hip.ops import pg_nb_total_count_grad
        grad = float(pg_nb_total_count_grad(self._targets, self._mean, self._sigma_diag, self._r, self._gh_nodes, self._gh_weights,
                                            out=self._grad_r).item())
        record["grad_total_count"] = grad
        if (outer + 1) % int(self.total_count_update_frequency) == 0:
            raw = self._raw_total_count_
            raw.grad = (torch.tensor(grad, dtype=torch.float64) * torch.exp(raw)).detach()
            self._total_count_optimizer_.step()
            self._total_count_optimizer_.zero_grad(set_to_none=True)
            self._r = self._current_total_count()
            record["total_count"] = self._r
            record["total_count_updated"] = 1.0
        return record

    def _final_record(self):
        return {"total_count": self._r, "grad_total_count": 0.0, "total_count_updated": 0.0}

    def fit(self, X, y):
        super().fit(X, y)
        self.total_count_ = self._r
        self.shape_parameter_ = self._r
        return self

    # -- prediction ----------------------------------------------------------------------------------------------------------
    def _response_mean(self, mean, variance):
        return negative_binomial_gaussian_mean(mean, variance, total_count=self.total_count_)

    def predict_mean_count(self, X, *, variance_method=None):
        return self.predict_response_mean(X, variance_method=variance_method)

    def sample_mean_count(self, X, n_samples, *, seed=None):
        """r exp(f) of every draw of `sample_latent(X, n_samples, seed=seed)` with the fitted total count r -> (n_samples, n): joint
        draws of the mean count, whose Gaussian expectation is `negative_binomial_gaussian_mean`."""
        f = torch.from_numpy(self.sample_latent(X, n_samples, seed=seed))
        return (self.total_count_ * torch.exp(f)).numpy()

    def predict(self, X):
        return self.predict_mean_count(X)

    def score(self, X, y, sample_weight=None):
        """R^2 of predict(X) against y (scikit-learn's RegressorMixin.score: 1.0 for a perfect fit of constant y, 0.0 for an
        imperfect one)."""
        y_true = np.asarray(y, dtype=np.float64).reshape(-1)
        y_pred = np.asarray(self.predict(X), dtype=np.float64).reshape(-1)
        w = np.ones_like(y_true) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64).reshape(-1)
        num = float(np.sum(w * (y_true - y_pred) ** 2))
        den = float(np.sum(w * (y_true - np.average(y_true, weights=w)) ** 2))
        if den == 0.0:
            return 1.0 if num == 0.0 else 0.0
        return 1.0 - num / den
