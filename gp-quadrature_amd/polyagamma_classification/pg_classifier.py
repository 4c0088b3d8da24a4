"""Polya-Gamma (PG) augmented GP classifier on the HIP EFGP operators (reference: polyagamma_classification/pg_classifier.py,
`PolyagammaGPClassifier`, Bernoulli likelihood with logistic link).

Every solve of the model is the weighted feature-space system  (I + D T_w D) u = b,  T_w the Toeplitz operator of
F* diag(w) F for the PG weights w = delta, D = ws (E-step) or the clamped D_s (M-step, mean, prediction).  Here each of
them is ONE batched call of the fused device solver (efgp_cg_solve, variant 1 with sigma^2 = 1), the transforms are the
library's NUFFT plans on a per-fit point layout, and the N-scale pointwise work of the PG update and the M-step's trace
estimator are kernels of their own (efgp_pg_estep_update, efgp_pg_weight_rows, efgp_pg_mstep_terms; csrc/pg_ops.hip).
torch carries allocations, the O(M) diagonal products around the solves and the O(#hypers) optimiser state.

Scope: SE kernel, float64, predictive_variance_method="exact", a GPU device.  Anything else is refused with an error that
names the option.  The product path does not import scikit-learn.
"""
from __future__ import annotations

import inspect
import math
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

__all__ = ["PolyagammaGPClassifier", "approximate_logistic_gaussian_prob", "_pg_omega_expectation"]

_SE_NAMES = ("squared_exponential", "se", "rbf")
_EXACT_VARIANCE = "exact"
_UNSUPPORTED_VARIANCE = ("stochastic", "stochastic_diag_sums", "chebyshev")


def approximate_logistic_gaussian_prob(mean: torch.Tensor, variance: torch.Tensor | None = None) -> torch.Tensor:
    """E[sigmoid(f)] for f ~ N(mean, variance) by the probit-style moment approximation
    sigmoid(mean / sqrt(1 + pi variance / 8)) (negative variances count as 0); sigmoid(mean) without a variance."""
    if variance is None:
        return torch.sigmoid(mean)
    scale = torch.sqrt(1.0 + (math.pi / 8.0) * variance.clamp_min(0.0))
    return torch.sigmoid(mean / scale)


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


class PolyagammaGPClassifier:
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
            raise ValueError(f"dtype={dt!r} is not supported: the PG classifier runs in float64 only")
        method = str(self.predictive_variance_method).lower()
        if method in _UNSUPPORTED_VARIANCE:
            raise NotImplementedError(f"predictive_variance_method={self.predictive_variance_method!r} is not implemented; "
                                      "use 'exact'")
        if method != _EXACT_VARIANCE:
            raise ValueError(f"predictive_variance_method={self.predictive_variance_method!r}: must be one of "
                             "{'exact', 'stochastic', 'stochastic_diag_sums', 'chebyshev'}")
        dev = str(self.device)
        if dev == "cpu" or dev.startswith("cpu:"):
            raise ValueError(f"device={self.device!r} is not supported: the PG classifier runs on the GPU only (HIP kernels, "
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
        from efgp_hip.ops import pg_estep_update
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
            mean, sdiag, resid, correct = pg_estep_update(S, self._delta, self._targets, rho, probes=probes, seed=pseed)
            self._mean, self._sigma_diag = mean, sdiag
            residual = float(resid.item())
            # the reference's metric is a float32 mean of the per-point hits (pg_classifier.py:129-138)
            metric = float(np.float32(int(correct.item())) / np.float32(N))
            if self.verbose > 1:
                print(f"E-step it {it:3d} rho={rho:.3f} max|Delta-Lambda|={residual:.3e} approx_acc={metric:.4f}")
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
        classes = np.unique(y_arr)
        if classes.size != 2:
            raise ValueError("PolyagammaGPClassifier only supports binary classification.")
        self._validate_options()
        from efgp_hip.ops import PointSet
        from kernels.squared_exponential import SquaredExponential

        dev = self._resolve_device()
        self._dev = dev
        self.classes_ = classes
        self.n_features_in_ = X_arr.shape[1]
        self._X_train_np_ = X_arr.copy()
        N, d = X_arr.shape
        self._N = N
        self.last_fit_stats = {"solves": []}

        xd = torch.as_tensor(X_arr).to(dev).contiguous()
        targets = torch.as_tensor((y_arr == classes[1]).astype(np.float64)).to(dev).contiguous()
        self._xd, self._targets = xd, targets
        self._kappa = (targets - 0.5).contiguous()                      # y - 1/2 (b = 1)
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
            self._delta = torch.full((N,), 0.25, dtype=torch.float64, device=dev)      # 0.25 b
        self._mean = self._sigma_diag = None
        kernel = self.kernel_
        raw = kernel._gp_params_ref.raw
        optimizer = torch.optim.Adam(kernel._gp_params_ref.parameters(), lr=self.lr, maximize=True)
        spec_args = (self._points, xd, L, self.spectral_eps, self.trunc_eps, self.nufft_eps)
        rs = self.random_state
        history = []
        mstep = None
        for outer in range(int(self.max_iter)):
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
            record = {"iter": float(outer), "lengthscale": float(kernel.lengthscale), "variance": float(kernel.variance),
                      "grad_lengthscale": g[0], "grad_variance": g[1], "e_residual": est["residual"], "e_cg_iters": est["cg_iters"],
                      "m_cg_iters": float(mstep["cg_iters"]), "approx_accuracy": est["metric"]}
            history.append(record)
            if self.verbose:
                print(f"outer {outer:3d} lengthscale={record['lengthscale']:.5f} variance={record['variance']:.5f} "
                      f"grad=({g[0]:+.3e}, {g[1]:+.3e}) approx_acc={est['metric']:.4f}")

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
        self.training_accuracy_ = fin["metric"]
        self.m_step_gradient_ = mstep["grad"].detach().cpu().numpy() if mstep is not None else np.zeros(2)
        self.beta_mean_ = self._beta_mean.detach().cpu().numpy()
        self.history_ = history if self.store_history else []
        self.history_.append({"iter": float(self.max_iter), "lengthscale": self.lengthscale_, "variance": self.variance_,
                              "grad_lengthscale": float(self.m_step_gradient_[0]), "grad_variance": float(self.m_step_gradient_[1]),
                              "e_residual": fin["residual"], "e_cg_iters": fin["cg_iters"], "m_cg_iters": float(beta_iters),
                              "approx_accuracy": fin["metric"]})
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

    def predictive_variance(self, X):
        self._check_fitted()
        X_arr = _check_array(X, self.n_features_in_)
        if self._is_training_input(X_arr):
            return self.posterior_var_diag_.copy()
        return self._latent_variance(self._device_points(X_arr)).cpu().numpy()

    def predict_response_mean(self, X):
        self._check_fitted()
        X_arr = _check_array(X, self.n_features_in_)
        if self._is_training_input(X_arr):
            mean = torch.as_tensor(self.posterior_mean_, dtype=torch.float64)
            variance = torch.as_tensor(self.posterior_var_diag_, dtype=torch.float64)
        else:
            xn = self._device_points(X_arr)
            mean, variance = self._latent_mean(xn), self._latent_variance(xn)
        return approximate_logistic_gaussian_prob(mean, variance).cpu().numpy()

    def predict_proba(self, X):
        p1 = np.clip(self.predict_response_mean(X), 1e-8, 1.0 - 1e-8)
        return np.column_stack([1.0 - p1, p1])

    def predict(self, X):
        self._check_fitted()
        return self.classes_[(self.predict_proba(X)[:, 1] >= 0.5).astype(int)]

    def score(self, X, y):
        return float(np.mean(self.predict(X) == np.asarray(y)))
