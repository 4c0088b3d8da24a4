"""Kernels with one lengthscale per dimension (automatic relevance determination, ARD).

k(x, x') = variance * kappa(r),  r^2 = sum_j ((x_j - x'_j) / l_j)^2,  with kappa the unit-lengthscale profile of the isotropic
class (`SquaredExponential`, `Matern` with nu in {1/2, 3/2, 5/2}).  In x-space frequencies omega the spectral density is

    S(omega) = (prod_j l_j) * S_1(rho),   rho^2 = sum_j l_j^2 omega_j^2,

S_1 being the isotropic density of the same class at lengthscale 1 (same variance, same dimension): the change of variables
x_j -> x_j / l_j.  Hyper-parameters are ``lengthscale_0 .. lengthscale_{d-1}, variance`` in the same `GPParams` as every
other kernel; EFGPND puts these kernels on a per-axis Fourier grid (`utils.kernels.get_xis_nd`).
"""
import math

import torch

from .kernel import Kernel
from .matern import Matern
from .squared_exponential import SquaredExponential

_TWO_PI = 2.0 * math.pi


class _ARDKernel(Kernel):
    """Shared parts of the ARD kernels; subclasses provide the profile, S_1 and d log S / d l_j."""
    ard_kind = None                 # 0 squared exponential, 1 Matern: the `kind` of efgp_spectral_weights_nd
    nu = 0.0

    def __init__(self, *, dimension, init_lengthscale=None, init_variance=None, **kwargs):
        if not isinstance(dimension, int) or isinstance(dimension, bool) or dimension < 1:
            raise ValueError(f"dimension must be an integer >= 1, got {dimension!r}")
        if init_lengthscale is None:
            init_lengthscale = 1.0
        if isinstance(init_lengthscale, (int, float)):
            ells = [float(init_lengthscale)] * dimension
        else:
            ells = [float(v) for v in (init_lengthscale.tolist() if torch.is_tensor(init_lengthscale) else init_lengthscale)]
            if len(ells) != dimension:
                raise ValueError(f"init_lengthscale must be a number or a sequence of {dimension} numbers, got {len(ells)}")
        # what Kernel.__init__ does, with a hyper list that depends on the dimension
        self.dimension = dimension
        self.hypers = [f"lengthscale_{j}" for j in range(dimension)] + ["variance"]
        self.num_hypers = dimension + 2
        self._gp_params_ref = None
        self._params_dict = {}
        for name, val in zip(self.hypers, ells + [1.0 if init_variance is None else float(init_variance)]):
            if not (val >= 1e-6):
                raise ValueError(f"init_{name} must be >= 1e-6, got {val}")
            setattr(self, "init_" + name, val)
            self._params_dict[name] = val
        from .kernel_params import GPParams
        GPParams(kernel=self, init_sig2=0.1)

    # -- hyper-parameter access ------------------------------------------------------------
    @property
    def lengthscales(self):
        """The d lengthscales as Python floats."""
        return tuple(self.get_hypers()[:self.dimension])

    @property
    def variance(self):
        return self.get_hyper("variance")

    @variance.setter
    def variance(self, v):
        self.set_hyper("variance", v)

    def set_hyper(self, name, value):
        """`lengthscale` sets every axis (a number) or all of them (a sequence of d): the form EFGPND's initialisation uses."""
        if name == "lengthscale":
            vals = [float(value)] * self.dimension if isinstance(value, (int, float)) else [float(v) for v in value]
            if len(vals) != self.dimension:
                raise ValueError(f"lengthscale needs {self.dimension} values, got {len(vals)}")
            for j, v in enumerate(vals):
                super().set_hyper(f"lengthscale_{j}", v)
            return
        super().set_hyper(name, value)

    def isotropic(self, axis):
        """The isotropic kernel of the same class, dimension and variance with this kernel's lengthscale of `axis`: the kernel
        whose truncation bounds size that axis of the grid (utils.kernels.get_xis_nd)."""
        vals = self.get_hypers()
        iso = self._iso_kernel(vals[axis], vals[-1])
        iso._gp_params_ref = None         # read the exact floats, not their round trip through a log-space parameter vector
        return iso

    # -- kernel values -------------------------------------------------------------------------
    def _profile(self, r):
        raise NotImplementedError

    def kernel(self, distance):
        if self.dimension != 1:
            raise ValueError(f"{type(self).__name__}.kernel(distance) is defined for dimension 1 only: with a lengthscale per axis the "
                             "kernel is a function of the coordinate differences -- use kernel_matrix(x, y)")
        return self.variance * self._profile(torch.abs(distance) / self.lengthscales[0])

    def kernel_matrix(self, x, y):
        if x.ndim == 1:
            x = x.unsqueeze(-1)
        if y.ndim == 1:
            y = y.unsqueeze(-1)
        if x.shape[1] != self.dimension or y.shape[1] != self.dimension:
            raise ValueError(f"kernel_matrix needs points with {self.dimension} columns")
        vals = self.get_hypers()
        ell = torch.tensor(vals[:-1], dtype=x.dtype, device=x.device)
        return vals[-1] * self._profile(torch.cdist(x / ell, y / ell))

    # -- spectral density ------------------------------------------------------------------------
    def _S1(self, rho2, var):
        raise NotImplementedError

    def _dlog(self, ell, w2, rho2):
        """d log S / d l_j for every node: (M, d)."""
        raise NotImplementedError

    def _nodes(self, omega):
        if omega.ndim == 1:
            omega = omega.unsqueeze(-1)
        if omega.shape[-1] != self.dimension:
            raise ValueError(f"frequencies need {self.dimension} columns, got {omega.shape[-1]}")
        vals = self.get_hypers()
        ell = torch.tensor(vals[:-1], dtype=omega.dtype, device=omega.device)
        w2 = omega ** 2
        return ell, vals[-1], w2, torch.sum(ell ** 2 * w2, dim=-1)

    def spectral_density(self, omega):
        ell, var, _, rho2 = self._nodes(omega)
        return math.prod(ell.tolist()) * self._S1(rho2, var)

    def spectral_grad(self, omega):
        """(M, d + 1): dS/dl_0 .. dS/dl_{d-1}, dS/dvariance."""
        ell, var, w2, rho2 = self._nodes(omega)
        S = math.prod(ell.tolist()) * self._S1(rho2, var)
        return torch.cat((S.unsqueeze(-1) * self._dlog(ell, w2, rho2), (S / var).unsqueeze(-1)), dim=-1)

    # -- dense helpers -----------------------------------------------------------------------------
    def log_marginal(self, x, y, sigmasq):
        return self._dense_log_marginal(x, y, sigmasq)

    def _axis_scale(self):
        return 1.0

    def estimate_hyperparameters(self, x, y, K=1000):
        """The isotropic class's median-distance heuristic applied per axis to |x_j - x'_j| -> ((l_0..l_{d-1}), variance, noise)."""
        if x.ndim == 1:
            x = x.unsqueeze(-1)
        y_var = torch.var(y).item()
        n = x.shape[0]
        xs = x[torch.randperm(n)[:K]] if n > K else x
        ells = []
        for j in range(self.dimension):
            dj = (xs[:, j, None] - xs[None, :, j]).abs()
            mask = dj > 0
            ells.append(self._axis_scale() * torch.median(dj[mask]).item() if mask.sum() > 0 else 1.0)
        return tuple(ells), y_var, 0.2 * y_var


class SquaredExponentialARD(_ARDKernel):
    """k = variance exp(-r^2 / 2), r^2 = sum_j ((x_j - x'_j) / l_j)^2."""
    ard_kind = 0

    def _iso_kernel(self, ell, var):
        return SquaredExponential(dimension=self.dimension, init_lengthscale=ell, init_variance=var)

    def _profile(self, r):
        return torch.exp(-0.5 * r ** 2)

    def _S1(self, rho2, var):
        return _TWO_PI ** (self.dimension / 2) * var * torch.exp(-(_TWO_PI ** 2) * rho2 / 2)

    def _dlog(self, ell, w2, rho2):
        return 1.0 / ell - (_TWO_PI ** 2) * ell * w2

    def _axis_scale(self):
        return 0.5                  # squared_exponential.py: 0.5 x the median distance


class MaternARD(_ARDKernel):
    """Matern(nu) profile of r, nu in {1/2, 3/2, 5/2}."""
    ard_kind = 1

    def __init__(self, *, dimension, nu=2.5, **kwargs):
        nu = float(nu)
        if nu not in (0.5, 1.5, 2.5):
            raise ValueError(f"nu must be one of 0.5, 1.5, 2.5, got {nu}")
        self.nu = nu
        super().__init__(dimension=dimension, **kwargs)

    def _iso_kernel(self, ell, var):
        return Matern(dimension=self.dimension, nu=self.nu, init_lengthscale=ell, init_variance=var)

    def _profile(self, s):
        if self.nu == 0.5:
            return torch.exp(-s)
        if self.nu == 1.5:
            return (1 + math.sqrt(3) * s) * torch.exp(-math.sqrt(3) * s)
        return (1 + math.sqrt(5) * s + 5 * s ** 2 / 3) * torch.exp(-math.sqrt(5) * s)

    def _scaling1(self):
        nu, d = self.nu, self.dimension
        return (2 * math.sqrt(math.pi)) ** d * math.gamma(nu + d / 2) * (2 * nu) ** nu / math.gamma(nu)

    def _S1(self, rho2, var):
        return var * self._scaling1() * (2 * self.nu + (4 * math.pi ** 2) * rho2) ** (-(self.nu + self.dimension / 2))

    def _dlog(self, ell, w2, rho2):
        den = (2 * self.nu + (4 * math.pi ** 2) * rho2).unsqueeze(-1)
        return 1.0 / ell - (self.nu + self.dimension / 2) * (8 * math.pi ** 2) * ell * w2 / den
