// Spectral density of the built-in kernels at one node of the frequency grid xi = h (-m..m)^d (efgpnd.py:766-780,
// kernels/*.py).  Shared by spectral_weights_kernel (variance_ops.hip) and the fused mean solve (cg_persistent.hip), so that
// the weights the solve evaluates for itself are bitwise those of the standalone launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace efgp {

// kind 0: squared exponential, 1: Matern (nu); c0 is the kernel's constant (utils/kernels.py kernel_constants).
// S = S(|xi_t|), q = |xi_t|^2 and hd = h^d for node t (row-major, last dimension fastest).
__device__ __forceinline__ void spectral_density_at(int kind, int dim, double nu, double ell, double c0, double h, int mtot, int64_t t,
                                                    double& S, double& q, double& hd) {
    const int m = (mtot - 1) / 2;
    int64_t rem = t;
    q = 0.0;
    for (int a = dim - 1; a >= 0; --a) {
        const double xa = (double)((int)(rem % mtot) - m) * h;
        rem /= mtot;
        q += xa * xa;
    }
    const double two_pi = 6.283185307179586476925286766559;
    hd = h;
    for (int a = 1; a < dim; ++a) hd *= h;
    if (kind == 0) {
        S = c0 * exp(-(two_pi * two_pi) * (ell * ell) * q / 2);
    } else {
        const double pi = 3.14159265358979323846264338327950288;
        const double den = 2 * nu / (ell * ell) + (4 * pi * pi) * q;
        S = c0 * pow(den, -(nu + dim / 2.0));
    }
}

// ws[t] = sqrt(S h^d): the real part of the feature weight (the imaginary part is 0)
__device__ __forceinline__ double spectral_weight_at(int kind, int dim, double nu, double ell, double c0, double h, int mtot, int64_t t) {
    double S, q, hd;
    spectral_density_at(kind, dim, nu, ell, c0, h, mtot, t, S, q, hd);
    return sqrt(S * hd);
}

}  // namespace efgp
