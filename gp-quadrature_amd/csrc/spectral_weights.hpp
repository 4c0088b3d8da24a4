// Spectral density of the built-in kernels at one node of the frequency grid xi = h (-m..m)^d (efgpnd.py:766-780,
// kernels/*.py).  Shared by spectral_weights_kernel (variance_ops.hip) and the fused mean solve (cg_herm.hip), so that
// the weights the solve evaluates for itself are bitwise those of the standalone launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
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

// ---- ARD kernels (kernels/ard.py) on the per-axis grid omega_a = k_a h_a, k_a = -(n_a - 1)/2 .. (n_a - 1)/2 --------------------
// S(omega) = (prod_a l_a) S_1(rho), rho^2 = sum_a (l_a omega_a)^2, S_1 the isotropic density of the class at lengthscale 1:
//   kind 0: S_1 = variance (2 pi)^(d/2) exp(-(2 pi)^2 rho^2 / 2);   kind 1: S_1 = variance scaling(1) (2 nu + 4 pi^2 rho^2)^-(nu + d/2).
// c1 = variance * prod l_a * the class constant (ard_spec forms it on the host).
struct ArdSpec {
    int kind, dim;
    double nu, c1;
    double ell[3], h[3];
    int n[3];
};

// S and d log S / d l_a at node t (row-major, last axis fastest): the density is evaluated once, every derivative row is S * dlog[a]
__host__ __device__ inline void spectral_density_nd_at(const ArdSpec& k, int64_t t, double& S, double* dlog) {
    const double two_pi = 6.283185307179586476925286766559, pi = 3.14159265358979323846264338327950288;
    double w2[3] = {0.0, 0.0, 0.0}, rho2 = 0.0;
    int64_t rem = t;
    for (int a = k.dim - 1; a >= 0; --a) {
        const double om = (double)((int)(rem % k.n[a]) - (k.n[a] - 1) / 2) * k.h[a];
        rem /= k.n[a];
        w2[a] = om * om;
    }
    for (int a = 0; a < k.dim; ++a) rho2 += (k.ell[a] * k.ell[a]) * w2[a];
    if (k.kind == 0) {
        S = k.c1 * exp(-(two_pi * two_pi) * rho2 / 2);
        for (int a = 0; a < k.dim; ++a) dlog[a] = 1.0 / k.ell[a] - (two_pi * two_pi) * k.ell[a] * w2[a];
    } else {
        const double p = k.nu + k.dim / 2.0, den = 2 * k.nu + (4 * pi * pi) * rho2;
        S = k.c1 * pow(den, -p);
        for (int a = 0; a < k.dim; ++a) dlog[a] = 1.0 / k.ell[a] - p * (8 * pi * pi) * k.ell[a] * w2[a] / den;
    }
}

// argument check and constants of the two `_nd` weight entries (host); *hd = prod_a h_a, *M = prod_a n_a
inline bool ard_spec(int kind, int dim, double nu, const double* ell, double variance, const double* h, const int64_t* n_modes, ArdSpec* k,
                     double* hd, int64_t* M) {
    if (!(kind == 0 || (kind == 1 && (nu == 0.5 || nu == 1.5 || nu == 2.5))) || dim < 1 || dim > 3 || !ell || !h || !n_modes ||
        !(variance > 0.0))
        return false;
    k->kind = kind;
    k->dim = dim;
    k->nu = nu;
    *hd = 1.0;
    *M = 1;
    double lprod = 1.0;
    for (int a = 0; a < 3; ++a) {
        k->ell[a] = 1.0;
        k->h[a] = 0.0;
        k->n[a] = 1;
    }
    for (int a = 0; a < dim; ++a) {
        if (!(ell[a] > 0.0) || !(h[a] > 0.0) || n_modes[a] < 1 || !(n_modes[a] & 1) || n_modes[a] > (1 << 20)) return false;
        k->ell[a] = ell[a];
        k->h[a] = h[a];
        k->n[a] = (int)n_modes[a];
        lprod *= ell[a];
        *hd *= h[a];
        *M *= n_modes[a];
    }
    if (*M > ((int64_t)1 << 31)) return false;
    const double pi = 3.14159265358979323846264338327950288;
    if (kind == 0) k->c1 = variance * lprod * pow(2.0 * pi, dim / 2.0);
    else k->c1 = variance * lprod * pow(2.0 * sqrt(pi), (double)dim) * tgamma(nu + dim / 2.0) * pow(2.0 * nu, nu) / tgamma(nu);
    return true;
}

}  // namespace efgp
