// Stand-alone host program for a sanitizer run of the grid's host code: csrc/grid_host.cpp (the two bisections, the isotropic host
// weights and the ARD host twin efgp_spectral_weights_host_nd) on the blocks the ARD tests use.  No device involved.
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/ard_host_check.cpp gp-quadrature_amd/csrc/grid_host.cpp -o ard_host_check && ./ard_host_check
//
// Every output array is allocated at its exact size, so a write past a block is an AddressSanitizer report; the program also
// checks the equal-lengthscale reduction to the isotropic weights and exits non-zero on any mismatch.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/efgp_hip.h"

namespace efgp {
void set_error(const char* fmt, ...) {          // what csrc/common.cpp provides inside the library
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    std::fputc('\n', stderr);
    va_end(ap);
}
}  // namespace efgp

static int fails = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static void run_block(int kind, double nu, int dim, const double* ell, const double* h, const int64_t* n) {
    int64_t M = 1;
    for (int a = 0; a < dim; ++a) M *= n[a];
    std::vector<double> ws(2 * M), dp(2 * M * (dim + 1)), ws2(2 * M);
    CHECK(efgp_spectral_weights_host_nd(kind, dim, nu, ell, 1.3, h, n, ws.data(), dp.data()) == 0);
    CHECK(efgp_spectral_weights_host_nd(kind, dim, nu, ell, 1.3, h, n, ws2.data(), nullptr) == 0);
    double big = 0.0;
    for (int64_t t = 0; t < M; ++t) {
        CHECK(std::isfinite(ws[2 * t]) && ws[2 * t] > 0.0 && ws[2 * t + 1] == 0.0 && ws2[2 * t] == ws[2 * t]);
        CHECK(ws[2 * t] == ws[2 * (M - 1 - t)]);                                   // even on the symmetric box
        big = std::fmax(big, ws[2 * t]);
        for (int j = 0; j <= dim; ++j) CHECK(std::isfinite(dp[2 * ((dim + 1) * t + j)]) && dp[2 * ((dim + 1) * t + j) + 1] == 0.0);
    }
    CHECK(ws[2 * ((M - 1) / 2)] == big);                                           // the largest weight sits at the zero frequency
    std::printf("kind %d nu %.1f block", kind, nu);
    for (int a = 0; a < dim; ++a) std::printf(" %lld", (long long)n[a]);
    std::printf(": M = %lld, max ws %.6e\n", (long long)M, big);
}

int main() {
    // the blocks of tests/test_gpu_ard.py
    const double l1[1] = {0.1}, h1[1] = {0.7};
    const int64_t n1[1] = {9};
    const double l2[2] = {0.08, 0.5}, h2[2] = {0.7444051126619937, 0.40883642260438513};
    const int64_t n2a[2] = {27, 9}, n2b[2] = {3, 11}, n2c[2] = {35, 11}, n2d[2] = {45, 17};
    const double l3[3] = {0.1, 0.5, 0.3}, h3[3] = {0.73, 0.42, 0.66};
    const int64_t n3a[3] = {5, 3, 7}, n3b[3] = {23, 7, 9};
    for (int kind = 0; kind < 2; ++kind) {
        for (double nu : {0.5, 1.5, 2.5}) {
            if (kind == 0 && nu != 0.5) continue;
            run_block(kind, nu, 1, l1, h1, n1);
            run_block(kind, nu, 2, l2, h2, n2a);
            run_block(kind, nu, 2, l2, h2, n2b);
            run_block(kind, nu, 2, l2, h2, n2c);
            run_block(kind, nu, 2, l2, h2, n2d);
            run_block(kind, nu, 3, l3, h3, n3a);
            run_block(kind, nu, 3, l3, h3, n3b);
        }
    }
    // equal lengthscales: the isotropic host weights (c0 formed as utils/kernels.py kernel_constants does for the SE kernel)
    {
        const double ell = 0.3, var = 1.3, h = 0.4371432699668902;
        const int mtot = 13;
        const double le[2] = {ell, ell}, he[2] = {h, h};
        const int64_t ne[2] = {mtot, mtot};
        std::vector<double> a(2 * mtot * mtot), da(4 * mtot * mtot), b(2 * mtot * mtot), db(6 * mtot * mtot);
        CHECK(efgp_spectral_weights_host(0, 2, 0.0, ell, var, 2.0 * M_PI * ell * ell * var, h, mtot, a.data(), da.data()) == 0);
        CHECK(efgp_spectral_weights_host_nd(0, 2, 0.0, le, var, he, ne, b.data(), db.data()) == 0);
        for (int t = 0; t < mtot * mtot; ++t) {
            CHECK(std::fabs(a[2 * t] - b[2 * t]) <= 1e-12 * a[2 * (mtot * mtot / 2)]);
            CHECK(std::fabs(da[4 * t] - (db[6 * t] + db[6 * t + 2])) <= 1e-12 * std::fabs(da[4 * (mtot * mtot / 2)]));
        }
    }
    // the two bisections at the lengthscales of the anisotropic fit
    for (double ell : {0.08, 0.5, 0.3}) {
        double lt = 0.0, lf = 0.0;
        const double c0 = 2.0 * M_PI * ell * ell;
        CHECK(efgp_grid_bounds(0, 2, 0.0, ell, 1.0, c0, c0, 1e-4, 1e-4, &lt, &lf) == 0);
        CHECK(lt > 0.0 && lf > 0.0);
        std::printf("l = %.2f: Ltime %.6f Lfreq %.6f\n", ell, lt, lf);
    }
    // refused arguments leave the outputs alone
    {
        const int64_t even[2] = {8, 9};
        double w[2] = {-1.0, -1.0};
        CHECK(efgp_spectral_weights_host_nd(0, 2, 0.0, l2, 1.0, h2, even, w, nullptr) != 0);
        CHECK(efgp_spectral_weights_host_nd(1, 2, 2.0, l2, 1.0, h2, n2a, w, nullptr) != 0);
        CHECK(efgp_spectral_weights_host_nd(0, 4, 0.0, l2, 1.0, h2, n2a, w, nullptr) != 0);
        CHECK(w[0] == -1.0 && w[1] == -1.0);
    }
    std::printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
