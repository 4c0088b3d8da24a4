// The value and the d first partial derivatives of a finite trigonometric sum, as rows of Fourier coefficients:
//   efgp_mode_jet_rows   out[b, 0, k]     = s_k f[b, k]
//                        out[b, 1 + a, k] = (2 pi h_a k_a) i (s_k f[b, k])          a = 0 .. d - 1
// f(x) = Re sum_k s_k f_k exp(2 pi i sum_a h_a k_a x_a) has the partial along axis a with mode k multiplied by 2 pi i h_a k_a, so the
// 1 + d rows of one coefficient row go through any type-2 transform of the library as they stand (EFGPND.predict_gradient).
//
// Shape: elementwise, bound by bandwidth (16 bytes read, 16 (1 + d) written per mode and row).  A thread owns a mode: it takes the
// slot apart into the d mode numbers ONCE, forms the d real factors 2 pi h_a k_a, and then walks the rows; per row one 16-byte
// load, one complex product s_k f (none without a scale) and 1 + d 16-byte stores.  i t p is a swap, a sign flip and two real
// multiplications.  A slot with k_a = 0 stores +0.0 + 0.0i.  The jobs (row, mode block) are strided inside the kernel over a bounded
// grid -- rows over gridDim.y, mode blocks over gridDim.x -- so any row count is one launch.  No atomics, no LDS, every output is
// written by one thread in a fixed order of operations: two calls agree bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace efgp {

namespace jet {

constexpr int kThreads = 256;                  // four wave64
constexpr int kMaxBlocksX = 1024;              // workgroups along the modes
constexpr int64_t kMaxWorkgroups = 8192;       // of the whole grid: 32 per compute unit

struct Args {
    int64_t M, nrows;
    int dim, modeord;
    int64_t n[3];
    double w[3];               // 2 pi h_a
    const double2* f;          // (nrows, M)
    const double2* s;          // (M) or null
    double2* out;              // (nrows, 1 + dim, M)
};

__global__ __launch_bounds__(kThreads) void mode_jet_rows_kernel(Args a) {
    const int64_t plane = a.M;
    const int64_t row_out = (int64_t)(1 + a.dim) * a.M;
    for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < a.M; m += (int64_t)gridDim.x * kThreads) {
        double t[3] = {0.0, 0.0, 0.0};
        int64_t rem = m;
#pragma unroll
        for (int ax = 2; ax >= 0; --ax) {
            if (ax < a.dim) {                  // row-major, last axis fastest
                const int64_t n = a.n[ax];
                const int64_t slot = rem % n;
                rem /= n;
                const int64_t k = a.modeord ? (slot <= (n - 1) / 2 ? slot : slot - n) : slot - n / 2;
                t[ax] = a.w[ax] * (double)k;
            }
        }
        const bool scaled = a.s != nullptr;
        const double2 s = scaled ? a.s[m] : make_double2(1.0, 0.0);
        for (int64_t b = blockIdx.y; b < a.nrows; b += gridDim.y) {
            double2 p = a.f[b * a.M + m];
            if (scaled) p = make_double2(s.x * p.x - s.y * p.y, s.x * p.y + s.y * p.x);
            double2* o = a.out + b * row_out + m;
            o[0] = p;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
                if (ax < a.dim) o[(1 + ax) * plane] = t[ax] == 0.0 ? make_double2(0.0, 0.0) : make_double2(-(t[ax] * p.y), t[ax] * p.x);
        }
    }
}

}  // namespace jet
}  // namespace efgp

using namespace efgp;

extern "C" {

int efgp_mode_jet_rows(int device, int dim, const int64_t* n_modes, const double* h, const void* f, const void* mode_scale, int64_t nrows,
                       int modeord, void* out, void* stream_) {
    using namespace jet;
    EFGP_REQUIRE(dim >= 1 && dim <= 3, "efgp_mode_jet_rows: dim must be 1, 2 or 3 (got %d)", dim);
    EFGP_REQUIRE(n_modes && h, "efgp_mode_jet_rows: null n_modes / h");
    EFGP_REQUIRE(modeord == 0 || modeord == 1, "efgp_mode_jet_rows: modeord must be 0 or 1 (got %d)", modeord);
    EFGP_REQUIRE(nrows >= 0, "efgp_mode_jet_rows: nrows must not be negative (got %lld)", (long long)nrows);
    Args a;
    a.M = 1;
    for (int ax = 0; ax < 3; ++ax) {
        a.n[ax] = 1;
        a.w[ax] = 0.0;
    }
    for (int ax = 0; ax < dim; ++ax) {
        EFGP_REQUIRE(n_modes[ax] >= 1 && n_modes[ax] <= (int64_t(1) << 40) / a.M, "efgp_mode_jet_rows: bad mode count %lld on axis %d",
                     (long long)n_modes[ax], ax);
        EFGP_REQUIRE(std::isfinite(h[ax]), "efgp_mode_jet_rows: h[%d] is not finite", ax);
        a.n[ax] = n_modes[ax];
        a.M *= n_modes[ax];
        a.w[ax] = 2.0 * M_PI * h[ax];
    }
    if (nrows == 0) return EFGP_OK;
    EFGP_REQUIRE(f && out, "efgp_mode_jet_rows: null argument");
    EFGP_REQUIRE(nrows <= (int64_t(1) << 58) / ((1 + dim) * a.M), "efgp_mode_jet_rows: %lld rows of %lld modes overflow the index",
                 (long long)nrows, (long long)a.M);
    EFGP_REQUIRE(((uintptr_t)f & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)mode_scale & 15) == 0,
                 "efgp_mode_jet_rows: f, mode_scale and out must be 16-byte aligned");
    if (!device_ctx(device)) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    a.nrows = nrows;
    a.dim = dim;
    a.modeord = modeord;
    a.f = (const double2*)f;
    a.s = (const double2*)mode_scale;
    a.out = (double2*)out;
    const int64_t nbx = std::min<int64_t>(kMaxBlocksX, (a.M + kThreads - 1) / kThreads);
    // further rows and mode blocks: strided inside the kernel
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nrows, kMaxGridRows), kMaxWorkgroups / nbx));
    hipLaunchKernelGGL(mode_jet_rows_kernel, dim3((unsigned)nbx, (unsigned)gy), dim3(kThreads), 0, (hipStream_t)stream_, a);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

}  // extern "C"
