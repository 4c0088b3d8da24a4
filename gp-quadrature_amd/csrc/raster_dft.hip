// Type-2 transform from a mode box onto a rectilinear raster, real float64 output:
//
//     out[b, j0..j_{d-1}] = Re sum_k (f[b,k] * mode_scale[k]) * exp(isign * 2 pi i * sum_a h[a] * k_a * (axis_a[j_a] - xcen[a]))
//
// The output points are a tensor product, so the sum separates exactly: per axis a table E_a[j, k] of phases, a complex contraction
// per leading axis (first to last) and, for the last axis, the real GEMM
//
//     out[r, j] = sum_k Tr[r, k] * Er[j, k] - Ti[r, k] * Ei[j, k]            r = (b, j0[, j1]),  K = 2 * m_last
//
// on v_mfma_f64_16x16x4_f64.  Tables and intermediates are padded with zeros to a multiple of 4 modes: the K tail needs no masking.
// Every output element is one chain of additions in mode order (no atomics, no split K), so a call is bitwise repeatable and does
// not depend on how the leading raster axis was cut into slabs (raster_plan_host.cpp).  All index arithmetic is 64-bit.
#include "raster_dft.hpp"

#include <algorithm>

namespace efgp {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kJB = 4;                 // table rows per thread of the contraction kernel: each mode value is loaded once for four outputs
constexpr int kColTiles = 4;           // 16-column tiles per wave of the GEMM: a wave owns 16 x 64 outputs
constexpr int kGemmWaves = 4;          // waves (16-row tiles) per workgroup of the GEMM
constexpr int64_t kMaxBlocks = int64_t(1) << 30;

// the integer frequency stored at `slot` of an axis of m modes
__device__ inline int64_t mode_number(int64_t slot, int64_t m, int modeord) {
    if (modeord) return slot <= (m - 1) / 2 ? slot : slot - m;
    return slot - m / 2;
}

// cos / sin planes (n, Kpad) of exp(isign 2 pi i h k (x[j] - xcen)), k in the stored order, zero for slots m <= s < Kpad.  The
// phase is reduced in turns BEFORE the sine: t = h k dx, its rounding error from the fma, r = t - rint(t), sincospi(2 r).
// by_mode: the planes are stored mode-major, element (j, s) at s * n + j -- the GEMM's operand lanes run along j, and 16 of them
// then share one 128-byte line (row-major they touch 16 lines per load, which bound the kernel at the texture path).
__global__ __launch_bounds__(kThreads) void raster_table_kernel(const double* __restrict__ x, int64_t n, int64_t m, int64_t Kpad, double h,
                                                                 double xcen, int isign, int modeord, int by_mode, double* __restrict__ cosp,
                                                                 double* __restrict__ sinp) {
    const int64_t total = n * Kpad;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const int64_t j = by_mode ? i % n : i / Kpad, s = by_mode ? i / n : i - j * Kpad;
        double c = 0.0, sn = 0.0;
        if (s < m) {
            const double hk = h * (double)mode_number(s, m, modeord);
            const double dx = x[j] - xcen;
            const double t = hk * dx;
            const double lo = fma(hk, dx, -t);
            const double r = (t - rint(t)) + lo;
            sincospi(2.0 * r, &sn, &c);
            if (isign < 0) sn = -sn;
        }
        cosp[i] = c;
        sinp[i] = sn;
    }
}

// d = 1: the GEMM's left operand is the mode rows themselves, scaled and padded: T[b, s] = f[b, s] * scale[s]
__global__ __launch_bounds__(kThreads) void raster_pack_kernel(const double2* __restrict__ f, const double2* __restrict__ scale, int64_t m,
                                                                int64_t Kpad, int64_t rows, double2* __restrict__ T) {
    const int64_t total = rows * Kpad;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const int64_t b = i / Kpad, s = i - b * Kpad;
        double2 v = make_double2(0.0, 0.0);
        if (s < m) {
            v = f[b * m + s];
            if (scale) {
                const double2 w = scale[s];
                v = make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            }
        }
        T[i] = v;
    }
}

// One leading axis:  out[o, j, i] = sum_k in[o, k, i] * scale[k, i] * E[j0 + j, k]   for j < J, i < I, and zero for I <= i < Ipad.
// A workgroup is one (o, group of kJB table rows, 256 values of i): the table entries are uniform over it.
__global__ __launch_bounds__(kThreads) void raster_contract_kernel(const double2* __restrict__ in, const double2* __restrict__ scale,
                                                                    const double* __restrict__ cosp, const double* __restrict__ sinp,
                                                                    int64_t Ktab, int64_t K, int64_t I, int64_t Ipad, int64_t J, int64_t j0,
                                                                    int64_t iblocks, int64_t jgroups, int64_t block0,
                                                                    double2* __restrict__ out) {
    const int64_t blk = block0 + blockIdx.x;
    const int64_t ib = blk % iblocks, rest = blk / iblocks;
    const int64_t jg = rest % jgroups, o = rest / jgroups;
    const int64_t i = ib * kThreads + threadIdx.x;
    if (i >= Ipad) return;
    const int64_t jl = jg * kJB;
    double2 acc[kJB];
#pragma unroll
    for (int q = 0; q < kJB; ++q) acc[q] = make_double2(0.0, 0.0);
    if (i < I) {
        int64_t trow[kJB];
#pragma unroll
        for (int q = 0; q < kJB; ++q) trow[q] = (j0 + std::min<int64_t>(jl + q, J - 1)) * Ktab;      // rows past J: computed, not stored
        const double2* src = in + o * K * I + i;
#pragma unroll 4
        for (int64_t k = 0; k < K; ++k) {                   // unrolled: the loads of four modes in flight; the order of the sums stays
            double2 v = src[k * I];
            if (scale) {
                const double2 w = scale[k * I + i];
                v = make_double2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            }
#pragma unroll
            for (int q = 0; q < kJB; ++q) {
                const double c = cosp[trow[q] + k], s = sinp[trow[q] + k];
                acc[q].x = fma(-v.y, s, fma(v.x, c, acc[q].x));
                acc[q].y = fma(v.y, c, fma(v.x, s, acc[q].y));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kJB; ++q)
        if (jl + q < J) out[(o * J + jl + q) * Ipad + i] = acc[q];
}

// The last axis.  T (R, Kpad) complex, tables mode-major (Kpad, n); a wave owns rows r0 .. r0 + 15 and columns c0 .. c0 + 63 in four
// accumulator tiles.  Operand lanes: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]; result lanes:
// D[row = (lane >> 4) + 4 * reg][col = lane & 15].  Rows and columns past the edge read the last valid one and are not stored.
// Row r of T is raster row (b, rr) = (r / rows_per_batch, r % rows_per_batch): output row b * out_batch_rows + out_row0 + rr.
__global__ __launch_bounds__(64 * kGemmWaves) void raster_gemm_kernel(const double2* __restrict__ T, int64_t R, int64_t Kpad,
                                                                       const double* __restrict__ cosp, const double* __restrict__ sinp,
                                                                       int64_t n, int64_t r_base, int64_t rows_per_batch,
                                                                       int64_t out_batch_rows, int64_t out_row0, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = r_base + ((int64_t)blockIdx.y * kGemmWaves + wave) * kRasterTile;
    if (r0 >= R) return;                                    // wave-uniform; the kernel has no barrier
    const int64_t c0 = (int64_t)blockIdx.x * (kRasterTile * kColTiles);
    const int q = lane >> 4, l16 = lane & 15;
    const int ntile = (int)std::min<int64_t>(kColTiles, (n - c0 + kRasterTile - 1) / kRasterTile);
    const double2* Ap = T + std::min<int64_t>(r0 + l16, R - 1) * Kpad + q;
    int64_t boff[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) boff[t] = std::min<int64_t>(c0 + t * kRasterTile + l16, n - 1) + q * n;
    d4 acc[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int64_t k = 0; k < Kpad; k += kRasterKStep) {      // two steps' operands in flight; one accumulation chain per tile
        const double2 a = Ap[k];
        const double nai = -a.y;
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            if (t < ntile) {
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, cosp[boff[t] + k * n], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai, sinp[boff[t] + k * n], acc[t], 0, 0, 0);
            }
        }
    }
    const bool one_batch = R <= rows_per_batch;             // uniform: no 64-bit division per row where there is one batch
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = r0 + q + 4 * reg;
        if (r >= R) continue;
        const int64_t b = one_batch ? 0 : r / rows_per_batch, rr = r - b * rows_per_batch;
        double* orow = out + (b * out_batch_rows + out_row0 + rr) * n;
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const int64_t j = c0 + t * kRasterTile + l16;
            if (t < ntile && j < n) orow[j] = acc[t][reg];
        }
    }
}

int grid_1d(int64_t work) { return (int)std::max<int64_t>(1, std::min<int64_t>((work + kThreads - 1) / kThreads, 1 << 16)); }

void contract(hipStream_t stream, const double2* in, const double2* scale, const double* cosp, const double* sinp, int64_t Ktab, int64_t outer,
              int64_t K, int64_t I, int64_t Ipad, int64_t J, int64_t j0, double2* out) {
    const int64_t iblocks = (Ipad + kThreads - 1) / kThreads;
    const int64_t jgroups = (J + kJB - 1) / kJB;
    const int64_t blocks = outer * jgroups * iblocks;
    for (int64_t b0 = 0; b0 < blocks; b0 += kMaxBlocks)
        hipLaunchKernelGGL(raster_contract_kernel, dim3((unsigned)std::min(kMaxBlocks, blocks - b0)), dim3(kThreads), 0, stream, in, scale,
                           cosp, sinp, Ktab, K, I, Ipad, J, j0, iblocks, jgroups, b0, out);
}

void gemm(hipStream_t stream, const double2* T, int64_t R, int64_t Kpad, const double* cosp, const double* sinp, int64_t n, int64_t rows_per_batch,
          int64_t out_batch_rows, int64_t out_row0, double* out) {
    const int64_t rows_per_block = kRasterTile * kGemmWaves, max_y = 65535;
    const unsigned gx = (unsigned)((n + kRasterTile * kColTiles - 1) / (kRasterTile * kColTiles));
    for (int64_t r_base = 0; r_base < R; r_base += max_y * rows_per_block) {
        const int64_t gy = std::min(max_y, (R - r_base + rows_per_block - 1) / rows_per_block);
        hipLaunchKernelGGL(raster_gemm_kernel, dim3(gx, (unsigned)gy), dim3(64 * kGemmWaves), 0, stream, T, R, Kpad, cosp, sinp, n, r_base,
                           rows_per_batch, out_batch_rows, out_row0, out);
    }
}

}  // namespace

void raster_table_enqueue(hipStream_t stream, const double* x, int64_t n, int64_t m, int64_t Kpad, double h, double xcen, int isign, int modeord,
                          int by_mode, double* cosp, double* sinp) {
    hipLaunchKernelGGL(raster_table_kernel, dim3(grid_1d(n * Kpad)), dim3(kThreads), 0, stream, x, n, m, Kpad, h, xcen, isign, modeord, by_mode,
                       cosp, sinp);
}

int raster_type2_enqueue(const RasterCall& c, const RasterPlan& plan, void* ws, hipStream_t stream) {
    const int d = c.dim;
    double* base = (double*)ws;
    double* cosp[3] = {nullptr, nullptr, nullptr};
    double* sinp[3] = {nullptr, nullptr, nullptr};
    const double* axis = c.axes;
    for (int a = 0; a < d; ++a) {
        const int64_t plane = c.n[a] * plan.Kpad[a];
        cosp[a] = base;
        sinp[a] = base + plane;
        base += 2 * plane;
        raster_table_enqueue(stream, axis, c.n[a], c.m[a], plan.Kpad[a], c.h[a], c.xcen[a], c.isign, c.modeord, a == d - 1 ? 1 : 0, cosp[a], sinp[a]);
        axis += c.n[a];
    }
    const int64_t B = c.nbatch;
    if (d == 1) {
        double2* T = (double2*)base;
        hipLaunchKernelGGL(raster_pack_kernel, dim3(grid_1d(B * plan.Kpad[0])), dim3(kThreads), 0, stream, c.f, c.scale, c.m[0], plan.Kpad[0], B, T);
        gemm(stream, T, B, plan.Kpad[0], cosp[0], sinp[0], c.n[0], /*rows_per_batch*/ 1, /*out_batch_rows*/ 1, 0, c.out);
        EFGP_HIP_CHECK(hipGetLastError());
        return EFGP_OK;
    }
    double2* T1 = (double2*)base;
    for (int64_t lo = 0; lo < c.n[0]; lo += plan.slab_rows) {
        const int64_t rows = std::min(plan.slab_rows, c.n[0] - lo);
        if (d == 2) {
            contract(stream, c.f, c.scale, cosp[0], sinp[0], plan.Kpad[0], B, c.m[0], c.m[1], plan.Kpad[1], rows, lo, T1);
            gemm(stream, T1, B * rows, plan.Kpad[1], cosp[1], sinp[1], c.n[1], rows, c.n[0], lo, c.out);
        } else {
            const int64_t inner = c.m[1] * c.m[2];
            double2* T2 = T1 + B * plan.slab_rows * inner;
            contract(stream, c.f, c.scale, cosp[0], sinp[0], plan.Kpad[0], B, c.m[0], inner, inner, rows, lo, T1);
            contract(stream, T1, nullptr, cosp[1], sinp[1], plan.Kpad[1], B * rows, c.m[1], c.m[2], plan.Kpad[2], c.n[1], 0, T2);
            gemm(stream, T2, B * rows * c.n[1], plan.Kpad[2], cosp[2], sinp[2], c.n[2], rows * c.n[1], c.n[0] * c.n[1], lo * c.n[1], c.out);
        }
    }
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

}  // namespace efgp

using namespace efgp;

extern "C" {

int efgp_raster_plan(int dim, const int64_t* n_modes, const int64_t* n_axis, int nbatch, int64_t max_workspace_bytes, int64_t* slab_rows_out,
                     int64_t* slabs_out, int64_t* workspace_bytes_out) {
    RasterPlan p;
    const int rc = plan_raster(dim, n_modes, n_axis, nbatch, max_workspace_bytes, &p);
    if (rc != EFGP_OK) return rc;
    if (slab_rows_out) *slab_rows_out = p.slab_rows;
    if (slabs_out) *slabs_out = p.slabs;
    if (workspace_bytes_out) *workspace_bytes_out = p.workspace_bytes;
    return EFGP_OK;
}

int efgp_raster_type2(int device, int dim, const int64_t* n_modes, const double* h, const double* xcen_host, const int64_t* n_axis,
                      const double* axes, const void* f, const void* mode_scale, int nbatch, int isign, int modeord, double* out,
                      int64_t max_workspace_bytes, void* stream_) {
    EFGP_REQUIRE(isign == 1 || isign == -1, "efgp_raster_type2: isign must be +1 or -1");
    EFGP_REQUIRE(modeord == 0 || modeord == 1, "efgp_raster_type2: modeord must be 0 or 1");
    RasterPlan plan;
    const int rc = plan_raster(dim, n_modes, n_axis, nbatch, max_workspace_bytes, &plan);
    if (rc != EFGP_OK) return rc;
    EFGP_REQUIRE(h && axes && f && out, "efgp_raster_type2: null argument");
    RasterCall c;
    c.dim = dim;
    for (int a = 0; a < dim; ++a) {
        c.m[a] = n_modes[a];
        c.n[a] = n_axis[a];
        c.h[a] = h[a];
        c.xcen[a] = xcen_host ? xcen_host[a] : 0.0;
    }
    c.axes = axes;
    c.f = (const double2*)f;
    c.scale = (const double2*)mode_scale;
    c.nbatch = nbatch;
    c.isign = isign;
    c.modeord = modeord;
    c.out = out;
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    void* ws = pool_alloc(ctx, (size_t)plan.workspace_bytes);
    if (!ws) return EFGP_ENOMEM;
    const int rc2 = raster_type2_enqueue(c, plan, ws, (hipStream_t)stream_);
    pool_free(ctx, ws, (size_t)plan.workspace_bytes);      // reused in stream order, behind the launches above
    return rc2;
}

}  // extern "C"
