// Type-1 transform from a rectilinear raster onto a mode box, the adjoint of raster_dft.hip:
//
//     out[b, k0..k_{d-1}] = sum_j values[b, j] * cell_scale[j] * exp(isign * 2 pi i * sum_a h[a] * k_a * (axis_a[j_a] - xcen[a]))
//
// The stages of the type-2 transform in reverse.  The last, contiguous raster axis is contracted first by the real GEMM
//
//     T[r, k] = sum_j V[r, j] * (cos, sin)[j, k]                r = (b, j0[, j1]),  K = n_last,  columns = m_last
//
// on v_mfma_f64_16x16x4_f64 (a last axis longer than kRasterSegment cells in segments of that length, added in order, so that a
// raster of few rows still fills the machine); then each leading axis (complex, n_a -> m_a) with VALU fma.  The leading raster axis is the long
// reduction with few outputs: it is split into partial sums over kRasterChunk rows, added in chunk order by a second kernel.  The
// chunk is a constant and a slab is a whole number of chunks, so every output is one fixed sequence of additions: no atomics, a
// call is bitwise repeatable and does not depend on how the leading axis was cut into slabs (raster_plan_host.cpp).  All index
// arithmetic is 64-bit.
#include "raster_dft.hpp"

#include <algorithm>

namespace efgp {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kReduceThreads = 64;     // values of i per workgroup of the leading-axis kernels
constexpr int kKB = 4;                 // modes per thread of the leading-axis contraction: each value is loaded once for four outputs
constexpr int kColTiles = 4;           // 16-column tiles per wave of the GEMM: a wave owns 16 rows x 64 modes, cos and sin
constexpr int kGemmWaves = 4;          // waves (16-row tiles) per workgroup of the GEMM
constexpr int kGemmK = 4 * kRasterKStep;   // raster cells per trip of the GEMM: four instructions per tile and plane
constexpr int64_t kMaxBlocks = int64_t(1) << 30;

// The last axis.  Row r of the slab is raster row (b, rr) = (r / rows_per_batch, r % rows_per_batch): its values start at
// values + (b * batch_rows + row0 + rr) * n, its scales at scale + (row0 + rr) * n.  A wave owns rows r0 .. r0 + 15 and modes
// c0 .. c0 + 63 in four pairs of accumulator tiles.  Operand lanes of the instruction (the f64 map): A[row = lane & 15][k = lane >> 4],
// B[k = lane >> 4][col = lane & 15]; results D[row = (lane >> 4) + 4 * reg][col = lane & 15].  A lane loads FOUR consecutive
// cells of its row per trip -- cell jb + 4 (lane >> 4) + s feeds instruction s -- so the 64 lanes read 128 contiguous bytes of each
// of 16 rows, and the row-major tables give the B operand 16 consecutive modes of one cell: four lines per load.  The order of the
// cells within a trip is the same on both operands, which is all the sum needs.  Scale and selection are applied as the value
// is loaded; cells past the end of the row and masked cells enter as +0, whatever the memory holds.  Rows and columns past
// the edge read the last valid one and are not stored.
// A long last axis is cut into S segments of kRasterSegment cells, one per workgroup column: segment `seg` of row r is written to
// row r * S + seg of T, and raster_adjoint_sum_kernel adds the segments in order.  S depends on the axis length alone.
__global__ __launch_bounds__(64 * kGemmWaves) void raster_adjoint_gemm_kernel(const double* __restrict__ values, const double* __restrict__ scale,
                                                                               int64_t n, int64_t R, int64_t r_base, int64_t rows_per_batch,
                                                                               int64_t batch_rows, int64_t row0, const double* __restrict__ cosp,
                                                                               const double* __restrict__ sinp, int64_t Kpad, int64_t m,
                                                                               int64_t strips, int64_t S, int64_t seg_base,
                                                                               double2* __restrict__ T) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = r_base + ((int64_t)blockIdx.y * kGemmWaves + wave) * kRasterTile;
    if (r0 >= R) return;                                    // wave-uniform; the kernel has no barrier
    const int64_t seg = seg_base + blockIdx.x / strips;
    const int64_t c0 = (int64_t)(blockIdx.x % strips) * (kRasterTile * kColTiles);
    const int64_t jlo = seg * kRasterSegment, jhi = std::min<int64_t>(n, jlo + kRasterSegment);
    const int q = lane >> 4, l16 = lane & 15;
    const int ntile = (int)std::min<int64_t>(kColTiles, (Kpad - c0 + kRasterTile - 1) / kRasterTile);
    const int64_t r = std::min<int64_t>(r0 + l16, R - 1);
    const int64_t b = R <= rows_per_batch ? 0 : r / rows_per_batch, rr = r - b * rows_per_batch;
    const double* vp = values + (b * batch_rows + row0 + rr) * n;
    const double* sp = scale ? scale + (row0 + rr) * n : nullptr;
    int64_t col[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) col[t] = std::min<int64_t>(c0 + t * kRasterTile + l16, Kpad - 1);
    d4 accc[kColTiles], accs[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) accc[t] = accs[t] = d4{0.0, 0.0, 0.0, 0.0};
    for (int64_t jb = jlo; jb < jhi; jb += kGemmK) {
        double a[kRasterKStep];
        int64_t trow[kRasterKStep];
#pragma unroll
        for (int s = 0; s < kRasterKStep; ++s) {
            const int64_t j = jb + kRasterKStep * q + s, jc = std::min<int64_t>(j, jhi - 1);
            double v = vp[jc];
            if (sp) {
                const double w = sp[jc];
                v = w != 0.0 ? v * w : 0.0;                 // selected out, not multiplied by zero: the cell may hold NaN
            }
            a[s] = j < jhi ? v : 0.0;
            trow[s] = jc * Kpad;
        }
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            if (t < ntile) {
#pragma unroll
                for (int s = 0; s < kRasterKStep; ++s) {
                    accc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], cosp[trow[s] + col[t]], accc[t], 0, 0, 0);
                    accs[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], sinp[trow[s] + col[t]], accs[t], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t ro = r0 + q + 4 * reg;
        if (ro >= R) continue;
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const int64_t k = c0 + t * kRasterTile + l16;
            if (t < ntile && k < m) T[(ro * S + seg) * m + k] = make_double2(accc[t][reg], accs[t][reg]);
        }
    }
}

// One leading axis, one chunk c of L raster rows per workgroup row:
//     out[(o * C + c), k, i] = sum_{j = c L}^{min(J, (c + 1) L) - 1} in[o, j, i] * E[j0 + j, k]          k < m, i < I
// A workgroup is one (o, c, group of kKB modes, kReduceThreads values of i): the table entries are uniform over it.  The table
// is row-major (rows of Ktab >= m doubles, zero past m); a group of modes never reaches past Ktab (both are multiples of four).
__global__ __launch_bounds__(kReduceThreads) void raster_adjoint_contract_kernel(const double2* __restrict__ in, const double* __restrict__ cosp,
                                                                                  const double* __restrict__ sinp, int64_t Ktab, int64_t m,
                                                                                  int64_t I, int64_t J, int64_t j0, int64_t L, int64_t C,
                                                                                  int64_t iblocks, int64_t kgroups, int64_t block0,
                                                                                  double2* __restrict__ out) {
    const int64_t blk = block0 + blockIdx.x;
    const int64_t ib = blk % iblocks, rest = blk / iblocks;
    const int64_t kg = rest % kgroups, rest2 = rest / kgroups;
    const int64_t c = rest2 % C, o = rest2 / C;
    const int64_t i = ib * kReduceThreads + threadIdx.x;
    if (i >= I) return;
    const int64_t kl = kg * kKB;
    const int64_t jbeg = c * L, jend = std::min<int64_t>(J, jbeg + L);
    double2 acc[kKB];
#pragma unroll
    for (int q = 0; q < kKB; ++q) acc[q] = make_double2(0.0, 0.0);
    const double2* src = in + o * J * I + i;
#pragma unroll 4
    for (int64_t j = jbeg; j < jend; ++j) {                 // unrolled: four rows' loads in flight; the order of the sums stays
        const double2 v = src[j * I];
        const int64_t trow = (j0 + j) * Ktab + kl;
#pragma unroll
        for (int q = 0; q < kKB; ++q) {
            const double cs = cosp[trow + q], sn = sinp[trow + q];
            acc[q].x = fma(-v.y, sn, fma(v.x, cs, acc[q].x));
            acc[q].y = fma(v.y, cs, fma(v.x, sn, acc[q].y));
        }
    }
#pragma unroll
    for (int q = 0; q < kKB; ++q)
        if (kl + q < m) out[((o * C + c) * m + kl + q) * I + i] = acc[q];
}

// out[b, e] = (first ? 0 : out[b, e]) + part[b, 0, e] + part[b, 1, e] + ..: the chunks of one slab in order, behind those of the
// slabs before it.  One thread per output, one chain of additions per output.
__global__ __launch_bounds__(kReduceThreads) void raster_adjoint_sum_kernel(const double2* __restrict__ part, int64_t C, int64_t M, int64_t total,
                                                                             int first, double2* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * kReduceThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kReduceThreads) {
        const int64_t b = e / M, k = e - b * M;
        double2 acc = first ? make_double2(0.0, 0.0) : out[e];
        const double2* src = part + b * C * M + k;
        for (int64_t c = 0; c < C; ++c) {
            const double2 v = src[c * M];
            acc.x += v.x;
            acc.y += v.y;
        }
        out[e] = acc;
    }
}

void sum_parts(hipStream_t stream, const double2* part, int64_t C, int64_t M, int64_t total, int first, double2* out) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((total + kReduceThreads - 1) / kReduceThreads, 1 << 16));
    hipLaunchKernelGGL(raster_adjoint_sum_kernel, dim3(grid), dim3(kReduceThreads), 0, stream, part, C, M, total, first, out);
}

// T (R, m_last) from the raster rows; `seg_buf` (R, S, m_last) holds the segments of a last axis longer than kRasterSegment.
void gemm(hipStream_t stream, const RasterAdjointCall& c, const RasterPlan& plan, int64_t R, int64_t rows_per_batch, int64_t batch_rows, int64_t row0,
          const double* cosp, const double* sinp, double2* seg_buf, double2* T) {
    const int a = c.dim - 1;
    const int64_t S = raster_segments(c.n[a]);
    double2* dst = S > 1 ? seg_buf : T;
    const int64_t rows_per_block = kRasterTile * kGemmWaves, max_y = 65535;
    const int64_t strips = (plan.Kpad[a] + kRasterTile * kColTiles - 1) / (kRasterTile * kColTiles);
    const int64_t segs_per_launch = std::max<int64_t>(1, kMaxBlocks / strips);
    for (int64_t r_base = 0; r_base < R; r_base += max_y * rows_per_block) {
        const int64_t gy = std::min(max_y, (R - r_base + rows_per_block - 1) / rows_per_block);
        for (int64_t seg_base = 0; seg_base < S; seg_base += segs_per_launch) {
            const int64_t segs = std::min(segs_per_launch, S - seg_base);
            hipLaunchKernelGGL(raster_adjoint_gemm_kernel, dim3((unsigned)(strips * segs), (unsigned)gy), dim3(64 * kGemmWaves), 0, stream, c.values,
                               c.cell_scale, c.n[a], R, r_base, rows_per_batch, batch_rows, row0, cosp, sinp, plan.Kpad[a], c.m[a], strips, S,
                               seg_base, dst);
        }
    }
    if (S > 1) sum_parts(stream, seg_buf, S, c.m[a], R * c.m[a], 1, T);
}

void contract(hipStream_t stream, const double2* in, const double* cosp, const double* sinp, int64_t Ktab, int64_t m, int64_t outer, int64_t I,
              int64_t J, int64_t j0, int64_t L, double2* out) {
    const int64_t C = (J + L - 1) / L;
    const int64_t iblocks = (I + kReduceThreads - 1) / kReduceThreads;
    const int64_t kgroups = (m + kKB - 1) / kKB;
    const int64_t blocks = outer * C * kgroups * iblocks;
    for (int64_t b0 = 0; b0 < blocks; b0 += kMaxBlocks)
        hipLaunchKernelGGL(raster_adjoint_contract_kernel, dim3((unsigned)std::min(kMaxBlocks, blocks - b0)), dim3(kReduceThreads), 0, stream, in,
                           cosp, sinp, Ktab, m, I, J, j0, L, C, iblocks, kgroups, b0, out);
}

}  // namespace

int raster_type1_enqueue(const RasterAdjointCall& c, const RasterPlan& plan, void* ws, hipStream_t stream) {
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
        raster_table_enqueue(stream, axis, c.n[a], c.m[a], plan.Kpad[a], c.h[a], c.xcen[a], c.isign, c.modeord, /*by_mode*/ 0, cosp[a], sinp[a]);
        axis += c.n[a];
    }
    const int64_t B = c.nbatch;
    if (d == 1) {
        gemm(stream, c, plan, B, /*rows_per_batch*/ 1, /*batch_rows*/ 1, 0, cosp[0], sinp[0], (double2*)base, c.out);
        EFGP_HIP_CHECK(hipGetLastError());
        return EFGP_OK;
    }
    const int64_t inner = d == 2 ? c.m[1] : c.m[1] * c.m[2];          // modes behind the leading axis
    const int64_t M = c.m[0] * inner;
    double2* T1 = (double2*)base;
    for (int64_t lo = 0; lo < c.n[0]; lo += plan.slab_rows) {
        const int64_t rows = std::min(plan.slab_rows, c.n[0] - lo);
        const int64_t chunks = (rows + kRasterChunk - 1) / kRasterChunk;
        double2* lead = T1;                                         // (B, rows, inner): what the leading axis contracts
        double2* part;
        if (d == 2) {
            part = T1 + B * plan.slab_rows * c.m[1];
            double2* seg_buf = part + B * (plan.slab_rows / kRasterChunk) * M;
            gemm(stream, c, plan, B * rows, rows, c.n[0], lo, cosp[1], sinp[1], seg_buf, T1);
        } else {
            double2* T2 = T1 + B * plan.slab_rows * c.n[1] * c.m[2];
            part = T2 + B * plan.slab_rows * inner;
            double2* seg_buf = part + B * (plan.slab_rows / kRasterChunk) * M;
            gemm(stream, c, plan, B * rows * c.n[1], rows * c.n[1], c.n[0] * c.n[1], lo * c.n[1], cosp[2], sinp[2], seg_buf, T1);
            contract(stream, T1, cosp[1], sinp[1], plan.Kpad[1], c.m[1], B * rows, c.m[2], c.n[1], 0, /*one chunk*/ c.n[1], T2);
            lead = T2;
        }
        contract(stream, lead, cosp[0], sinp[0], plan.Kpad[0], c.m[0], B, inner, rows, lo, kRasterChunk, part);
        sum_parts(stream, part, chunks, M, B * M, lo == 0 ? 1 : 0, c.out);
    }
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

}  // namespace efgp

using namespace efgp;

extern "C" {

int efgp_raster_type1_plan(int dim, const int64_t* n_modes, const int64_t* n_axis, int nbatch, int64_t max_workspace_bytes, int64_t* slab_rows_out,
                           int64_t* slabs_out, int64_t* workspace_bytes_out) {
    RasterPlan p;
    const int rc = plan_raster_type1(dim, n_modes, n_axis, nbatch, max_workspace_bytes, &p);
    if (rc != EFGP_OK) return rc;
    if (slab_rows_out) *slab_rows_out = p.slab_rows;
    if (slabs_out) *slabs_out = p.slabs;
    if (workspace_bytes_out) *workspace_bytes_out = p.workspace_bytes;
    return EFGP_OK;
}

int efgp_raster_type1(int device, int dim, const int64_t* n_modes, const double* h, const double* xcen_host, const int64_t* n_axis,
                      const double* axes, const double* values, const double* cell_scale, int nbatch, int isign, int modeord, void* out,
                      int64_t max_workspace_bytes, void* stream_) {
    EFGP_REQUIRE(isign == 1 || isign == -1, "efgp_raster_type1: isign must be +1 or -1");
    EFGP_REQUIRE(modeord == 0 || modeord == 1, "efgp_raster_type1: modeord must be 0 or 1");
    RasterPlan plan;
    const int rc = plan_raster_type1(dim, n_modes, n_axis, nbatch, max_workspace_bytes, &plan);
    if (rc != EFGP_OK) return rc;
    EFGP_REQUIRE(h && axes && values && out, "efgp_raster_type1: null argument");
    RasterAdjointCall c;
    c.dim = dim;
    for (int a = 0; a < dim; ++a) {
        c.m[a] = n_modes[a];
        c.n[a] = n_axis[a];
        c.h[a] = h[a];
        c.xcen[a] = xcen_host ? xcen_host[a] : 0.0;
    }
    c.axes = axes;
    c.values = values;
    c.cell_scale = cell_scale;
    c.nbatch = nbatch;
    c.isign = isign;
    c.modeord = modeord;
    c.out = (double2*)out;
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    void* ws = pool_alloc(ctx, (size_t)plan.workspace_bytes);
    if (!ws) return EFGP_ENOMEM;
    const int rc2 = raster_type1_enqueue(c, plan, ws, (hipStream_t)stream_);
    pool_free(ctx, ws, (size_t)plan.workspace_bytes);      // reused in stream order, behind the launches above
    return rc2;
}

}  // extern "C"
