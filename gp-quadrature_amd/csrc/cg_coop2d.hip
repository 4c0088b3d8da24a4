// The cooperative single-launch CG solve of the 2-D grids 96^2 .. 512^2: the general and the Hermitian kernel, and the host side
// that picks the kernel of a launch shape, lays out the scratch and enqueues the launches (coop_enqueue).
// The operator object, its spectra and the dispatch of a solve: toeplitz_cg.hip.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

#include "cg_plan_host.hpp"
#include "common.hpp"
#include "toeplitz_cg.hpp"
#include "toeplitz_line_dev.hpp"
#include "toeplitz_op.hpp"

namespace efgp {

// ==========================================================================================================
// Cooperative single-launch solve for the same 2-D grids: the WHOLE CG loop in one kernel spread over G workgroups
// (one per CU) per system, with grid barriers between the phases instead of kernel boundaries -- no launch latency
// (3-4 us x 4 launches per iteration above), no host poll, no hipGraph.
//   phase R  : own rows  -- ws .* p (from registers), zero-padded, forward FFT along dim 1           -> B1 (write-through)
//   barrier
//   phase C  : own column block -- forward FFT along dim 0 of the n non-zero inputs, .* vhat, inverse, crop rows -> B2
//   barrier
//   phase Ri : own rows  -- inverse FFT along dim 1, crop, A p (registers), partial <p, A p>
//   barrier  : every workgroup adds the G partials in index order (same bits everywhere: uniform control flow)
//   update   : own rows  -- x, r, z in registers, partial <r,r>, <r,z>
//   barrier  : sums, stopping rule, beta, p
// Ownership is fixed for the whole solve: workgroup g owns rows [g L, (g+1) L) of the mode block in the row phases and
// the vector elements of those rows (x, r, p, A p, ws, diag stay in ITS registers: 4 per thread), and columns
// [g c, (g+1) c) in the column phase.  Only B1, B2 and the partial sums cross workgroups; they are written and read
// with agent-scope accesses (write-through stores / cache-bypassing loads: the XCDs' L2 caches are not coherent with
// each other), so a barrier needs no cache write-back or invalidate: the stores are waited for (s_waitcnt) before the
// workgroup's arrival is counted.  A barrier is one agent-scope atomic add on a monotone counter and a bounded poll;
// a poll that runs out (a co-resident workgroup never arrived) sets a status flag on which every workgroup leaves and
// the host falls back to the multi-launch iteration above.  All G x systems workgroups must be resident at once:
// the host launches at most one workgroup per CU.
// ==========================================================================================================
constexpr int kCoopSlots = 4;                 // vector elements per thread (own rows x n1 <= 4 x 256)
constexpr unsigned kCoopPollLimit = 1u << 22; // ~ seconds of polling before a barrier is declared dead

struct CoopArgs {
    ToepGeom g;
    const double2* ws;
    const double* diag;
    const double* diag_scale;  // when diag is null and this is not: Jacobi diagonal (*diag_scale) |ws|^2 + sigmasq (device scalar)
    int b_times_ws;           // right-hand side is ws .* b (the fit's D F*y, efgpnd.py:792)
    int zero_x0;              // x0 = 0: x is output only, the initial operator application is skipped (A 0 = 0)
    double sigmasq;
    int variant;
    double tol;
    int early_stop;
    int batched;
    int max_iter;
    const double2* b;         // [systems][M]
    double2* x;               // in: x0 (unless zero_x0), out: solution
    const double2* vhat;
    const double2* tw0;
    const double2* tw1;
    double2* b1;              // [systems][n0][F1]
    double2* b2;              // [systems][n0][F1]
    double2* b3;              // [systems][n0][F1]  (Hermitian kernel: row transforms of the current direction)
    int spec_lds;             // Hermitian kernel: the workgroup's slice of the spectrum lives in LDS (cols_wg == lpbc)
    double* partial;          // [systems][3][kCoopMaxG]
    unsigned* bar;            // [systems] arrival counters, 64 bytes apart, zero at launch
    int* iters;               // [systems]
    int* status;              // [0] != 0: a barrier timed out
    int nan_on_dead;          // asynchronous entries: a system whose barrier died gets NaN in x (nobody may mistake x0 for a solution)
    double* hist;
    int hist_cap;
    int G;                    // workgroups per system
    int bar_need;             // arrivals a barrier waits for: G (G + 1 under the test hook EFGP_COOP_TEST_DEAD: every barrier dies)
    int rows_wg;              // rows of the mode block owned per workgroup (ceil(n0 / G))
    int cols_wg;              // columns owned per workgroup (F1 / G)
    int lines;                // rows per LDS pass of the row phases
    int lpbc;                 // columns per LDS pass of the column phase (a power of two)
    int dbg;                  // EFGP_COOP_DBG=2: cycle counters per phase (workgroup 0 of system 0)
    double* stamps;
};

// w / F for w < 2^16 and the line lengths of these kernels (96 .. 512) through one multiply-high: magic = floor(2^32 / F) + 1 is
// exact on that range (F w < 2^32 / F); the loops that scatter rows into LDS images and back did a full integer division per
// element (~40 instructions each, 16 per thread and phase)
__device__ __forceinline__ int coop_div(int w, unsigned magic) { return (int)__umulhi((unsigned)w, magic); }

// Jacobi diagonal entry t of the cooperative kernels: explicit array, or scale |ws_t|^2 + sigmasq with the two roundings of the
// reference's torch expression (efgpnd.py:795-799; pcg::jacobi_entry), or 1
__device__ __forceinline__ double coop_jacobi(const CoopArgs& a, double2 w, int64_t t) {
    if (a.diag) return a.diag[t];
    if (a.diag_scale) return __dadd_rn(__dmul_rn(*a.diag_scale, __dadd_rn(__dmul_rn(w.x, w.x), __dmul_rn(w.y, w.y))), a.sigmasq);
    return 1.0;
}

// SOLO (G == 1): the intermediate grids are private to the workgroup -- ordinary cached accesses, no grid barrier
template <bool SOLO>
__device__ __forceinline__ void store_x2(double2* p, double2 v) {
    if (SOLO) {
        *p = v;
    } else {
        __hip_atomic_store(&p->x, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&p->y, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <bool SOLO>
__device__ __forceinline__ double2 load_x2(const double2* p) {
    if (SOLO) return *p;
    return make_double2(__hip_atomic_load(&p->x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                        __hip_atomic_load(&p->y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// returns false (in every thread of the workgroup) when the barrier is dead
__device__ __forceinline__ bool coop_barrier(unsigned* bar, unsigned& epoch, int G, int* status, int* sflag) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);                       // this thread's write-through stores have been acknowledged
    __syncthreads();
    ++epoch;
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = epoch * (unsigned)G;
        int ok = 1;
        unsigned polls = 0;
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            ++polls;
            if (polls > kCoopPollLimit || ((polls & 255u) == 0u && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                ok = 0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *sflag = ok;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return *sflag != 0;
}

// KS: vector elements per thread (owned rows x n1 <= KS x 256).  Two launch shapes (chosen by the host):
//   latency  (few systems)  : G = F1 / lpbc workgroups per system, one row pass and one column pass per phase, KS = 4
//   throughput (many systems): as few workgroups per system as the registers allow (G = 1: no grid barrier at all, the
//                              intermediate grids stay in this CU's caches), several LDS passes per phase, KS = 8
template <int KS, bool SOLO>
__global__ __launch_bounds__(kLineThreads) void cg_coop2d_kernel(CoopArgs a) {
    extern __shared__ double2 lsm[];
    __shared__ double red[kLineThreads / 64];
    __shared__ double fin[3 * kCoopMaxG];
    __shared__ int sflag;
    const int tid = threadIdx.x, wg = blockIdx.x, sys = blockIdx.y, G = a.G;
    const int n0 = (int)a.g.n[0], n1 = (int)a.g.n[1], F0 = (int)a.g.F[0], F1 = (int)a.g.F[1];
    const int ldr = F1 + 1, ldc = F0 + 1;
    const int lgC = ilog2(a.lpbc);
    const unsigned magicF1 = 0xFFFFFFFFu / (unsigned)F1 + 1u, magicZ = 0xFFFFFFFFu / (unsigned)max(1, F1 - n1) + 1u;
    const int bufsz = max(a.lines * ldr, a.lpbc * ldc);
    double2* A = lsm;
    double2* B = lsm + bufsz;
    double2* tw1s = B + bufsz;
    double2* tw0s = F0 == F1 ? tw1s : tw1s + F1;
    load_twiddles(tw1s, a.tw1, F1);
    if (F0 != F1) load_twiddles(tw0s, a.tw0, F0);
    __syncthreads();
    const int64_t M = a.g.M;
    const int r0 = wg * a.rows_wg;
    const int nrows = max(0, min(a.rows_wg, n0 - r0));      // rows owned (0 for trailing workgroups)
    const int cnt = nrows * n1;
    const int64_t base = (int64_t)sys * M + (int64_t)r0 * n1;    // the owned elements are contiguous in the flat vector
    const int c_lo = wg * a.cols_wg;
    double2* b1 = a.b1 + (int64_t)sys * n0 * F1;
    double2* b2 = a.b2 + (int64_t)sys * n0 * F1;
    double* part = a.partial + (int64_t)sys * 3 * kCoopMaxG;
    unsigned* bar = a.bar + (int64_t)sys * 16;
    unsigned epoch = 0;
    long long st_prev = (long long)__builtin_readcyclecounter();
#define COOP_STAMP(slot_)                                                                     \
    do {                                                                                      \
        if (a.dbg == 2 && wg == 0 && sys == 0 && tid == 0) {                                  \
            const long long now_ = (long long)__builtin_readcyclecounter();                   \
            a.stamps[slot_] += (double)(now_ - st_prev);                                      \
            st_prev = now_;                                                                   \
        }                                                                                     \
    } while (0)

    double2 xv[KS], rv[KS], pv[KS], wsv[KS];
    double dg[KS];
    int lrow[KS], lcol[KS];                              // owned element s: row r0 + lrow[s], column lcol[s] of the mode block
    bool ok[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int e = tid + s * kLineThreads;
        ok[s] = e < cnt;
        lrow[s] = ok[s] ? e / n1 : 0;
        lcol[s] = ok[s] ? e - lrow[s] * n1 : 0;
        if (ok[s]) {
            const int t = r0 * n1 + e;
            xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x[base + e];
            wsv[s] = a.ws[t];
            dg[s] = coop_jacobi(a, wsv[s], t);
        } else {
            xv[s] = wsv[s] = make_double2(0.0, 0.0);
            dg[s] = 1.0;
        }
        rv[s] = pv[s] = make_double2(0.0, 0.0);
    }
    auto sync_grid = [&]() __attribute__((always_inline)) -> bool {
        if (SOLO) {
            __syncthreads();
            return true;
        }
        return coop_barrier(bar, epoch, a.bar_need, a.status, &sflag);
    };

    // Au = A u for the owned elements; false when a barrier died
    // sum of K (<= 2) per-workgroup partials over the G (<= 64) workgroups, the same bits in every workgroup: both values go
    // through ONE workgroup reduction (fixed shuffle tree, then the four wave sums in order), and every wave then loads the G
    // partials into its lanes and reduces them with the same fixed butterfly -- no LDS staging, no serial chain of G adds.
    // `slot0`: first of the three partial arrays used -- consecutive sums must use DIFFERENT arrays (a fast workgroup writes
    // its next partial while a slow one still reads the previous sum's: no barrier sits between a sum's reads and the next
    // sum's writes)
    auto all_sum = [&](double (&v)[3], int K, int slot0) __attribute__((always_inline)) -> bool {
        double a0 = v[0], a1 = K > 1 ? v[1] : 0.0;
        for (int off = 32; off > 0; off >>= 1) {
            a0 += __shfl_down(a0, off, 64);
            a1 += __shfl_down(a1, off, 64);
        }
        const int lane = tid & 63, wid = tid >> 6;
        __syncthreads();
        if (lane == 0) {
            red[wid] = a0;
            fin[wid] = a1;
        }
        __syncthreads();
        a0 = ((red[0] + red[1]) + red[2]) + red[3];
        a1 = ((fin[0] + fin[1]) + fin[2]) + fin[3];
        if (SOLO) {
            v[0] = a0;
            v[1] = a1;
            __syncthreads();
            return true;
        }
        if (tid == 0) {
            __hip_atomic_store(&part[slot0 * kCoopMaxG + wg], a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (K > 1) __hip_atomic_store(&part[(slot0 + 1) * kCoopMaxG + wg], a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!coop_barrier(bar, epoch, a.bar_need, a.status, &sflag)) return false;
        double b0 = lane < G ? __hip_atomic_load(&part[slot0 * kCoopMaxG + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        double b1 = (K > 1 && lane < G) ? __hip_atomic_load(&part[(slot0 + 1) * kCoopMaxG + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        for (int off = 32; off > 0; off >>= 1) {
            b0 += __shfl_xor(b0, off, 64);
            b1 += __shfl_xor(b1, off, 64);
        }
        v[0] = b0;
        v[1] = b1;
        return true;
    };
    // <u, A u> comes out of the operator application itself: sigma^2 |u|^2 (own rows, phase R) + sum_f Re(vhat_c) |FFT(ws u)|^2 (own
    // columns, phase C; Parseval with the CENTRED spectrum vhat_c = vhat . e^(2 pi i f (n-1)/F), whose circular convolution has its
    // crop window at [0, n)), reduced over the workgroups ON the barrier between phases C and Ri -- the separate <p, A p> barrier
    // and all-reduce of an iteration are gone (3 grid barriers instead of 4)
    auto apply = [&](const double2 (&u)[KS], double2 (&Au)[KS], double& uAu) __attribute__((always_inline)) -> bool {
        double pp = 0.0, cs = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) pp += u[s].x * u[s].x + u[s].y * u[s].y;
        // R: owned rows in passes of a.lines
        for (int p0 = 0; p0 < nrows; p0 += a.lines) {
            const int nl = min(a.lines, nrows - p0);
            // zero padding behind the n1 inputs of each row, all rows of the pass as one index range (a loop over the rows left
            // all but F1 - n1 threads idle in each of its trips: 8.4 k of the 100 k ticks of a 96 x 96 iteration)
            const int zw = F1 - n1;
            for (int e = tid; e < nl * zw; e += kLineThreads) {
                const int l = coop_div(e, magicZ);
                A[l * ldr + n1 + (e - l * zw)] = make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (ok[s] && lrow[s] >= p0 && lrow[s] < p0 + nl) A[(lrow[s] - p0) * ldr + lcol[s]] = cmul(u[s], wsv[s]);
            __syncthreads();
            COOP_STAMP(12);
            const double2* X = line_fft_fast(A, B, F1, ldr, nl, tw1s);
            COOP_STAMP(13);
            for (int w = tid; w < nl * F1; w += kLineThreads) {
                const int l = coop_div(w, magicF1), i1 = w - l * F1;
                store_x2<SOLO>(b1 + (int64_t)(r0 + p0 + l) * F1 + i1, X[l * ldr + i1]);
            }
            __syncthreads();                                                  // the next pass refills the buffers
        }
        COOP_STAMP(0);
        if (!sync_grid()) return false;
        COOP_STAMP(1);
        // C: owned columns in passes of a.lpbc
        for (int c0 = c_lo; c0 < c_lo + a.cols_wg; c0 += a.lpbc) {
            // every thread's loads are issued before the first is consumed (one at a time costs a memory round trip each)
            double2 tmp[kCoopLoads];
#pragma unroll
            for (int q = 0; q < kCoopLoads; ++q) {
                const int w = tid + q * kLineThreads, i0 = w >> lgC;
                tmp[q] = (w < (F0 << lgC) && i0 < n0) ? load_x2<SOLO>(b1 + (int64_t)i0 * F1 + c0 + (w & (a.lpbc - 1))) : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int q = 0; q < kCoopLoads; ++q) {
                const int w = tid + q * kLineThreads;
                if (w < (F0 << lgC)) A[(w & (a.lpbc - 1)) * ldc + (w >> lgC)] = tmp[q];
            }
            __syncthreads();
            COOP_STAMP(8);
            // forward transform, .* vhat and the conjugation in front of the inverse transform on the result registers
            double2* X = line_fft_fast_mul(A, B, F0, ldc, a.lpbc, tw0s, a.vhat + c0, F1, cs);
            double2* Y = X == A ? B : A;
            COOP_STAMP(9);
            COOP_STAMP(10);
            const double2* Z = line_fft_fast(X, Y, F0, ldc, a.lpbc, tw0s);
            COOP_STAMP(11);
            for (int w = tid; w < (n0 << lgC); w += kLineThreads) {
                const int j = w >> lgC, l = w & (a.lpbc - 1);
                const double2 z = Z[l * ldc + j];
                store_x2<SOLO>(b2 + (int64_t)j * F1 + c0 + l, make_double2(z.x, -z.y));
            }
            __syncthreads();
        }
        COOP_STAMP(2);
        {
            double t3[3] = {a.variant == 0 ? a.sigmasq * pp + cs : pp + cs / a.sigmasq, 0.0, 0.0};
            if (!all_sum(t3, 1, 2)) return false;
            uAu = t3[0];
        }
        COOP_STAMP(3);
        // Ri: owned rows in passes
#pragma unroll
        for (int s = 0; s < KS; ++s) Au[s] = make_double2(0.0, 0.0);
        for (int p0 = 0; p0 < nrows; p0 += a.lines) {
            const int nl = min(a.lines, nrows - p0);
            double2 tmp[kCoopLoads];
#pragma unroll
            for (int q = 0; q < kCoopLoads; ++q) {
                const int w = tid + q * kLineThreads;
                tmp[q] = w < nl * F1 ? load_x2<SOLO>(b2 + (int64_t)(r0 + p0) * F1 + w) : make_double2(0.0, 0.0);   // rows are contiguous
            }
#pragma unroll
            for (int q = 0; q < kCoopLoads; ++q) {
                const int w = tid + q * kLineThreads;
                if (w < nl * F1) A[(w / F1) * ldr + (w % F1)] = make_double2(tmp[q].x, -tmp[q].y);
            }
            __syncthreads();
            const double2* X = line_fft_fast(A, B, F1, ldr, nl, tw1s);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (ok[s] && lrow[s] >= p0 && lrow[s] < p0 + nl) {
                    const double2 z = X[(lrow[s] - p0) * ldr + lcol[s]];
                    const double2 gq = cmul(wsv[s], make_double2(z.x, -z.y));
                    if (a.variant == 0) Au[s] = make_double2(gq.x + a.sigmasq * u[s].x, gq.y + a.sigmasq * u[s].y);
                    else Au[s] = make_double2(gq.x / a.sigmasq + u[s].x, gq.y / a.sigmasq + u[s].y);
                }
            }
            __syncthreads();                                      // the next pass / phase overwrites the buffers
        }
        COOP_STAMP(4);
        return true;
    };
    auto dead = [&]() {
        if (wg == 0 && tid == 0) a.iters[sys] = -3;
        // The asynchronous entries have no host that reads the iteration counts before the result is used (EFGPND keeps them as
        // lazy device values): the unsolved system must show in the DATA, as the Hermitian kernel's refusal does.  The synchronous
        // entry keeps x0 in place and re-solves the system through the multi-launch iteration.
        if (a.nan_on_dead) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (ok[s]) a.x[base + tid + s * kLineThreads] = make_double2(__builtin_nan(""), __builtin_nan(""));
        }
    };

    const bool precond = a.diag != nullptr || a.diag_scale != nullptr;
    double2 Ap[KS];
    double uAu = 0.0;
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Ap[s] = make_double2(0.0, 0.0);
    } else if (!apply(xv, Ap, uAu)) {
        return dead();
    }
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (ok[s]) {
            double2 bv = a.b[base + tid + s * kLineThreads];
            if (a.b_times_ws) bv = cmul(wsv[s], bv);
            rv[s] = make_double2(bv.x - Ap[s].x, bv.y - Ap[s].y);
            pv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            acc[0] += rv[s].x * pv[s].x + rv[s].y * pv[s].y;
            acc[1] += bv.x * bv.x + bv.y * bv.y;
        }
    }
    if (!all_sum(acc, 2, 0)) return dead();
    double rz = acc[0];
    const double bn = sqrt(acc[1]);
    const double den = bn > 0.0 ? bn : 1.0;
    int it = 0;
    for (; it < a.max_iter;) {
        if (!apply(pv, Ap, uAu)) return dead();
        COOP_STAMP(5);
        const double alpha = rz / (uAu + kDivEps);
        acc[0] = acc[1] = 0.0;
        double2 zv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xv[s].x += alpha * pv[s].x;
            xv[s].y += alpha * pv[s].y;
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            acc[0] += rv[s].x * rv[s].x + rv[s].y * rv[s].y;
            acc[1] += rv[s].x * zv[s].x + rv[s].y * zv[s].y;
        }
        COOP_STAMP(6);
        if (!all_sum(acc, 2, 0)) return dead();
        COOP_STAMP(7);
        ++it;
        const double rnorm = sqrt(acc[0]), rzn = acc[1];
        if (a.hist && sys == 0 && wg == 0 && tid == 0 && it <= a.hist_cap) a.hist[it - 1] = rnorm / (den + kDivEps);
        const bool conv = a.early_stop && ((rnorm / (den + kDivEps) < a.tol) || (a.batched && rnorm < 1e-12));
        if (!a.batched && conv) break;                            // cg.py:132
        const double beta = rzn / (rz + kDivEps);
#pragma unroll
        for (int s = 0; s < KS; ++s) pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
        rz = rzn;
        if (conv) break;                                          // cg.py:229-241
    }
#pragma unroll
    for (int s = 0; s < KS; ++s)
        if (ok[s]) a.x[base + tid + s * kLineThreads] = xv[s];
    if (wg == 0 && tid == 0) a.iters[sys] = it;
#undef COOP_STAMP
}

// ==========================================================================================================
// Hermitian specialisation of the cooperative solve (round 3; the mid-size counterpart of cg_herm64_kernel).
// Every CG system of an EFGP model has vectors that are coefficient arrays of REAL functions (u[-k] = conj u[k] on the
// centred modes k in [-h, h]^2), a real even ws and a real centred spectrum S = vhat_c.  With the modes placed CENTRED
// on the torus (mode k at position k mod F) the operator is
//     coefficients -> real function r(f) -> S r -> coefficients,
// and only half of every phase is needed:
//   R : rows k0 = 0..h0 of ws .* u, forward transform along dim 1              -> B1[k0][f1]      (h0 + 1 of n0 rows)
//   C : the column of a real function is the transform of a Hermitian sequence z[k0] = G[k0][c], z[-k0] = conj G[k0][c]:
//       REAL, so two columns c = q, q + F1/2 ride through one complex transform as real and imaginary part (F1/2 column
//       lines); .* the two real spectra (halved), conjugate, transform again; unpack T_q[k0] = T[k0] + conj T[-k0],
//       T_q'[k0] = (T[k0] - conj T[-k0]) / i for k0 >= 0                       -> B2[k0][f1]
//   Ri: rows k0 >= 0, inverse transform along dim 1, crop to |k1| <= h1, A u = ws .* (.) + sigma^2 u
// Row k0 = 0 stores BOTH +k1 and -k1; its line G[0][.] is real only up to the anti-Hermitian rounding noise of the iterates,
// so phase C keeps its real part only (the projection the 64 x 64 kernel needed, see cg_herm.hip).  Dot products weigh
// the rows k0 > 0 twice.  Same recurrences, stopping rule, barrier / all-reduce machinery as cg_coop2d_kernel; a right-hand
// side that is not conjugate-even (or a ws that is not real and even) is refused: -2 iterations, NaN in x.
// Launch geometry in CoopArgs: rows_wg = rows k0 per workgroup (of h0 + 1), cols_wg = column PAIRS per workgroup (of F1 / 2),
// lpbc = pairs per LDS pass.
// ==========================================================================================================
template <int KS, bool SOLO>
__global__ __launch_bounds__(kLineThreads) void cg_coop2d_herm_kernel(CoopArgs a) {
    long long st_prev = (long long)__builtin_readcyclecounter();   // EFGP_COOP_DBG=2: shader clock ticks per phase (workgroup 0, system 0)
#define COOP_STAMP(slot_)                                                                     \
    do {                                                                                      \
        if (a.dbg == 2 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {           \
            const long long now_ = (long long)__builtin_readcyclecounter();                   \
            a.stamps[slot_] += (double)(now_ - st_prev);                                      \
            st_prev = now_;                                                                   \
        }                                                                                     \
    } while (0)
    extern __shared__ double2 lsm[];
    __shared__ double red[kLineThreads / 64];
    __shared__ double fin[3 * kCoopMaxG];
    __shared__ int sflag;
    const int tid = threadIdx.x, wg = blockIdx.x, sys = blockIdx.y, G = a.G;
    const int n0 = (int)a.g.n[0], n1 = (int)a.g.n[1], F0 = (int)a.g.F[0], F1 = (int)a.g.F[1];
    const int h0 = (n0 - 1) / 2, h1 = (n1 - 1) / 2, nh = h0 + 1, halfF1 = F1 >> 1;
    const int ldr = F1 + 1, ldc = F0 + 1;
    const int lgC = ilog2(a.lpbc);
    const unsigned magicF1 = 0xFFFFFFFFu / (unsigned)F1 + 1u;
    const int bufsz = max(a.lines * ldr, a.lpbc * ldc);
    double2* A = lsm;
    double2* B = lsm + bufsz;
    double2* tw1s = B + bufsz;
    double2* tw0s = F0 == F1 ? tw1s : tw1s + F1;
    load_twiddles(tw1s, a.tw1, F1);
    if (F0 != F1) load_twiddles(tw0s, a.tw0, F0);
    // the real spectra of this workgroup's column pairs, [t0][pair] as (S_a, S_b): read inside every column phase
    double2* specL = tw0s + F0;
    if (a.spec_lds) {
        const int c_first = wg * a.cols_wg;
        for (int w = tid; w < F0 * a.lpbc; w += kLineThreads) {
            const int k = w / a.lpbc, l = w - k * a.lpbc;
            specL[w] = make_double2(a.vhat[(int64_t)k * F1 + c_first + l].x, a.vhat[(int64_t)k * F1 + c_first + l + (F1 >> 1)].x);
        }
    }
    __syncthreads();
    const int64_t M = a.g.M;
    const int r0 = wg * a.rows_wg;                            // first owned row k0
    const int nrows = max(0, min(a.rows_wg, nh - r0));
    const int cnt = nrows * n1;
    const int64_t base = (int64_t)sys * M;
    const int p_lo = wg * a.cols_wg;                          // first owned column pair
    double2* b1 = a.b1 + (int64_t)sys * n0 * F1;              // row transforms of the vector just handed to phase R
    double2* b2 = a.b2 + (int64_t)sys * n0 * F1;              // column phase output
    double2* b3 = a.b3 + (int64_t)sys * n0 * F1;              // row transforms of ws .* p, carried from iteration to iteration
    double* part = a.partial + (int64_t)sys * 3 * kCoopMaxG;
    unsigned* bar = a.bar + (int64_t)sys * 16;
    unsigned epoch = 0;

    double2 xv[KS], rv[KS], pv[KS];
    double wsr[KS], dg[KS], wgt[KS];
    int lrow[KS], pos1[KS], tix[KS];                          // owned element s: row k0 = r0 + lrow, torus position of k1, flat index
    bool ok[KS];
    double ws_bad = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int e = tid + s * kLineThreads;
        ok[s] = e < cnt;
        lrow[s] = ok[s] ? e / n1 : 0;
        const int lcol = ok[s] ? e - lrow[s] * n1 : 0;
        const int k0 = r0 + lrow[s];
        pos1[s] = (lcol - h1 + F1) % F1;
        tix[s] = (h0 + k0) * n1 + lcol;
        wgt[s] = k0 == 0 ? 1.0 : 2.0;
        if (ok[s]) {
            xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x[base + tix[s]];
            const double2 w = a.ws[tix[s]], wm = a.ws[M - 1 - tix[s]];
            wsr[s] = w.x;
            ws_bad += w.y * w.y + (w.x - wm.x) * (w.x - wm.x) + wm.y * wm.y;
            dg[s] = coop_jacobi(a, w, tix[s]);
        } else {
            xv[s] = make_double2(0.0, 0.0);
            wsr[s] = 0.0;
            dg[s] = 1.0;
            wgt[s] = 0.0;
        }
        rv[s] = pv[s] = make_double2(0.0, 0.0);
    }
    auto sync_grid = [&]() __attribute__((always_inline)) -> bool {
        if (SOLO) {
            __syncthreads();
            return true;
        }
        return coop_barrier(bar, epoch, a.bar_need, a.status, &sflag);
    };
    auto all_sum = [&](double (&v)[3], int K, int slot0) __attribute__((always_inline)) -> bool {
        double a0 = v[0], a1 = K > 1 ? v[1] : 0.0;
        for (int off = 32; off > 0; off >>= 1) {
            a0 += __shfl_down(a0, off, 64);
            a1 += __shfl_down(a1, off, 64);
        }
        const int lane = tid & 63, wid = tid >> 6;
        __syncthreads();
        if (lane == 0) {
            red[wid] = a0;
            fin[wid] = a1;
        }
        __syncthreads();
        a0 = ((red[0] + red[1]) + red[2]) + red[3];
        a1 = ((fin[0] + fin[1]) + fin[2]) + fin[3];
        if (SOLO) {
            v[0] = a0;
            v[1] = a1;
            __syncthreads();
            return true;
        }
        if (tid == 0) {
            __hip_atomic_store(&part[slot0 * kCoopMaxG + wg], a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (K > 1) __hip_atomic_store(&part[(slot0 + 1) * kCoopMaxG + wg], a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!coop_barrier(bar, epoch, a.bar_need, a.status, &sflag)) return false;
        double b0 = lane < G ? __hip_atomic_load(&part[slot0 * kCoopMaxG + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        double b1v = (K > 1 && lane < G) ? __hip_atomic_load(&part[(slot0 + 1) * kCoopMaxG + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        for (int off = 32; off > 0; off >>= 1) {
            b0 += __shfl_xor(b0, off, 64);
            b1v += __shfl_xor(b1v, off, 64);
        }
        v[0] = b0;
        v[1] = b1v;
        return true;
    };
    // R: row transforms of ws .* u for the owned rows k0 (mode k1 at position k1 mod F1) -> b1
    auto phase_rows = [&](const double2 (&u)[KS]) __attribute__((always_inline)) {
        for (int p0 = 0; p0 < nrows; p0 += a.lines) {
            const int nl = min(a.lines, nrows - p0);
            for (int l = 0; l < nl; ++l)                                      // zeros between the two ends of the mode range
                for (int i1 = h1 + 1 + tid; i1 < F1 - h1; i1 += kLineThreads) A[l * ldr + i1] = make_double2(0.0, 0.0);
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (ok[s] && lrow[s] >= p0 && lrow[s] < p0 + nl) A[(lrow[s] - p0) * ldr + pos1[s]] = make_double2(wsr[s] * u[s].x, wsr[s] * u[s].y);
            __syncthreads();
            const double2* X = line_fft_fast(A, B, F1, ldr, nl, tw1s);
            for (int w = tid; w < nl * F1; w += kLineThreads) {
                const int l = coop_div(w, magicF1), i1 = w - l * F1;
                store_x2<SOLO>(b1 + (int64_t)(r0 + p0 + l) * F1 + i1, X[l * ldr + i1]);
            }
            __syncthreads();
        }
    };
    // C: owned column pairs (q, q + F1/2) in passes of a.lpbc lines.  mode 0: the columns of b1 as they are (operator on a given
    // vector); 1: the same and b3 <- b1 (first direction); 2: b3 <- b1 + beta b3 first -- the row transform of ws .* p follows the
    // direction's own recurrence p = z + beta p, so phase R could run on z BEFORE beta was known (see the iteration below).
    auto phase_cols = [&](int mode, double beta, double& cs) __attribute__((always_inline)) {
        for (int c0 = p_lo; c0 < p_lo + a.cols_wg; c0 += a.lpbc) {
            double2 ta[kCoopLoads / 2], tb[kCoopLoads / 2], tc[kCoopLoads / 2], td[kCoopLoads / 2];
#pragma unroll
            for (int q = 0; q < kCoopLoads / 2; ++q) {                        // every load is issued before the first is used
                const int w = tid + q * kLineThreads, l = w & (a.lpbc - 1), k0 = w >> lgC;
                const bool in = k0 < nh;
                const int64_t o = (int64_t)k0 * F1 + c0 + l;
                ta[q] = in ? load_x2<SOLO>(b1 + o) : make_double2(0.0, 0.0);
                tb[q] = in ? load_x2<SOLO>(b1 + o + halfF1) : make_double2(0.0, 0.0);
                tc[q] = (in && mode == 2) ? load_x2<SOLO>(b3 + o) : make_double2(0.0, 0.0);
                td[q] = (in && mode == 2) ? load_x2<SOLO>(b3 + o + halfF1) : make_double2(0.0, 0.0);
            }
            for (int w = tid; w < a.lpbc * (F0 - 2 * h0 - 1); w += kLineThreads) {          // zeros between the two ends
                const int l = w & (a.lpbc - 1), i0 = h0 + 1 + (w >> lgC);
                A[l * ldc + i0] = make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int q = 0; q < kCoopLoads / 2; ++q) {
                const int w = tid + q * kLineThreads, l = w & (a.lpbc - 1), k0 = w >> lgC;
                if (k0 < nh) {
                    double2 ga = ta[q], gb = tb[q];
                    if (mode == 2) {
                        ga = make_double2(ga.x + beta * tc[q].x, ga.y + beta * tc[q].y);
                        gb = make_double2(gb.x + beta * td[q].x, gb.y + beta * td[q].y);
                    }
                    if (mode != 0) {
                        const int64_t o = (int64_t)k0 * F1 + c0 + l;
                        store_x2<SOLO>(b3 + o, ga);
                        store_x2<SOLO>(b3 + o + halfF1, gb);
                    }
                    if (k0 == 0) {
                        A[l * ldc] = make_double2(ga.x, gb.x);                                    // real part of line k0 = 0
                    } else {
                        A[l * ldc + k0] = make_double2(ga.x - gb.y, ga.y + gb.x);                 // G_a + i G_b
                        A[l * ldc + F0 - k0] = make_double2(ga.x + gb.y, gb.x - ga.y);            // conj G_a + i conj G_b
                    }
                }
            }
            __syncthreads();
            COOP_STAMP(4);
            double2* X = a.spec_lds ? line_fft_fast_mul4(A, B, F0, ldc, a.lpbc, tw0s, specL, a.lpbc, cs)
                                    : line_fft_fast_mul2(A, B, F0, ldc, a.lpbc, tw0s, a.vhat + c0, F1, halfF1, cs);
            double2* Y = X == A ? B : A;
            const double2* Z = line_fft_fast(X, Y, F0, ldc, a.lpbc, tw0s);    // Z = conj T (T = packed, halved result)
            COOP_STAMP(5);
            for (int w = tid; w < (nh << lgC); w += kLineThreads) {
                const int l = w & (a.lpbc - 1), k0 = w >> lgC;
                const double2 zp = Z[l * ldc + k0], zm = Z[l * ldc + (k0 == 0 ? 0 : F0 - k0)];
                const double px = zp.x, py = -zp.y, mx = zm.x, my = -zm.y;       // T[k0], T[-k0]
                store_x2<SOLO>(b2 + (int64_t)k0 * F1 + c0 + l, make_double2(px + mx, py - my));            // T + conj T(-)
                store_x2<SOLO>(b2 + (int64_t)k0 * F1 + c0 + l + halfF1, make_double2(py + my, mx - px));   // (T - conj T(-)) / i
            }
            __syncthreads();
            COOP_STAMP(6);
        }
    };
    // Ri: inverse row transforms of b2 for the owned rows, crop, A u = ws .* (.) + sigma^2 u (or / sigma^2 + u)
    auto phase_rows_inv = [&](const double2 (&u)[KS], double2 (&Au)[KS]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Au[s] = make_double2(0.0, 0.0);
        for (int p0 = 0; p0 < nrows; p0 += a.lines) {
            const int nl = min(a.lines, nrows - p0);
            double2 tmp[kCoopLoads];
#pragma unroll
            for (int q = 0; q < kCoopLoads; ++q) {
                const int w = tid + q * kLineThreads;
                tmp[q] = w < nl * F1 ? load_x2<SOLO>(b2 + (int64_t)(r0 + p0) * F1 + w) : make_double2(0.0, 0.0);   // rows are contiguous
            }
#pragma unroll
            for (int q = 0; q < kCoopLoads; ++q) {
                const int w = tid + q * kLineThreads;
                if (w < nl * F1) A[(w / F1) * ldr + (w % F1)] = make_double2(tmp[q].x, -tmp[q].y);
            }
            __syncthreads();
            COOP_STAMP(8);
            const double2* X = line_fft_fast(A, B, F1, ldr, nl, tw1s);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (ok[s] && lrow[s] >= p0 && lrow[s] < p0 + nl) {
                    const double2 z = X[(lrow[s] - p0) * ldr + pos1[s]];
                    const double2 gq = make_double2(wsr[s] * z.x, -wsr[s] * z.y);
                    if (a.variant == 0) Au[s] = make_double2(gq.x + a.sigmasq * u[s].x, gq.y + a.sigmasq * u[s].y);
                    else Au[s] = make_double2(gq.x / a.sigmasq + u[s].x, gq.y / a.sigmasq + u[s].y);
                }
            }
            __syncthreads();
        }
    };
    auto fill_nan = [&]() {
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (ok[s]) {
                a.x[base + tix[s]] = make_double2(__builtin_nan(""), __builtin_nan(""));
                a.x[base + M - 1 - tix[s]] = make_double2(__builtin_nan(""), __builtin_nan(""));
            }
    };
    auto dead = [&]() {
        if (wg == 0 && tid == 0) a.iters[sys] = -3;
        if (a.nan_on_dead) fill_nan();
    };

    // the contract: b conjugate-even, ws real and even (rounding leaves ~1e-32 |b|^2)
    double2 bv[KS];
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        bv[s] = make_double2(0.0, 0.0);
        if (ok[s]) {
            bv[s] = a.b[base + tix[s]];
            double2 bm = a.b[base + M - 1 - tix[s]];
            if (a.b_times_ws) {                     // ws is real and even here (anything else trips ws_bad above)
                bv[s] = make_double2(wsr[s] * bv[s].x, wsr[s] * bv[s].y);
                bm = make_double2(wsr[s] * bm.x, wsr[s] * bm.y);
            }
            acc[0] += (bv[s].x - bm.x) * (bv[s].x - bm.x) + (bv[s].y + bm.y) * (bv[s].y + bm.y);
            acc[1] += wgt[s] * (bv[s].x * bv[s].x + bv[s].y * bv[s].y);
        }
    }
    acc[0] += ws_bad > 0.0 ? 1e300 : 0.0;
    if (!all_sum(acc, 2, 0)) return dead();
    const double bb = acc[1];
    if (!(acc[0] <= 1e-16 * bb)) {
        fill_nan();
        if (wg == 0 && tid == 0) a.iters[sys] = -2;
        return;
    }
    // r_0 = b - A x_0: one plain operator application (R | barrier | C | barrier | Ri)
    const bool precond = a.diag != nullptr || a.diag_scale != nullptr;
    double2 Ap[KS];
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Ap[s] = make_double2(0.0, 0.0);
    } else {
        double cs = 0.0;
        phase_rows(xv);
        if (!sync_grid()) return dead();
        phase_cols(0, 0.0, cs);
        if (!sync_grid()) return dead();
        phase_rows_inv(xv, Ap);
    }
    double2 zv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        rv[s] = ok[s] ? make_double2(bv[s].x - Ap[s].x, bv[s].y - Ap[s].y) : make_double2(0.0, 0.0);
        zv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
    }
    const double bn = sqrt(bb);
    const double den = bn > 0.0 ? bn : 1.0;
    // Iteration with TWO grid barriers (the complex kernel needs three): the all-reduce of <r,r>, <r,z> rides on the barrier
    // between the row and the column phase of the NEXT operator application.  That application needs p = z + beta p, and beta
    // needs <r,z> -- but the row transform is linear: phase R transforms ws .* z while beta is unknown, and the column phase
    // forms  rows(ws p) = rows(ws z) + beta rows(ws p_prev)  from the copy b3 it keeps of the previous direction's row
    // transforms.  Same recurrences as cg.py:116-150, the direction's transform updated by the direction's own recurrence.
    //   top of trip i: r_i, z_i local; p_{i-1}, <r,z>_{i-1} known; b3 = rows(ws p_{i-1})
    double rz = 0.0;
    int it = 0;
    st_prev = (long long)__builtin_readcyclecounter();
    for (;;) {
        acc[0] = acc[1] = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            acc[0] += wgt[s] * (rv[s].x * rv[s].x + rv[s].y * rv[s].y);
            acc[1] += wgt[s] * (rv[s].x * zv[s].x + rv[s].y * zv[s].y);
        }
        COOP_STAMP(0);
        phase_rows(zv);
        COOP_STAMP(1);
        if (!all_sum(acc, 2, 0)) return dead();                               // barrier 1: <r,r>, <r,z> of r_i
        COOP_STAMP(2);
        const double rnorm = sqrt(acc[0]), rzn = acc[1];
        bool conv = false;
        if (it > 0) {
            if (a.hist && sys == 0 && wg == 0 && tid == 0 && it <= a.hist_cap) a.hist[it - 1] = rnorm / (den + kDivEps);
            conv = a.early_stop && ((rnorm / (den + kDivEps) < a.tol) || (a.batched && rnorm < 1e-12));
            if (conv) break;                                                  // cg.py:132 / :229-241 (p is not an output)
        }
        if (it >= a.max_iter) break;
        const double beta = it > 0 ? rzn / (rz + kDivEps) : 0.0;
        double pp = 0.0, cs = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
            pp += wgt[s] * (pv[s].x * pv[s].x + pv[s].y * pv[s].y);
        }
        rz = rzn;
        COOP_STAMP(3);
        phase_cols(it > 0 ? 2 : 1, beta, cs);
        double t3[3] = {a.variant == 0 ? a.sigmasq * pp + cs : pp + cs / a.sigmasq, 0.0, 0.0};
        if (!all_sum(t3, 1, 2)) return dead();                                // barrier 2: <p, A p>
        COOP_STAMP(7);
        phase_rows_inv(pv, Ap);
        COOP_STAMP(9);
        const double alpha = rz / (t3[0] + kDivEps);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xv[s].x += alpha * pv[s].x;
            xv[s].y += alpha * pv[s].y;
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
        }
        ++it;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s)
        if (ok[s]) {
            a.x[base + tix[s]] = xv[s];
            if (r0 + lrow[s] > 0) a.x[base + M - 1 - tix[s]] = make_double2(xv[s].x, -xv[s].y);        // mode -k
        }
    if (wg == 0 && tid == 0) a.iters[sys] = it;
#undef COOP_STAMP
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
// diagnostic runs of the cooperative solve (EFGP_COOP_DBG=2): the phase shares of workgroup 0, system 0
int coop_print_stamps(const CoopInfo& ci, int iters0) {
    const CoopShape& sh = ci.shape;
    double hs[14];
    EFGP_HIP_CHECK(hipMemcpy(hs, ci.stamps, sizeof(hs), hipMemcpyDeviceToHost));
    const char* nm[14] = {"R store to b1", "barrier 1", "C store", "barrier 2", "Ri load+fft", "pAp sum (incl. barrier)", "update", "rr/rz sum (incl. barrier)",
                          "C load", "C transform 1 (+ multiply)", "-", "C transform 2", "R zero fill, ws u", "R transform"};
    double tot = 0;
    for (int q = 0; q < 14; ++q) tot += hs[q];
    std::fprintf(stderr, "[coop] G = %d, rows/wg %d, lines/pass %d, columns/wg %d, systems/launch %d\n", sh.G, sh.rows_wg, sh.lines, sh.cols_wg, sh.per);
    for (int q = 0; q < 14; ++q) std::fprintf(stderr, "[coop] %-28s %9.0f cycles/iter %5.1f%%\n", nm[q], hs[q] / std::max(1, iters0), 100.0 * hs[q] / tot);
    return EFGP_OK;
}
// ... of the Hermitian kernel: waits for the solve and prints at once
static int coop_print_herm_stamps(const CoopShape& sh, const double* stamps, const int* d_iters, hipStream_t stream) {
    double hs[12];
    int it0 = 0;
    EFGP_HIP_CHECK(stream_wait(stream));
    EFGP_HIP_CHECK(hipMemcpy(hs, stamps, sizeof(hs), hipMemcpyDeviceToHost));
    EFGP_HIP_CHECK(hipMemcpy(&it0, d_iters, sizeof(int), hipMemcpyDeviceToHost));
    const char* nm[10] = {"partial <r,r>, <r,z>", "R: rows of ws z -> b1", "barrier 1 + all-reduce", "beta, p update", "C: loads b1/b3, assemble",
                          "C: transform, spectrum, transform", "C: unpack, stores to b2", "barrier 2 + all-reduce", "Ri: loads of b2", "Ri: transform, A p, x r z"};
    double tot = 0;
    for (int q = 0; q < 10; ++q) tot += hs[q];
    std::fprintf(stderr, "[coop-herm] G = %d, rows/wg %d, lines/pass %d, column pairs/wg %d, systems/launch %d, %d iterations\n", sh.G, sh.rows_wg, sh.lines, sh.cols_wg, sh.per, it0);
    for (int q = 0; q < 10; ++q) std::fprintf(stderr, "[coop-herm] %-36s %9.0f ticks/iter %5.1f%%\n", nm[q], hs[q] / std::max(1, it0), 100.0 * hs[q] / tot);
    return EFGP_OK;
}

// The kernel of a launch shape, by (Hermitian, 8 vector entries per thread, G == 1).  One combination has no kernel: the general
// solve with G = 1 and at most 1024 vector entries.  A cooperative grid has F >= 128 on the reference's grid, so n >= 33 per axis,
// and a workgroup that owns a whole system then holds n0 n1 >= 1089 > 1024 entries: ks is 8 (tools/cg_plan_check.cpp --sweep walks
// every block and batch size and asserts it).  coop_enqueue answers EFGP_EUNSUPPORTED for it like for a shape that does not fit.
using CoopKernel = void (*)(CoopArgs);
static CoopKernel coop_kernel(const CoopShape& sh) {
    static const CoopKernel table[2][2][2] = {
        {{cg_coop2d_kernel<4, false>, nullptr}, {cg_coop2d_kernel<8, false>, cg_coop2d_kernel<8, true>}},
        {{cg_coop2d_herm_kernel<4, false>, cg_coop2d_herm_kernel<4, true>}, {cg_coop2d_herm_kernel<8, false>, cg_coop2d_herm_kernel<8, true>}}};
    return table[sh.herm ? 1 : 0][sh.ks == 8 ? 1 : 0][sh.G == 1 ? 1 : 0];
}

// One cooperative launch of nsys systems.  The hand-rolled grid barrier needs every workgroup of a launch resident: at most one
// workgroup per CU is asked for (G * nsys <= num_cu: coop_shape), so it is enough that ONE fits a CU with these registers and this
// much LDS -- asked once per (device, kernel, LDS size), the query is a host round trip into the runtime.
static int launch_coop(CoopKernel kern, int device, const CoopShape& sh, int nsys, const CoopArgs& ca, hipStream_t stream) {
    if (const int rc = raise_dynamic_lds((const void*)kern, sh.lds, "cooperative CG")) return rc;
    static std::mutex mu;
    static std::map<std::tuple<int, const void*, size_t>, bool> fits;
    const auto key = std::make_tuple(device, (const void*)kern, sh.lds);
    bool known;
    {
        std::lock_guard<std::mutex> lk(mu);
        known = fits.count(key) != 0;
    }
    if (!known) {
        int fit = 0;
        EFGP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kern, kLineThreads, sh.lds));
        if (fit < 1) {
            set_error("cooperative CG: no workgroup with %zu bytes of LDS fits a CU", sh.lds);
            return EFGP_EHIP;
        }
        std::lock_guard<std::mutex> lk(mu);
        fits[key] = true;
    }
    hipLaunchKernelGGL(kern, dim3(sh.G, nsys), dim3(kLineThreads), sh.lds, stream, ca);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

// scratch of one launch of sh.per systems: three intermediate grids | partial sums | arrival counters (64 B apart) | status | stamps
struct CoopScratch {
    double2* pad = nullptr;
    char* scb = nullptr;
    size_t grid_elems = 0, off_bar = 0, off_status = 0;
};
static bool coop_scratch(DeviceCtx* ctx, const ToepGeom& g, const CoopShape& sh, CoopScratch* sc) {
    sc->grid_elems = (size_t)sh.per * (size_t)g.n[0] * (size_t)g.F[1];
    sc->pad = (double2*)scratch(ctx, SLOT_TOEP_PAD, 3 * sc->grid_elems * sizeof(double2));
    sc->off_bar = (size_t)sh.per * 3 * kCoopMaxG * sizeof(double);
    sc->off_status = sc->off_bar + (size_t)sh.per * 64;
    sc->scb = (char*)scratch(ctx, SLOT_MISC, sc->off_status + 64 + 128);
    return sc->pad && sc->scb;
}

// the kernel's arguments but for the slab of systems (b, x, iters, hist: set per launch)
static CoopArgs coop_args(const efgp_toeplitz_s* op, const CgSolve& s, const ToepGeom& g, bool small, const CoopShape& sh, const CoopScratch& sc,
                          int nan_on_dead, bool test_dead) {
    CoopArgs ca;
    ca.g = g;
    ca.ws = s.ws;
    ca.diag = s.diag;
    ca.diag_scale = s.diag ? nullptr : s.diag_scale;
    ca.b_times_ws = s.b_times_ws;
    ca.zero_x0 = s.zero_x0;
    ca.sigmasq = s.sigmasq;
    ca.variant = s.variant;
    ca.tol = s.tol;
    ca.early_stop = s.early_stop;
    ca.batched = s.batched;
    ca.max_iter = s.max_iter;
    ca.vhat = small ? op->vhat_co : op->vhat_c;
    ca.tw0 = small ? op->tw_co[0] : op->tw[0];
    ca.tw1 = small ? op->tw_co[1] : op->tw[1];
    ca.b1 = sc.pad;
    ca.b2 = sc.pad + sc.grid_elems;
    ca.b3 = sc.pad + 2 * sc.grid_elems;
    ca.spec_lds = sh.spec_lds ? 1 : 0;
    ca.partial = (double*)sc.scb;
    ca.bar = (unsigned*)(sc.scb + sc.off_bar);
    ca.status = (int*)(sc.scb + sc.off_status);
    ca.hist_cap = cg_history().capacity;
    ca.nan_on_dead = nan_on_dead;
    ca.G = sh.G;
    ca.bar_need = test_dead ? sh.G + 1 : sh.G;
    ca.rows_wg = sh.rows_wg;
    ca.cols_wg = sh.cols_wg;
    ca.lines = sh.lines;
    ca.lpbc = sh.lpbc;
    ca.dbg = std::getenv("EFGP_COOP_DBG") ? std::atoi(std::getenv("EFGP_COOP_DBG")) : 0;
    ca.stamps = (double*)(sc.scb + sc.off_status + 64);
    return ca;
}

// Enqueues the cooperative solve of `nbatch` systems on a 2-D 128^2..512^2 grid in the launch shape coop_shape gives.  Iteration
// counts go to d_iters (device, nbatch ints; -3 where a grid barrier died), *d_status (device int) is non-zero when one did.
// EFGP_EUNSUPPORTED when no launch shape fits.
int coop_enqueue(efgp_toeplitz_s* op, const CgSolve& s, int* d_iters, hipStream_t stream, CoopInfo* info, int nan_on_dead) {
    const int nbatch = s.nbatch;
    const bool small = op->coop_small && std::getenv("EFGP_NO_COOP_SMALL") == nullptr;
    const ToepGeom g = small ? op->g_co : op->g;
    const CoopShape sh = coop_shape(g, nbatch, s.hermitian != 0, op->ctx->num_cu, op->ctx->max_lds);
    const CoopKernel kern = coop_kernel(sh);
    if (!sh.ok || !kern) return EFGP_EUNSUPPORTED;
    CoopScratch sc;
    if (!coop_scratch(op->ctx, g, sh, &sc)) return EFGP_ENOMEM;
    if (!small && !ensure_centred_spectrum(op, stream)) return EFGP_EUNSUPPORTED;
    // test hook (tests/test_gpu_variance_ops.py): every grid barrier of this launch dies at once -- one arrival more than there
    // are workgroups is awaited and the status word is preset, so the first status check (256 polls) ends the wait
    const bool test_dead = sh.G > 1 && std::getenv("EFGP_COOP_TEST_DEAD") != nullptr;
    CoopArgs ca = coop_args(op, s, g, small, sh, sc, nan_on_dead, test_dead);
    if (ca.dbg == 2) EFGP_HIP_CHECK(hipMemsetAsync(ca.stamps, 0, 128, stream));
    {
        KernelTimer timer("cg_coop", stream);
        for (int s0 = 0; s0 < nbatch; s0 += sh.per) {
            const int nsys = std::min(sh.per, nbatch - s0);
            ca.b = s.b + (int64_t)s0 * g.M;
            ca.x = s.x + (int64_t)s0 * g.M;
            ca.iters = d_iters + s0;
            ca.hist = s0 == 0 ? cg_history().buf : nullptr;
            // the status word is cleared before EVERY launch: a dead barrier in one slab of systems must not make the later
            // slabs give up at their first poll (the per-system iteration counts carry the -3 of the slab that died).  It sits
            // right behind the arrival counters: one fill for both
            if (!test_dead) {
                EFGP_HIP_CHECK(hipMemsetAsync(sc.scb + sc.off_bar, 0, (size_t)sh.per * 64 + 64, stream));
            } else {
                EFGP_HIP_CHECK(hipMemsetAsync(sc.scb + sc.off_bar, 0, (size_t)sh.per * 64, stream));
                EFGP_HIP_CHECK(hipMemsetAsync(sc.scb + sc.off_status, 1, 64, stream));
            }
            if (const int rc = launch_coop(kern, op->device, sh, nsys, ca, stream)) return rc;
        }
    }
    if (info) *info = CoopInfo{ca.status, sh, ca.stamps, ca.dbg};
    if (sh.herm && ca.dbg == 2) return coop_print_herm_stamps(sh, ca.stamps, d_iters, stream);
    return EFGP_OK;
}

}  // namespace efgp
