// The multi-launch CG solver of the EFGP normal equations (every grid the single-launch solves do not take, and the re-solve of a
// cooperative launch whose grid barrier died): the vector kernels of the generic iteration, the pruned in-LDS line-transform kernels
// of the 2-D and 3-D grids, and the host loop that enqueues bursts of iterations and polls the row scalars (solve_multi_launch).
// The operator object, its spectra and the dispatch of a solve: toeplitz_cg.hip.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <vector>

#include "cg_plan_host.hpp"
#include "common.hpp"
#include "line_fft.hpp"
#include "toeplitz_cg.hpp"
#include "toeplitz_line_dev.hpp"
#include "toeplitz_op.hpp"

namespace efgp {

// EFGP_CG_TRACE=1: report host-side spans of the multi-kernel solve that take longer than 2 ms (stderr)
struct TraceSpan {
    const char* what;
    std::chrono::steady_clock::time_point t0;
    bool on;
    explicit TraceSpan(const char* w) : what(w), on(std::getenv("EFGP_CG_TRACE") != nullptr) {
        if (on) t0 = std::chrono::steady_clock::now();
    }
    ~TraceSpan() {
        if (!on) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > 2.0) std::fprintf(stderr, "[efgp cg trace] %s: %.1f ms\n", what, ms);
    }
};

// ------------------------------------------------------------------------------------------
// CG state
// ------------------------------------------------------------------------------------------
struct CgRowScalars {   // one per row
    double rz;
    double den;        // |b| or 1
    double pAp;        // <p, A p> + div_eps of the current iteration (written by the last block of cg_dot_kernel)
    double beta;       // p <- z + beta p is applied by the NEXT iteration's cg_pad_kernel when do_p is set
    int active;
    int iters;         // iterations in which this row was updated
    int do_p;
    int pad_;
};

constexpr int kCgBlocksMax = 256;    // workgroups per system in the multi-kernel update (partials per reduction; <= block size)

struct CgArgs {
    ToepGeom g;
    const double2* ws;
    const double* diag;       // may be null
    double sigmasq;
    int variant;              // 0 A_mean, 1 A_var
    double tol;
    int early_stop;
    int batched;              // convergence-test placement (cg.py single vs batched)
    const double2* b;
    double2* x;
    double2* r;
    double2* p;
    double2* ap;              // A p of the current iteration (written by cg_dot_kernel, read by cg_axpy_kernel)
    const double2* pad;       // inverse-FFT output, row slot = blockIdx.y
    double2* pad_out;         // the same buffer, written by cg_pad_kernel
    const int* rows;          // slot -> row (null: identity)
    CgRowScalars* sc;
    int* status;              // [0] = number of active rows (recomputed by host), [1] = any-change flag
    double* partial;          // [rows][3][kCgBlocksMax] per-workgroup partial sums
    int* counter;             // [rows][2] arrival counters of the two reductions
    int nblk;                 // workgroups per system
    double* hist;             // diagnostic: row 0's |r_i| / |b| per iteration (efgp_cg_record_history) or null
    int hist_cap;
    // the part of every vector the update kernels walk: [v_off, v_off + v_len) of the M entries; entries below v_off + v_w1
    // count once in the dot products, the others twice.  General systems: (0, M, M).  Hermitian 3-D systems (round 3): the
    // planes k0 >= 0 -- (h0 n1 n2, (h0 + 1) n1 n2, n1 n2): plane k0 = 0 once, every other plane for itself and its mirror image.
    int64_t v_off, v_len, v_w1;
};

// A u for block element t given the cropped Toeplitz product Tu = T(ws*u)[t]
__device__ __forceinline__ double2 apply_A(const CgArgs& a, double2 wst, double2 Tu, double2 u) {
    double2 g = cmul(wst, Tu);
    if (a.variant == 0) return make_double2(g.x + a.sigmasq * u.x, g.y + a.sigmasq * u.y);
    return make_double2(g.x / a.sigmasq + u.x, g.y / a.sigmasq + u.y);
}

// ---- one CG iteration (cg.py:116-150 / :193-241), spread over nblk workgroups per system ----------------
// A system with M up to ~2e5 unknowns is far too long for one workgroup (measured: 60 us per iteration at
// M = 12167), so the iteration is three launches over (nblk, slots) grids; dot products are reduced in two
// deterministic levels: fixed-order sums inside a workgroup, then the LAST workgroup to arrive (device-scope
// arrival counter) adds the nblk partials in index order and publishes the scalars.  The direction update
// p <- z + beta p is deferred into the next iteration's pad kernel, which needs ws .* p anyway.
__device__ __forceinline__ double load_agent(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // bypasses this CU's L1
}
__device__ __forceinline__ void store_agent(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // write-through, leaves no dirty L2 line behind
}
// Arrival at a reduction: returns true in every thread of the LAST of `nblk` workgroups to arrive at `counter`.
// Thread 0 has stored this workgroup's partial sums with store_agent; it drains them (s_waitcnt vmcnt(0)) before its arrival,
// and the last arriver reads all partials with load_agent (L1-bypassing): the hand-off form R1 of MI355X_MICROARCH.md, no
// fence.  Round 3: the __threadfence() pair that stood here cost EVERY workgroup an L2 write-back, serialised per XCD --
// 15-18 of cg3_inv2_kernel's 23 us at 207 workgroups, ~9 of cg_axpy_kernel's 14 us at 64.  Everything else these kernels write
// is read by later launches only (kernel boundary).
__device__ __forceinline__ bool arrive_count(int* counter, int nblk, int* flag) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int prev = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = prev == nblk - 1;
        if (*flag) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // all arrivals of this launch are in
    }
    __syncthreads();
    return *flag != 0;
}
__device__ __forceinline__ bool arrive_last(const CgArgs& a, int row, int which, int* flag) {
    return arrive_count(&a.counter[2 * row + which], a.nblk, flag);
}
__device__ __forceinline__ void block_range(const CgArgs& a, int64_t& lo, int64_t& hi) {
    const int64_t per = (a.v_len + a.nblk - 1) / a.nblk, end = a.v_off + a.v_len;
    lo = a.v_off + (int64_t)blockIdx.x * per;
    hi = lo + per < end ? lo + per : end;
}

// r = b - A x0, z = r/diag, p = z, rz = <r,z>, den = |b| (cg.py:94-111 / :164-186).  grid = (nblk, rows): round 3 -- with ONE
// workgroup per system (as before) a 3-D system of 185 k unknowns (BASELINE configs[4] at eps 1e-3) spent 630 us here, 11 % of
// a hyper-gradient step; the two sums are reduced like the iteration's (fixed order inside a workgroup, partials added in index
// order by the last workgroup to arrive).
__global__ __launch_bounds__(kVecThreads) void cg_init_kernel(CgArgs a) {
    __shared__ double red[kVecThreads / 64];
    __shared__ int flag;
    const int row = blockIdx.y;
    const double2* P = a.pad + (int64_t)row * a.g.Ftot;
    const int64_t base = (int64_t)row * a.g.M;
    int64_t lo, hi;
    block_range(a, lo, hi);
    double rz = 0.0, bb = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kVecThreads) {
        const int64_t o = base + t;
        double2 x0 = a.x[o];
        double2 Ax = apply_A(a, a.ws[t], P[pad_index(a.g, t, 1)], x0);
        double2 bv = a.b[o];
        double2 rv = make_double2(bv.x - Ax.x, bv.y - Ax.y);
        double2 zv = rv;
        if (a.diag) {
            zv.x = rv.x / a.diag[t];
            zv.y = rv.y / a.diag[t];
        }
        a.r[o] = rv;
        a.p[o] = zv;
        rz += rv.x * zv.x + rv.y * zv.y;
        bb += bv.x * bv.x + bv.y * bv.y;
    }
    rz = block_sum(rz, red);
    bb = block_sum(bb, red);
    double* part = a.partial + (int64_t)row * 3 * kCgBlocksMax;
    if (threadIdx.x == 0) {
        store_agent(&part[kCgBlocksMax + blockIdx.x], rz);
        store_agent(&part[2 * kCgBlocksMax + blockIdx.x], bb);
    }
    if (!arrive_last(a, row, 1, &flag)) return;
    __shared__ double fin[2 * kCgBlocksMax];
    if (threadIdx.x < a.nblk) {
        fin[threadIdx.x] = load_agent(&part[kCgBlocksMax + threadIdx.x]);
        fin[kCgBlocksMax + threadIdx.x] = load_agent(&part[2 * kCgBlocksMax + threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double srz = 0.0, sbb = 0.0;
        for (int i = 0; i < a.nblk; ++i) {
            srz += fin[i];
            sbb += fin[kCgBlocksMax + i];
        }
        const double bn = sqrt(sbb);
        a.sc[row].rz = srz;
        a.sc[row].den = bn > 0.0 ? bn : 1.0;
        a.sc[row].active = 1;
        a.sc[row].iters = 0;
        a.sc[row].pAp = 1.0;
        a.sc[row].beta = 0.0;
        a.sc[row].do_p = 0;
        a.sc[row].pad_ = 0;
    }
}

// pad[slot] = zero-padded ws .* p, after the deferred direction update p <- r/diag + beta p
__global__ __launch_bounds__(kVecThreads) void cg_pad_kernel(CgArgs a) {
    const int slot = blockIdx.y;
    const int row = a.rows ? a.rows[slot] : slot;
    if (row < 0) return;
    const CgRowScalars sc = a.sc[row];
    if (!sc.active) return;
    const ToepGeom& g = a.g;
    double2* P = a.pad_out + (int64_t)slot * g.Ftot;
    const int64_t base = (int64_t)row * g.M;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.Ftot; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t rem = t, flat = 0;
        bool inside = true;
        int64_t coords[3];
        for (int q = g.d - 1; q >= 0; --q) {
            coords[q] = rem % g.F[q];
            rem /= g.F[q];
            inside = inside && coords[q] < g.n[q];
        }
        double2 v = make_double2(0.0, 0.0);
        if (inside) {
            for (int q = 0; q < g.d; ++q) flat = flat * g.n[q] + coords[q];
            double2 pv = a.p[base + flat];
            if (sc.do_p) {
                double2 zv = a.r[base + flat];
                if (a.diag) {
                    zv.x /= a.diag[flat];
                    zv.y /= a.diag[flat];
                }
                pv = make_double2(zv.x + sc.beta * pv.x, zv.y + sc.beta * pv.y);
                a.p[base + flat] = pv;
            }
            v = cmul(pv, a.ws[flat]);
        }
        P[t] = v;
    }
}

// A p and <p, A p>
__global__ __launch_bounds__(kVecThreads) void cg_dot_kernel(CgArgs a) {
    __shared__ double red[kVecThreads / 64];
    __shared__ int flag;
    const int slot = blockIdx.y;
    const int row = a.rows ? a.rows[slot] : slot;
    if (row < 0) return;
    if (!a.sc[row].active) return;
    const double2* P = a.pad + (int64_t)slot * a.g.Ftot;
    const int64_t base = (int64_t)row * a.g.M;
    int64_t lo, hi;
    block_range(a, lo, hi);
    double pAp = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kVecThreads) {
        const double2 pv = a.p[base + t];
        const double2 Ap = apply_A(a, a.ws[t], P[pad_index32(a.g, (int)t, 1)], pv);
        a.ap[base + t] = Ap;
        pAp += pv.x * Ap.x + pv.y * Ap.y;
    }
    pAp = block_sum(pAp, red);
    double* part = a.partial + (int64_t)row * 3 * kCgBlocksMax;
    if (threadIdx.x == 0) store_agent(&part[blockIdx.x], pAp);
    if (arrive_last(a, row, 0, &flag)) {
        __shared__ double fin[kCgBlocksMax];
        if (threadIdx.x < a.nblk) fin[threadIdx.x] = load_agent(&part[threadIdx.x]);     // loads in parallel
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int i = 0; i < a.nblk; ++i) t += fin[i];                                    // summed in index order
            a.sc[row].pAp = t + kDivEps;
        }
    }
}

// x += alpha p, r -= alpha A p, |r|^2, <r, r/diag>; the last workgroup decides convergence and beta
__global__ __launch_bounds__(kVecThreads) void cg_axpy_kernel(CgArgs a) {
    __shared__ double red[kVecThreads / 64];
    __shared__ int flag;
    const int slot = blockIdx.y;
    const int row = a.rows ? a.rows[slot] : slot;
    if (row < 0) return;
    const CgRowScalars sc = a.sc[row];
    if (!sc.active) return;
    const int64_t base = (int64_t)row * a.g.M;
    int64_t lo, hi;
    block_range(a, lo, hi);
    const double alpha = sc.rz / sc.pAp;
    double rr = 0.0, rz_new = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += kVecThreads) {
        const double2 pv = a.p[base + t];
        const double2 Ap = a.ap[base + t];
        double2 xv = a.x[base + t];
        double2 rv = a.r[base + t];
        xv.x += alpha * pv.x;
        xv.y += alpha * pv.y;
        rv.x -= alpha * Ap.x;
        rv.y -= alpha * Ap.y;
        a.x[base + t] = xv;
        a.r[base + t] = rv;
        const double q = (t - a.v_off < a.v_w1 ? 1.0 : 2.0) * (rv.x * rv.x + rv.y * rv.y);
        rr += q;
        rz_new += a.diag ? q / a.diag[t] : q;
    }
    rr = block_sum(rr, red);
    rz_new = block_sum(rz_new, red);
    double* part = a.partial + (int64_t)row * 3 * kCgBlocksMax;
    if (threadIdx.x == 0) {
        store_agent(&part[kCgBlocksMax + blockIdx.x], rr);
        store_agent(&part[2 * kCgBlocksMax + blockIdx.x], rz_new);
    }
    if (!arrive_last(a, row, 1, &flag)) return;
    __shared__ double fin[2 * kCgBlocksMax];
    if (threadIdx.x < a.nblk) {
        fin[threadIdx.x] = load_agent(&part[kCgBlocksMax + threadIdx.x]);
        fin[kCgBlocksMax + threadIdx.x] = load_agent(&part[2 * kCgBlocksMax + threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double srr = 0.0, srz = 0.0;
        for (int i = 0; i < a.nblk; ++i) {
            srr += fin[i];
            srz += fin[kCgBlocksMax + i];
        }
        const double rnorm = sqrt(srr);
        if (a.hist && row == 0 && sc.iters < a.hist_cap) a.hist[sc.iters] = rnorm / (sc.den + kDivEps);
        const bool conv = a.early_stop && ((rnorm / (sc.den + kDivEps) < a.tol) || (a.batched && rnorm < 1e-12));
        CgRowScalars out = sc;
        out.iters = sc.iters + 1;
        if (conv) {                          // single: stop before the p update (cg.py:132); batched: after it
            out.active = 0;                  // (cg.py:229-241) -- p is never used again either way
            out.do_p = 0;
            atomicAdd(&a.status[1], 1);
        } else {
            out.beta = srz / (sc.rz + kDivEps);
            out.do_p = 1;
        }
        if (!(conv && !a.batched)) out.rz = srz;
        a.sc[row] = out;
    }
}

// ==========================================================================================================
// Fused line-FFT iteration for 2-D grids beyond one CU's LDS (F = 128..512 per dimension).
//   The generic iteration above spends 11 launches (pad, 2x2 rocFFT passes, multiply, update kernels) and moves
//   the whole padded F x F grid through HBM five times although only n of its F rows are non-zero on the way in
//   and only n rows / columns are kept on the way out.  Here a matvec is three launches of batched in-LDS line
//   transforms with the pruning built in:
//     cg_rows_fwd_kernel : (deferred p update) ws .* p, zero-padded, forward FFT along dim 1 of the n rows -> B1[n][F]
//     cg_cols_mid_kernel : per group of columns: forward FFT along dim 0 (n non-zero inputs), .* vhat, inverse FFT,
//                          rows of the crop window -> B2[n][F]
//     cg_rows_inv_kernel : inverse FFT along dim 1 of the n window rows, crop, A p, <p, A p> (two-level reduction)
//   followed by cg_axpy_kernel.  Lines are transformed with a Stockham autosort FFT (radix 4, one radix-2 stage
//   for odd log2 F) in two LDS ping-pong buffers; twiddles come from the per-length table exp(-2 pi i q / F).
// ==========================================================================================================
// kLineThreads, kCoopMaxG, kCoopLoads: cg_plan_host.hpp (the host's planners use them too)

struct LineArgs {
    CgArgs c;
    const double2* vhat;      // [F0][F1], already divided by F0*F1
    const double2* tw0;       // exp(-2 pi i q / F0)
    const double2* tw1;
    double2* b1;              // [slots][n0][F1]
    double2* b2;              // [slots][n0][F1]
    int nblk_rows;            // row blocks per system = ceil(n0 / lpb): partial sums of <p, A p>
    int lpb;                  // lines per workgroup (a power of two; larger for batched solves: fewer reduction arrivals)
};

__global__ __launch_bounds__(kLineThreads) void cg_rows_fwd_kernel(LineArgs a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    const CgRowScalars sc = c.sc[row];
    if (!sc.active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], F1 = (int)c.g.F[1], ld = F1 + 1;
    const int r0 = blockIdx.x * a.lpb;
    const int nl = min(a.lpb, n0 - r0);
    double2* A = lsm;
    double2* B = lsm + a.lpb * ld;
    double2* tws = B + a.lpb * ld;
    load_twiddles(tws, a.tw1, F1);
    const int64_t base = (int64_t)row * c.g.M;
    for (int w = threadIdx.x; w < nl * F1; w += kLineThreads) {
        const int l = w / F1, i1 = w - l * F1;
        double2 v = make_double2(0.0, 0.0);
        if (i1 < n1) {
            const int t = (r0 + l) * n1 + i1;
            double2 pv = c.p[base + t];
            if (sc.do_p) {                                       // deferred p <- r/diag + beta p
                double2 zv = c.r[base + t];
                if (c.diag) {
                    zv.x /= c.diag[t];
                    zv.y /= c.diag[t];
                }
                pv = make_double2(zv.x + sc.beta * pv.x, zv.y + sc.beta * pv.y);
                c.p[base + t] = pv;
            }
            v = cmul(pv, c.ws[t]);
        }
        A[l * ld + i1] = v;
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F1, ld, nl, tws);
    double2* out = a.b1 + ((int64_t)slot * n0 + r0) * F1;
    for (int w = threadIdx.x; w < nl * F1; w += kLineThreads) {
        const int l = w / F1, i1 = w - l * F1;
        out[(int64_t)l * F1 + i1] = X[l * ld + i1];
    }
}

__global__ __launch_bounds__(kLineThreads) void cg_cols_mid_kernel(LineArgs a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], F0 = (int)c.g.F[0], F1 = (int)c.g.F[1], ld = F0 + 1;
    const int c0 = blockIdx.x * a.lpb;                  // first column of this block (F1 % 8 == 0)
    double2* A = lsm;
    double2* B = lsm + a.lpb * ld;
    double2* tws = B + a.lpb * ld;
    load_twiddles(tws, a.tw0, F0);
    const double2* in = a.b1 + (int64_t)slot * n0 * F1;
    // line l = column c0 + l; consecutive threads read consecutive columns of one row (128-B segments)
    for (int w = threadIdx.x; w < a.lpb * F0; w += kLineThreads) {
        const int i0 = w / a.lpb, l = w - i0 * a.lpb;
        A[l * ld + i0] = i0 < n0 ? in[(int64_t)i0 * F1 + c0 + l] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    double2* X = line_fft_any(A, B, F0, ld, a.lpb, tws);
    double2* Y = X == A ? B : A;
    // .* vhat, conjugate: the inverse transform is conj(FFT(conj(.)))
    for (int w = threadIdx.x; w < a.lpb * F0; w += kLineThreads) {
        const int i0 = w / a.lpb, l = w - i0 * a.lpb;
        const double2 m = cmul(X[l * ld + i0], a.vhat[(int64_t)i0 * F1 + c0 + l]);
        X[l * ld + i0] = make_double2(m.x, -m.y);
    }
    __syncthreads();
    const double2* Z = line_fft_any(X, Y, F0, ld, a.lpb, tws);
    double2* out = a.b2 + (int64_t)slot * n0 * F1;
    for (int w = threadIdx.x; w < a.lpb * n0; w += kLineThreads) {
        const int j = w / a.lpb, l = w - j * a.lpb;
        const double2 z = Z[l * ld + (n0 - 1) + j];               // crop window rows [n0-1, 2 n0-1)
        out[(int64_t)j * F1 + c0 + l] = make_double2(z.x, -z.y);
    }
}

__global__ __launch_bounds__(kLineThreads) void cg_rows_inv_kernel(LineArgs a) {
    extern __shared__ double2 lsm[];
    __shared__ double red[kLineThreads / 64];
    __shared__ int flag;
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], F1 = (int)c.g.F[1], ld = F1 + 1;
    const int r0 = blockIdx.x * a.lpb;
    const int nl = min(a.lpb, n0 - r0);
    double2* A = lsm;
    double2* B = lsm + a.lpb * ld;
    double2* tws = B + a.lpb * ld;
    load_twiddles(tws, a.tw1, F1);
    const double2* in = a.b2 + ((int64_t)slot * n0 + r0) * F1;
    for (int w = threadIdx.x; w < nl * F1; w += kLineThreads) {
        const int l = w / F1, i1 = w - l * F1;
        const double2 v = in[(int64_t)l * F1 + i1];
        A[l * ld + i1] = make_double2(v.x, -v.y);
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F1, ld, nl, tws);
    const int64_t base = (int64_t)row * c.g.M;
    double pAp = 0.0;
    for (int w = threadIdx.x; w < nl * n1; w += kLineThreads) {
        const int l = w / n1, i1 = w - l * n1;
        const int t = (r0 + l) * n1 + i1;
        const double2 z = X[l * ld + (n1 - 1) + i1];
        const double2 pv = c.p[base + t];
        const double2 Ap = apply_A(c, c.ws[t], make_double2(z.x, -z.y), pv);
        c.ap[base + t] = Ap;
        pAp += pv.x * Ap.x + pv.y * Ap.y;
    }
    pAp = block_sum(pAp, red);
    double* part = c.partial + (int64_t)row * 3 * kCgBlocksMax;
    if (threadIdx.x == 0) store_agent(&part[blockIdx.x], pAp);
    if (!arrive_count(&c.counter[2 * row], a.nblk_rows, &flag)) return;      // arrival counter 0 with this kernel's own block count
    __shared__ double fin[kCgBlocksMax];
    if (threadIdx.x < a.nblk_rows) fin[threadIdx.x] = load_agent(&part[threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < a.nblk_rows; ++i) t += fin[i];
        c.sc[row].pAp = t + kDivEps;
    }
}

// ==========================================================================================================
// The same for 3-D grids (F = 64..256 per dimension): five launches of pruned batched line transforms.
//   fwd2 : (deferred p update) ws .* p, FFT along dim 2 of the n0*n1 non-zero lines            -> B1[n0][n1][F2]
//   fwd1 : per (i0, group of t2): FFT along dim 1 of n1 non-zero inputs                        -> B2[n0][F1][F2]
//   mid0 : per (t1, group of t2): FFT along dim 0 of n0 non-zero inputs, .* vhat, inverse FFT,
//          crop-window rows, in place                                                           -> B2[n0][F1][F2]
//   inv1 : per (j0, group of t2): inverse FFT along dim 1, crop-window rows                    -> B1[n0][n1][F2]
//   inv2 : inverse FFT along dim 2 of the n0*n1 window lines, crop, A p, <p, A p>
//   The generic iteration moves the full F^3 grid (4 MB at 64^3) through ~12 passes per matvec; these kernels touch
//   n0 F1 F2 elements at most (1.5 MB) four times.  `lpb` lines per workgroup (a power of two chosen by the host).
// ==========================================================================================================
struct Line3Args {
    CgArgs c;
    const double2* vhat;      // [F0][F1][F2], already divided by F0*F1*F2
    const double2* tw[3];     // exp(-2 pi i q / F[a])
    double2* b1;              // [slots][n0][n1][F2]
    double2* b2;              // [slots][n0][F1][F2]
    int lpb_c;                // lines per workgroup, contiguous kernels (fwd2, inv2)
    int lpb_s;                // adjacent t2 columns per workgroup, strided kernels (fwd1, mid0, inv1)
    int nblk_lines;           // workgroups of inv2 per system: partial sums of <p, A p>
};

__global__ __launch_bounds__(kLineThreads) void cg3_fwd2_kernel(Line3Args a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    const CgRowScalars sc = c.sc[row];
    if (!sc.active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], n2 = (int)c.g.n[2], F2 = (int)c.g.F[2], ld = F2 + 1;
    const int nlines = n0 * n1;
    const int l0 = blockIdx.x * a.lpb_c;
    const int nl = min(a.lpb_c, nlines - l0);
    double2* A = lsm;
    double2* B = lsm + a.lpb_c * ld;
    double2* tws = B + a.lpb_c * ld;
    load_twiddles(tws, a.tw[2], F2);
    const int64_t base = (int64_t)row * c.g.M;
    for (int w = threadIdx.x; w < nl * F2; w += kLineThreads) {
        const int l = w / F2, i2 = w - l * F2;
        double2 v = make_double2(0.0, 0.0);
        if (i2 < n2) {
            const int t = (l0 + l) * n2 + i2;                     // flat block index: line = i0*n1 + i1
            double2 pv = c.p[base + t];
            if (sc.do_p) {                                       // deferred p <- r/diag + beta p
                double2 zv = c.r[base + t];
                if (c.diag) {
                    zv.x /= c.diag[t];
                    zv.y /= c.diag[t];
                }
                pv = make_double2(zv.x + sc.beta * pv.x, zv.y + sc.beta * pv.y);
                c.p[base + t] = pv;
            }
            v = cmul(pv, c.ws[t]);
        }
        A[l * ld + i2] = v;
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F2, ld, nl, tws);
    double2* out = a.b1 + ((int64_t)slot * nlines + l0) * F2;
    for (int w = threadIdx.x; w < nl * F2; w += kLineThreads) {
        const int l = w / F2, i2 = w - l * F2;
        out[(int64_t)l * F2 + i2] = X[l * ld + i2];
    }
}

// MODE 0: forward along dim 1 (B1 -> B2);  MODE 1: inverse along dim 1 with crop (B2 -> B1)
template <int MODE>
__global__ __launch_bounds__(kLineThreads) void cg3_dim1_kernel(Line3Args a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], F1 = (int)c.g.F[1], F2 = (int)c.g.F[2], ld = F1 + 1;
    const int L = a.lpb_s;
    const int groups = F2 / L;
    const int i0 = blockIdx.x / groups, c0 = (blockIdx.x - i0 * groups) * L;      // plane i0 (or j0), first t2 column
    double2* A = lsm;
    double2* B = lsm + L * ld;
    double2* tws = B + L * ld;
    load_twiddles(tws, a.tw[1], F1);
    const double2* b1 = a.b1 + (int64_t)slot * n0 * n1 * F2;
    double2* b2 = a.b2 + (int64_t)slot * n0 * F1 * F2;
    if (MODE == 0) {
        for (int w = threadIdx.x; w < L * F1; w += kLineThreads) {
            const int i1 = w / L, l = w - i1 * L;
            A[l * ld + i1] = i1 < n1 ? b1[((int64_t)i0 * n1 + i1) * F2 + c0 + l] : make_double2(0.0, 0.0);
        }
    } else {
        for (int w = threadIdx.x; w < L * F1; w += kLineThreads) {
            const int t1 = w / L, l = w - t1 * L;
            const double2 v = b2[((int64_t)i0 * F1 + t1) * F2 + c0 + l];
            A[l * ld + t1] = make_double2(v.x, -v.y);
        }
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F1, ld, L, tws);
    if (MODE == 0) {
        for (int w = threadIdx.x; w < L * F1; w += kLineThreads) {
            const int t1 = w / L, l = w - t1 * L;
            b2[((int64_t)i0 * F1 + t1) * F2 + c0 + l] = X[l * ld + t1];
        }
    } else {
        double2* out = a.b1 + (int64_t)slot * n0 * n1 * F2;
        for (int w = threadIdx.x; w < L * n1; w += kLineThreads) {
            const int j1 = w / L, l = w - j1 * L;
            const double2 z = X[l * ld + (n1 - 1) + j1];
            out[((int64_t)i0 * n1 + j1) * F2 + c0 + l] = make_double2(z.x, -z.y);
        }
    }
}

__global__ __launch_bounds__(kLineThreads) void cg3_mid0_kernel(Line3Args a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], F0 = (int)c.g.F[0], F1 = (int)c.g.F[1], F2 = (int)c.g.F[2], ld = F0 + 1;
    const int L = a.lpb_s;
    const int groups = F2 / L;
    const int t1 = blockIdx.x / groups, c0 = (blockIdx.x - t1 * groups) * L;
    double2* A = lsm;
    double2* B = lsm + L * ld;
    double2* tws = B + L * ld;
    load_twiddles(tws, a.tw[0], F0);
    double2* b2 = a.b2 + (int64_t)slot * n0 * F1 * F2;
    for (int w = threadIdx.x; w < L * F0; w += kLineThreads) {
        const int i0 = w / L, l = w - i0 * L;
        A[l * ld + i0] = i0 < n0 ? b2[((int64_t)i0 * F1 + t1) * F2 + c0 + l] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    double2* X = line_fft_any(A, B, F0, ld, L, tws);
    double2* Y = X == A ? B : A;
    for (int w = threadIdx.x; w < L * F0; w += kLineThreads) {
        const int t0 = w / L, l = w - t0 * L;
        const double2 m = cmul(X[l * ld + t0], a.vhat[((int64_t)t0 * F1 + t1) * F2 + c0 + l]);
        X[l * ld + t0] = make_double2(m.x, -m.y);
    }
    __syncthreads();
    const double2* Z = line_fft_any(X, Y, F0, ld, L, tws);
    for (int w = threadIdx.x; w < L * n0; w += kLineThreads) {
        const int j0 = w / L, l = w - j0 * L;
        const double2 z = Z[l * ld + (n0 - 1) + j0];
        b2[((int64_t)j0 * F1 + t1) * F2 + c0 + l] = make_double2(z.x, -z.y);
    }
}

__global__ __launch_bounds__(kLineThreads) void cg3_inv2_kernel(Line3Args a) {
    extern __shared__ double2 lsm[];
    __shared__ double red[kLineThreads / 64];
    __shared__ int flag;
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], n2 = (int)c.g.n[2], F2 = (int)c.g.F[2], ld = F2 + 1;
    const int nlines = n0 * n1;
    const int l0 = blockIdx.x * a.lpb_c;
    const int nl = min(a.lpb_c, nlines - l0);
    double2* A = lsm;
    double2* B = lsm + a.lpb_c * ld;
    double2* tws = B + a.lpb_c * ld;
    load_twiddles(tws, a.tw[2], F2);
    const double2* in = a.b1 + ((int64_t)slot * nlines + l0) * F2;
    for (int w = threadIdx.x; w < nl * F2; w += kLineThreads) {
        const int l = w / F2, i2 = w - l * F2;
        const double2 v = in[(int64_t)l * F2 + i2];
        A[l * ld + i2] = make_double2(v.x, -v.y);
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F2, ld, nl, tws);
    const int64_t base = (int64_t)row * c.g.M;
    double pAp = 0.0;
    for (int w = threadIdx.x; w < nl * n2; w += kLineThreads) {
        const int l = w / n2, i2 = w - l * n2;
        const int t = (l0 + l) * n2 + i2;
        const double2 z = X[l * ld + (n2 - 1) + i2];
        const double2 pv = c.p[base + t];
        const double2 Ap = apply_A(c, c.ws[t], make_double2(z.x, -z.y), pv);
        c.ap[base + t] = Ap;
        pAp += pv.x * Ap.x + pv.y * Ap.y;
    }
    pAp = block_sum(pAp, red);
    double* part = c.partial + (int64_t)row * 3 * kCgBlocksMax;
    if (threadIdx.x == 0) store_agent(&part[blockIdx.x], pAp);
    if (!arrive_count(&c.counter[2 * row], a.nblk_lines, &flag)) return;
    __shared__ double fin[kCgBlocksMax];
    if (threadIdx.x < a.nblk_lines) fin[threadIdx.x] = load_agent(&part[threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < a.nblk_lines; ++i) t += fin[i];
        c.sc[row].pAp = t + kDivEps;
    }
}

// ==========================================================================================================
// Round 3: the 3-D line iteration for HERMITIAN systems (vectors = Fourier coefficients of real functions on the symmetric mode
// box, ws real and even, Toeplitz vector Hermitian -- every system EFGP solves: efgpnd.py:119-141, 192-206, 926-941).
//   u[-k] = conj u[k]: only the planes k0 = 0..h0 are carried ((h0 + 1) n1 n2 of the M entries, the upper half of the flat
//   vector).  Modes sit CENTRED on the torus (k at k mod F), which makes the spectrum of the (Hermitian) Toeplitz vector real:
//   vc = Re(vhat e^(2 pi i sum f_a (n_a - 1) / F_a)), stored as doubles.
//     fwd2 / dim1<0> : as above on the (h0 + 1) planes: half the lines
//     mid0           : the k0-sequence of a column (t1, t2) is Hermitian, its transform real: TWO columns (t2, t2 + F2/2) ride
//                      through one complex transform as real and imaginary part (line_fft_inwave<R, 3>), are multiplied by
//                      their real spectra and come back through the second transform; unpacked as T + conj T(-) and
//                      (T - conj T(-)) / i.  Plane k0 = 0 keeps its real part only (projection on the Hermitian subspace:
//                      without it rounding noise in that plane is fed back, cf. cg_herm64_kernel).
//     dim1<1> / inv2 : back on the (h0 + 1) planes; <p, A p> counts plane 0 once and the others twice
//   Per operator application at mtot = 57 (F = 128): 66 MB through HBM/L2 instead of 150 MB (the spectrum alone 33.5 -> 16.8 MB).
// ==========================================================================================================
struct Line3HArgs {
    CgArgs c;
    const double* vc;         // [F0][F1][F2] real centred spectrum, already divided by F0*F1*F2
    const double2* tw[3];
    double2* b1;              // [slots][(h0+1) n1][F2]
    double2* b2;              // [slots][h0+1][F1][F2]
    int lpb_c;                // lines per workgroup, contiguous kernels (fwd2, inv2)
    int lpb_s;                // adjacent t2 columns per workgroup, dim-1 kernels
    int lpb_m;                // column pairs per workgroup, mid0
    int nblk_lines;           // workgroups of inv2 per system
};
// torus position -> index into the centred mode range of n = 2h+1 (or -1)
__device__ __forceinline__ int centred_index(int pos, int h, int F) { return pos <= h ? pos + h : (pos >= F - h ? pos - (F - h) : -1); }

__global__ __launch_bounds__(kLineThreads) void cg3h_fwd2_kernel(Line3HArgs a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    const CgRowScalars sc = c.sc[row];
    if (!sc.active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], n2 = (int)c.g.n[2], F2 = (int)c.g.F[2], ld = F2 + 1;
    const int h2 = (n2 - 1) / 2, lgF2 = ilog2(F2);
    const int nlines = ((n0 + 1) / 2) * n1;
    const int l0 = blockIdx.x * a.lpb_c;
    const int nl = min(a.lpb_c, nlines - l0);
    double2* A = lsm;
    double2* B = lsm + a.lpb_c * ld;
    double2* tws = B + a.lpb_c * ld;
    load_twiddles(tws, a.tw[2], F2);
    const int64_t base = (int64_t)row * c.g.M;
    for (int w = threadIdx.x; w < (nl << lgF2); w += kLineThreads) {
        const int l = w >> lgF2, pos = w & (F2 - 1);
        const int i2 = centred_index(pos, h2, F2);
        double2 v = make_double2(0.0, 0.0);
        if (i2 >= 0) {
            const int64_t t = c.v_off + (int64_t)(l0 + l) * n2 + i2;
            double2 pv = c.p[base + t];
            if (sc.do_p) {                                       // deferred p <- r/diag + beta p
                double2 zv = c.r[base + t];
                if (c.diag) {
                    zv.x /= c.diag[t];
                    zv.y /= c.diag[t];
                }
                pv = make_double2(zv.x + sc.beta * pv.x, zv.y + sc.beta * pv.y);
                c.p[base + t] = pv;
            }
            const double wr = c.ws[t].x;
            v = make_double2(wr * pv.x, wr * pv.y);
        }
        A[l * ld + pos] = v;
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F2, ld, nl, tws);
    double2* out = a.b1 + ((int64_t)slot * nlines + l0) * F2;
    for (int w = threadIdx.x; w < (nl << lgF2); w += kLineThreads) {
        const int l = w >> lgF2, i2 = w & (F2 - 1);
        out[(int64_t)l * F2 + i2] = X[l * ld + i2];
    }
}

// MODE 0: forward along dim 1 (b1 -> b2);  MODE 1: inverse along dim 1 with crop (b2 -> b1); planes k0 = 0..h0
template <int MODE>
__global__ __launch_bounds__(kLineThreads) void cg3h_dim1_kernel(Line3HArgs a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], F1 = (int)c.g.F[1], F2 = (int)c.g.F[2], ld = F1 + 1;
    const int nh = (n0 + 1) / 2, h1 = (n1 - 1) / 2;
    const int L = a.lpb_s, lgL = ilog2(L);
    const int groups = F2 / L;
    const int k0 = blockIdx.x / groups, c0 = (blockIdx.x - k0 * groups) * L;
    double2* A = lsm;
    double2* B = lsm + L * ld;
    double2* tws = B + L * ld;
    load_twiddles(tws, a.tw[1], F1);
    double2* b1 = a.b1 + (int64_t)slot * nh * n1 * F2;
    double2* b2 = a.b2 + (int64_t)slot * nh * F1 * F2;
    if (MODE == 0) {
        for (int w = threadIdx.x; w < (F1 << lgL); w += kLineThreads) {
            const int pos = w >> lgL, l = w & (L - 1);
            const int i1 = centred_index(pos, h1, F1);
            A[l * ld + pos] = i1 >= 0 ? b1[((int64_t)k0 * n1 + i1) * F2 + c0 + l] : make_double2(0.0, 0.0);
        }
    } else {
        for (int w = threadIdx.x; w < (F1 << lgL); w += kLineThreads) {
            const int t1 = w >> lgL, l = w & (L - 1);
            const double2 v = b2[((int64_t)k0 * F1 + t1) * F2 + c0 + l];
            A[l * ld + t1] = make_double2(v.x, -v.y);
        }
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F1, ld, L, tws);
    if (MODE == 0) {
        for (int w = threadIdx.x; w < (F1 << lgL); w += kLineThreads) {
            const int t1 = w >> lgL, l = w & (L - 1);
            b2[((int64_t)k0 * F1 + t1) * F2 + c0 + l] = X[l * ld + t1];
        }
    } else {
        for (int w = threadIdx.x; w < (n1 << lgL); w += kLineThreads) {
            const int i1 = w >> lgL, l = w & (L - 1);
            const double2 z = X[l * ld + ((i1 - h1) & (F1 - 1))];
            b1[((int64_t)k0 * n1 + i1) * F2 + c0 + l] = make_double2(z.x, -z.y);
        }
    }
}

// per (t1, group of L column pairs (c, c + F2/2)): packed transform along dim 0, real spectra, back, in place in b2
__global__ __launch_bounds__(kLineThreads) void cg3h_mid0_kernel(Line3HArgs a) {
    extern __shared__ double2 lsm[];
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], F0 = (int)c.g.F[0], F1 = (int)c.g.F[1], F2 = (int)c.g.F[2], ld = F0 + 1;
    const int nh = (n0 + 1) / 2, h0 = nh - 1, halfF2 = F2 >> 1;
    const int L = a.lpb_m, lgL = ilog2(L);
    const int groups = halfF2 / L;
    const int t1 = blockIdx.x / groups, c0 = (blockIdx.x - t1 * groups) * L;
    double2* A = lsm;
    double2* B = lsm + L * ld;
    double2* tws = B + L * ld;
    // the spectrum values this thread multiplies by behind the first transform: requested before anything else, so that their
    // round trip runs beside the load of the lines and the transform instead of inside it
    const double* spec = a.vc + (int64_t)t1 * F2 + c0;
    const bool pre_ok = (F0 == 64 && L <= 32) || (F0 == 128 && L <= 16) || (F0 == 256 && L <= 8);
    double2 pre[8];
    if (pre_ok) {
        if (F0 == 64) spectrum_prefetch<1>(spec, (int64_t)F1 * F2, halfF2, L, pre);
        else if (F0 == 128) spectrum_prefetch<2>(spec, (int64_t)F1 * F2, halfF2, L, pre);
        else spectrum_prefetch<4>(spec, (int64_t)F1 * F2, halfF2, L, pre);
    }
    load_twiddles(tws, a.tw[0], F0);
    double2* b2 = a.b2 + (int64_t)slot * nh * F1 * F2;
    for (int w = threadIdx.x; w < ((F0 - 2 * h0 - 1) << lgL); w += kLineThreads) {           // zeros between the two ends
        const int l = w & (L - 1), i0 = h0 + 1 + (w >> lgL);
        A[l * ld + i0] = make_double2(0.0, 0.0);
    }
    for (int w = threadIdx.x; w < (nh << lgL); w += kLineThreads) {
        const int k0 = w >> lgL, l = w & (L - 1);
        const int64_t o = ((int64_t)k0 * F1 + t1) * F2 + c0 + l;
        const double2 ga = b2[o], gb = b2[o + halfF2];
        if (k0 == 0) {
            A[l * ld] = make_double2(ga.x, gb.x);                                       // real part of plane k0 = 0
        } else {
            A[l * ld + k0] = make_double2(ga.x - gb.y, ga.y + gb.x);                    // G_a + i G_b
            A[l * ld + F0 - k0] = make_double2(ga.x + gb.y, gb.x - ga.y);               // conj G_a + i conj G_b
        }
    }
    __syncthreads();
    double2* X;
    if (pre_ok) {
        if (F0 == 64) line_fft_inwave<1, 5>(A, B, ld, L, tws, pre);
        else if (F0 == 128) line_fft_inwave<2, 5>(A, B, ld, L, tws, pre);
        else line_fft_inwave<4, 5>(A, B, ld, L, tws, pre);
        X = B;
    } else if (F0 == 64 || F0 == 128 || F0 == 256 || F0 == 512) {
        X = line_fft_fast_mul3(A, B, F0, ld, L, tws, spec, (int64_t)F1 * F2, halfF2);
    } else {
        X = line_fft(A, B, F0, ld, L, tws);
        for (int w = threadIdx.x; w < (F0 << lgL); w += kLineThreads) {
            const int t0 = w >> lgL, l = w & (L - 1);
            const int64_t o = ((int64_t)t0 * F1 + t1) * F2 + c0 + l;
            const double2 v = X[l * ld + t0];
            X[l * ld + t0] = make_double2(0.5 * a.vc[o] * v.x, -0.5 * a.vc[o + halfF2] * v.y);
        }
        __syncthreads();
    }
    double2* Y = X == A ? B : A;
    const double2* Z = line_fft_any(X, Y, F0, ld, L, tws);                              // Z = conj T (T = packed, halved result)
    for (int w = threadIdx.x; w < (nh << lgL); w += kLineThreads) {
        const int k0 = w >> lgL, l = w & (L - 1);
        const double2 zp = Z[l * ld + k0], zm = Z[l * ld + ((F0 - k0) & (F0 - 1))];
        const double px = zp.x, py = -zp.y, mx = zm.x, my = -zm.y;                      // T[k0], T[-k0]
        const int64_t o = ((int64_t)k0 * F1 + t1) * F2 + c0 + l;
        b2[o] = make_double2(px + mx, py - my);                                         // T + conj T(-)
        b2[o + halfF2] = make_double2(py + my, mx - px);                                // (T - conj T(-)) / i
    }
}

__global__ __launch_bounds__(kLineThreads) void cg3h_inv2_kernel(Line3HArgs a) {
    extern __shared__ double2 lsm[];
    __shared__ double red[kLineThreads / 64];
    __shared__ int flag;
    const CgArgs& c = a.c;
    const int slot = blockIdx.y;
    const int row = c.rows ? c.rows[slot] : slot;
    if (row < 0) return;
    if (!c.sc[row].active) return;
    const int n0 = (int)c.g.n[0], n1 = (int)c.g.n[1], n2 = (int)c.g.n[2], F2 = (int)c.g.F[2], ld = F2 + 1;
    const int h2 = (n2 - 1) / 2, lgF2 = ilog2(F2);
    const int nlines = ((n0 + 1) / 2) * n1;
    const int l0 = blockIdx.x * a.lpb_c;
    const int nl = min(a.lpb_c, nlines - l0);
    double2* A = lsm;
    double2* B = lsm + a.lpb_c * ld;
    double2* tws = B + a.lpb_c * ld;
    load_twiddles(tws, a.tw[2], F2);
    const double2* in = a.b1 + ((int64_t)slot * nlines + l0) * F2;
    for (int w = threadIdx.x; w < (nl << lgF2); w += kLineThreads) {
        const int l = w >> lgF2, i2 = w & (F2 - 1);
        const double2 v = in[(int64_t)l * F2 + i2];
        A[l * ld + i2] = make_double2(v.x, -v.y);
    }
    __syncthreads();
    const double2* X = line_fft_any(A, B, F2, ld, nl, tws);
    const int64_t base = (int64_t)row * c.g.M;
    double pAp = 0.0;
    for (int w = threadIdx.x; w < nl * n2; w += kLineThreads) {
        const int l = w / n2, i2 = w - l * n2;
        const int64_t t = c.v_off + (int64_t)(l0 + l) * n2 + i2;
        const double2 z = X[l * ld + ((i2 - h2) & (F2 - 1))];
        const double2 pv = c.p[base + t];
        const double2 Ap = apply_A(c, make_double2(c.ws[t].x, 0.0), make_double2(z.x, -z.y), pv);
        c.ap[base + t] = Ap;
        pAp += (l0 + l < n1 ? 1.0 : 2.0) * (pv.x * Ap.x + pv.y * Ap.y);                 // plane k0 = 0 once, the others twice
    }
    pAp = block_sum(pAp, red);
    double* part = c.partial + (int64_t)row * 3 * kCgBlocksMax;
    if (threadIdx.x == 0) store_agent(&part[blockIdx.x], pAp);
    if (!arrive_count(&c.counter[2 * row], a.nblk_lines, &flag)) return;
    __shared__ double fin[kCgBlocksMax];
    if (threadIdx.x < a.nblk_lines) fin[threadIdx.x] = load_agent(&part[threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < a.nblk_lines; ++i) t += fin[i];
        c.sc[row].pAp = t + kDivEps;
    }
}

// x[-k] = conj x[k] for the planes k0 > 0 (the iteration carried k0 >= 0 only)
__global__ __launch_bounds__(kVecThreads) void cg3h_mirror_kernel(CgArgs a) {
    const int row = blockIdx.y;
    double2* x = a.x + (int64_t)row * a.g.M;
    for (int64_t e = a.v_w1 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.v_len; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = a.v_off + e;
        const double2 v = x[t];
        x[a.g.M - 1 - t] = make_double2(v.x, -v.y);
    }
}

// the contract of the Hermitian iteration, checked on the data: out[0] = sum |b[t] - conj b[M-1-t]|^2 + |x0[t] - conj x0[M-1-t]|^2,
// out[1] = sum |b|^2 + |x0|^2 over all rows, out[2] = sum over t of (Im ws)^2 + (ws[t] - ws[M-1-t])^2
__global__ __launch_bounds__(kVecThreads) void cg_herm_check_kernel(const double2* __restrict__ b, const double2* __restrict__ x0,
                                                                    const double2* __restrict__ ws, int64_t M, int rows, double* out) {
    __shared__ double red[kVecThreads / 64];
    double viol = 0.0, bb = 0.0, wbad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)rows * M; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / M, t = i - r * M;
        const double2 u = b[i], um = b[r * M + M - 1 - t], y = x0[i], ym = x0[r * M + M - 1 - t];
        viol += (u.x - um.x) * (u.x - um.x) + (u.y + um.y) * (u.y + um.y) + (y.x - ym.x) * (y.x - ym.x) + (y.y + ym.y) * (y.y + ym.y);
        bb += u.x * u.x + u.y * u.y + y.x * y.x + y.y * y.y;
        if (r == 0) {
            const double2 w = ws[t], wm = ws[M - 1 - t];
            wbad += w.y * w.y + (w.x - wm.x) * (w.x - wm.x);
        }
    }
    viol = block_sum(viol, red);
    bb = block_sum(bb, red);
    wbad = block_sum(wbad, red);
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], viol);
        atomicAdd(&out[1], bb);
        atomicAdd(&out[2], wbad);
    }
}

// vc[f] = Re(vhat[f] e^(2 pi i sum_a f_a (n_a - 1) / F_a)): the real spectrum of the Hermitian Toeplitz vector with its lags centred
__global__ __launch_bounds__(256) void center_spectrum3_real_kernel(const double2* __restrict__ vhat, const double2* __restrict__ tw0,
                                                                    const double2* __restrict__ tw1, const double2* __restrict__ tw2,
                                                                    int n0, int n1, int n2, int F0, int F1, int F2, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)F0 * F1 * F2) return;
    const int f2 = (int)(t % F2), f1 = (int)((t / F2) % F1), f0 = (int)(t / ((int64_t)F1 * F2));
    const double2 a = tw0[((int64_t)(n0 - 1) * f0) & (F0 - 1)], b = tw1[((int64_t)(n1 - 1) * f1) & (F1 - 1)], cc = tw2[((int64_t)(n2 - 1) * f2) & (F2 - 1)];
    const double2 ab = cmul(a, b), abc = cmul(ab, cc);
    out[t] = cmul(vhat[t], make_double2(abc.x, -abc.y)).x;
}

// ---- the multi-launch solver ----------------------------------------------------------------------------------------------------
constexpr int kPollEvery = 8;        // iterations per burst: enqueued (or replayed) together, then the host reads the scalars

// The pruned line-transform kernels keep 2 x lpb lines of F + 1 elements and the F twiddles in LDS: the lines that fit, and the
// bytes of lpb of them
static int64_t line_lds_fit(const DeviceCtx* ctx, int64_t F) {
    return ((int64_t)ctx->max_lds / (int64_t)sizeof(double2) - F) / (2 * (F + 1));
}
static size_t line_lds_bytes(int lpb, int64_t F) { return ((size_t)2 * lpb * (size_t)(F + 1) + (size_t)F) * sizeof(double2); }
// Lines per workgroup of the reducing line kernels, from `lpb`: doubled while the workgroups (one partial sum each) outnumber
// kCgBlocksMax, then for more than 8 systems up to `many_cap`.  Every workgroup of the reducing kernels pays a device-scope fence
// (an L2 write-back, ~2 us each, serialised per XCD): few systems -> many small workgroups for parallelism, many systems -> few
// large ones (fewer reduction fences).  Both limits must hold, LDS and partial sums (found at full size: mtot = 57, F = 128 asked
// for 64 lines per block = 266 KB of LDS).
static int lines_per_block(int lpb, int64_t nlines, int64_t fit, int rows, int many_cap) {
    while ((nlines + lpb - 1) / lpb > kCgBlocksMax && lpb * 2 <= fit) lpb <<= 1;
    if (rows > 8) {
        while (lpb * 2 <= fit && lpb < many_cap) lpb <<= 1;
    }
    return lpb;
}

// How an iteration of the multi-launch solver applies the operator to p: the chosen kind with its kernel arguments (their copy of
// the CgArgs, `c`, is set at every enqueue) and LDS bytes
struct OperatorApply {
    enum Kind {
        kFft,        // pad + FFT + multiply + FFT (circulant) and the dot kernel
        kLines2,     // 2-D mid-size grids: three launches of pruned in-LDS line transforms instead of pad + rocFFT + multiply
        kLines3,     // 3-D: the same with five pruned line passes
        kLines3H     // Hermitian 3-D systems: the planes k0 >= 0 only (cg3h_* kernels)
    } kind = kFft;
    LineArgs la;
    Line3Args l3;
    Line3HArgs l3h;
    size_t lds[3] = {0, 0, 0};       // of the kernels that transform along dimension q
};

// every line kernel of a kind with the dimension it transforms along (its dynamic LDS is OperatorApply::lds[axis])
struct LineKernel {
    const void* kernel;
    int axis;
};
static int raise_line_lds(const LineKernel* begin, const LineKernel* end, const size_t* lds) {
    for (const LineKernel* k = begin; k != end; ++k)
        if (const int rc = raise_dynamic_lds(k->kernel, lds[k->axis], "CG line kernels")) return rc;
    return EFGP_OK;
}

// The Hermitian 3-D set-up on top of the general one: the real centred spectrum on first use, the check of the data (once per group
// of rows, through the pinned `host`), the half block in `a`
static int setup_apply_herm3(efgp_toeplitz_s* op, CgArgs& a, int rows, int shape_rows, int* host, hipStream_t stream, OperatorApply* ap) {
    DeviceCtx* ctx = op->ctx;
    const ToepGeom& g = op->g;
    if (!op->vc3) {
        op->vc3 = (double*)pool_alloc(ctx, real_spectrum_bytes(g));
        if (!op->vc3) return EFGP_ENOMEM;
        hipLaunchKernelGGL(center_spectrum3_real_kernel, dim3((unsigned)((g.Ftot + 255) / 256)), dim3(256), 0, stream, op->vhat, op->tw[0],
                           op->tw[1], op->tw[2], (int)g.n[0], (int)g.n[1], (int)g.n[2], (int)g.F[0], (int)g.F[1], (int)g.F[2], op->vc3);
        EFGP_HIP_CHECK(hipGetLastError());
    }
    double* chk_buf = (double*)scratch(ctx, SLOT_MISC, 64);
    if (!chk_buf) return EFGP_ENOMEM;
    EFGP_HIP_CHECK(hipMemsetAsync(chk_buf, 0, 64, stream));
    hipLaunchKernelGGL(cg_herm_check_kernel, dim3(256), dim3(kVecThreads), 0, stream, a.b, (const double2*)a.x, a.ws, g.M, rows, chk_buf);
    EFGP_HIP_CHECK(hipGetLastError());
    EFGP_HIP_CHECK(hipMemcpyAsync(host, chk_buf, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
    EFGP_HIP_CHECK(stream_wait(stream));
    double hv[3];
    std::memcpy(hv, host, sizeof(hv));
    if (!(hv[0] <= 1e-16 * hv[1]) || hv[2] > 0.0) {
        set_error("efgp_cg_solve_hermitian: right-hand side / start vector not conjugate-even or ws not real and even");
        return EFGP_EINVAL;
    }
    const int64_t nh = (g.n[0] + 1) / 2;
    a.v_off = (nh - 1) * g.n[1] * g.n[2];
    a.v_len = nh * g.n[1] * g.n[2];
    a.v_w1 = g.n[1] * g.n[2];
    Line3HArgs& l3h = ap->l3h;
    l3h.vc = op->vc3;
    for (int q = 0; q < 3; ++q) l3h.tw[q] = op->tw[q];
    l3h.b1 = a.pad_out;
    l3h.b2 = a.pad_out + (int64_t)rows * nh * g.n[1] * g.F[2];
    const int64_t nlines = nh * g.n[1];
    const int64_t fit = line_lds_fit(ctx, g.F[2]);
    int lpb = lines_per_block(8, nlines, fit, shape_rows, 64);
    if (shape_rows >= 3 && lpb < 16 && 32 <= fit) lpb = 16;          // measured at mtot 57: 125 vs 133 us per iteration of 3 systems
    auto knob = [](const char* name, int dflt) {
        const char* e = std::getenv(name);
        int v = e ? std::atoi(e) : dflt;
        int p2 = 1;
        while (p2 * 2 <= v) p2 <<= 1;
        return std::max(1, p2);
    };
    if (std::getenv("EFGP_CG3_LC")) {
        lpb = knob("EFGP_CG3_LC", lpb);
        while ((nlines + lpb - 1) / lpb > kCgBlocksMax) lpb <<= 1;
    }
    l3h.lpb_c = lpb;
    l3h.lpb_s = (int)std::min<int64_t>(knob("EFGP_CG3_LS", 16), g.F[2] / 2);
    l3h.lpb_m = (int)std::min<int64_t>(knob("EFGP_CG3_LM", shape_rows >= 3 ? 32 : 16), g.F[2] / 2);      // 3 systems: 124.6 vs 132.6 us
    l3h.nblk_lines = (int)((nlines + lpb - 1) / lpb);
    ap->lds[2] = line_lds_bytes(lpb, g.F[2]);
    ap->lds[1] = line_lds_bytes(l3h.lpb_s, g.F[1]);
    ap->lds[0] = line_lds_bytes(l3h.lpb_m, g.F[0]);
    static const LineKernel kLines3H[] = {{(const void*)cg3h_fwd2_kernel, 2}, {(const void*)cg3h_inv2_kernel, 2}, {(const void*)cg3h_dim1_kernel<0>, 1},
                                          {(const void*)cg3h_dim1_kernel<1>, 1}, {(const void*)cg3h_mid0_kernel, 0}};
    if (const int rc = raise_line_lds(std::begin(kLines3H), std::end(kLines3H), ap->lds)) return rc;
    a.nblk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(std::min(kCgBlocksMax, knob("EFGP_CG_NBLK", 128)), (a.v_len + kVecThreads - 1) / kVecThreads),
                                                        std::max<int64_t>(1, 1024 / shape_rows)));
    ap->kind = OperatorApply::kLines3H;
    return EFGP_OK;
}

// Chooses how the iterations of this group of `rows` systems apply the operator and sets it up (the 2-D line kernels need the
// reference grid's spectrum; the Hermitian 3-D ones change the block `a` describes).  The launch shapes -- lines per workgroup, and
// with them the order of the partial sums -- follow `shape_rows`, the size of a full group of the solve (solve_multi_launch)
static int setup_apply(efgp_toeplitz_s* op, const CgSolve& s, CgArgs& a, int rows, int shape_rows, int* host, hipStream_t stream,
                       OperatorApply* ap) {
    DeviceCtx* ctx = op->ctx;
    const ToepGeom& g = op->g;
    if (std::getenv("EFGP_NO_CG_LINES") != nullptr) return EFGP_OK;
    if (op->lines_ok) {
        const int rc = ensure_reference_spectrum(op, stream);
        if (rc != EFGP_OK) return rc;
        LineArgs& la = ap->la;
        la.vhat = op->vhat;
        la.tw0 = op->tw[0];
        la.tw1 = op->tw[1];
        la.b1 = a.pad_out;                                                     // [rows][n0][F1] fits: Ftot >= 2 n0 F1
        la.b2 = a.pad_out + (int64_t)rows * g.n[0] * g.F[1];
        la.lpb = lines_per_block(4, g.n[0], line_lds_fit(ctx, std::max(g.F[0], g.F[1])), shape_rows, 32);
        la.nblk_rows = (int)((g.n[0] + la.lpb - 1) / la.lpb);
        ap->lds[1] = line_lds_bytes(la.lpb, g.F[1]);
        ap->lds[0] = line_lds_bytes(la.lpb, g.F[0]);
        static const LineKernel kLines2[] = {{(const void*)cg_rows_fwd_kernel, 1}, {(const void*)cg_rows_inv_kernel, 1}, {(const void*)cg_cols_mid_kernel, 0}};
        if (const int rc = raise_line_lds(std::begin(kLines2), std::end(kLines2), ap->lds)) return rc;
        ap->kind = OperatorApply::kLines2;
        return EFGP_OK;
    }
    if (!op->lines3_ok) return EFGP_OK;
    const int64_t nlines = g.n[0] * g.n[1];
    const int64_t fit = line_lds_fit(ctx, g.F[2]);
    int64_t lmax = 16;
    while (lmax * 2 <= fit) lmax <<= 1;
    if (fit < 16 || (nlines + lmax - 1) / lmax > kCgBlocksMax) return EFGP_OK;      // no lines-per-block count meets both limits
    Line3Args& l3 = ap->l3;
    l3.vhat = op->vhat;
    for (int q = 0; q < 3; ++q) l3.tw[q] = op->tw[q];
    l3.b1 = a.pad_out;
    l3.b2 = a.pad_out + (int64_t)rows * nlines * g.F[2];
    l3.lpb_c = lines_per_block(16, nlines, fit, shape_rows, 64);
    l3.lpb_s = 16;
    l3.nblk_lines = (int)((nlines + l3.lpb_c - 1) / l3.lpb_c);
    ap->lds[2] = line_lds_bytes(l3.lpb_c, g.F[2]);
    for (int q = 0; q < 2; ++q) ap->lds[q] = line_lds_bytes(l3.lpb_s, g.F[q]);
    static const LineKernel kLines3[] = {{(const void*)cg3_fwd2_kernel, 2}, {(const void*)cg3_inv2_kernel, 2}, {(const void*)cg3_dim1_kernel<0>, 1},
                                         {(const void*)cg3_dim1_kernel<1>, 1}, {(const void*)cg3_mid0_kernel, 0}};
    if (const int rc = raise_line_lds(std::begin(kLines3), std::end(kLines3), ap->lds)) return rc;
    ap->kind = OperatorApply::kLines3;
    if (s.hermitian && (g.n[0] & 1) && (g.n[1] & 1) && (g.n[2] & 1) && g.n[0] >= 3 && std::getenv("EFGP_NO_CG_HERM3") == nullptr)
        return setup_apply_herm3(op, a, rows, shape_rows, host, stream, ap);
    return EFGP_OK;
}

// one CG iteration of `slots` systems: A p by the chosen kind, then the fused update
static int enqueue_iteration(efgp_toeplitz_s* op, OperatorApply& ap, const CgArgs& a, int slots, hipStream_t stream) {
    const ToepGeom& g = op->g;
    switch (ap.kind) {
    case OperatorApply::kLines3H: {
        Line3HArgs& l3h = ap.l3h;
        l3h.c = a;
        const unsigned nhp = (unsigned)((g.n[0] + 1) / 2);
        const unsigned gs = (unsigned)(g.F[2] / l3h.lpb_s), gp = (unsigned)(g.F[2] / 2 / l3h.lpb_m);
        hipLaunchKernelGGL(cg3h_fwd2_kernel, dim3(l3h.nblk_lines, slots), dim3(kLineThreads), ap.lds[2], stream, l3h);
        hipLaunchKernelGGL((cg3h_dim1_kernel<0>), dim3(nhp * gs, slots), dim3(kLineThreads), ap.lds[1], stream, l3h);
        hipLaunchKernelGGL(cg3h_mid0_kernel, dim3((unsigned)g.F[1] * gp, slots), dim3(kLineThreads), ap.lds[0], stream, l3h);
        hipLaunchKernelGGL((cg3h_dim1_kernel<1>), dim3(nhp * gs, slots), dim3(kLineThreads), ap.lds[1], stream, l3h);
        hipLaunchKernelGGL(cg3h_inv2_kernel, dim3(l3h.nblk_lines, slots), dim3(kLineThreads), ap.lds[2], stream, l3h);
        break;
    }
    case OperatorApply::kLines3: {
        Line3Args& l3 = ap.l3;
        l3.c = a;
        const unsigned gs = (unsigned)(g.F[2] / l3.lpb_s);
        hipLaunchKernelGGL(cg3_fwd2_kernel, dim3(l3.nblk_lines, slots), dim3(kLineThreads), ap.lds[2], stream, l3);
        hipLaunchKernelGGL((cg3_dim1_kernel<0>), dim3((unsigned)g.n[0] * gs, slots), dim3(kLineThreads), ap.lds[1], stream, l3);
        hipLaunchKernelGGL(cg3_mid0_kernel, dim3((unsigned)g.F[1] * gs, slots), dim3(kLineThreads), ap.lds[0], stream, l3);
        hipLaunchKernelGGL((cg3_dim1_kernel<1>), dim3((unsigned)g.n[0] * gs, slots), dim3(kLineThreads), ap.lds[1], stream, l3);
        hipLaunchKernelGGL(cg3_inv2_kernel, dim3(l3.nblk_lines, slots), dim3(kLineThreads), ap.lds[2], stream, l3);
        break;
    }
    case OperatorApply::kLines2: {
        LineArgs& la = ap.la;
        la.c = a;
        hipLaunchKernelGGL(cg_rows_fwd_kernel, dim3(la.nblk_rows, slots), dim3(kLineThreads), ap.lds[1], stream, la);
        hipLaunchKernelGGL(cg_cols_mid_kernel, dim3((unsigned)(g.F[1] / la.lpb), slots), dim3(kLineThreads), ap.lds[0], stream, la);
        hipLaunchKernelGGL(cg_rows_inv_kernel, dim3(la.nblk_rows, slots), dim3(kLineThreads), ap.lds[1], stream, la);
        break;
    }
    case OperatorApply::kFft: {
        hipLaunchKernelGGL(cg_pad_kernel, grid_for(g.Ftot, slots, kVecThreads), dim3(kVecThreads), 0, stream, a);
        EFGP_HIP_CHECK(hipGetLastError());
        const int rc = circulant(op, a.pad_out, slots, stream);
        if (rc != EFGP_OK) return rc;
        hipLaunchKernelGGL(cg_dot_kernel, dim3(a.nblk, slots), dim3(kVecThreads), 0, stream, a);
        break;
    }
    }
    hipLaunchKernelGGL(cg_axpy_kernel, dim3(a.nblk, slots), dim3(kVecThreads), 0, stream, a);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

// The replayed burst.  One iteration = 5 launches of ours + two rocFFT executions (~11 kernels): enqueueing them one by one costs
// the host ~300 us per iteration (measured, 3-D 64^3), far more than the GPU needs.  A full burst is therefore captured ONCE into a
// hipGraph per (slots, row map) state and replayed with one launch.  Owns the instantiated graph: every return path destroys it.
struct BurstGraph {
    efgp_toeplitz_s* op;
    hipStream_t stream;
    bool usable;                     // false: kernel timing on, EFGP_NO_CG_GRAPH, or this runtime cannot capture the sequence
    hipGraphExec_t exec = nullptr;
    int slots = -1;                  // the state `exec` was built for
    const int* rows = nullptr;
    BurstGraph(efgp_toeplitz_s* op_, hipStream_t stream_)
        : op(op_), stream(stream_), usable(!timing_enabled() && std::getenv("EFGP_NO_CG_GRAPH") == nullptr) {}
    BurstGraph(const BurstGraph&) = delete;
    BurstGraph& operator=(const BurstGraph&) = delete;
    ~BurstGraph() {
        if (!exec) return;
        TraceSpan span_destroy("hipGraphExecDestroy");
        (void)hipGraphExecDestroy(exec);
    }

    // captures and instantiates a full burst for this state; on failure `usable` goes false and nothing is held
    template <class Enqueue>
    int build(int slots_now, const int* rows_now, Enqueue& enqueue) {
        TraceSpan span_build("graph build (plan + capture + instantiate)");
        const ToepGeom& g = op->g;
        hipGraph_t graph = nullptr;
        // make sure the FFT plan exists and is bound to the stream before capturing
        int rc;
        if (own_fft_supported(g.d, g.F)) {
            rc = own_fft_prepare(op->ctx, g.d, g.F, stream);
        } else {
            hipfftHandle fh_unused;
            rc = fft_plan(op->ctx, g.d, g.F, slots_now, stream, &fh_unused);
        }
        if (rc != EFGP_OK) return rc;
        bool ok = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            int rcap = EFGP_OK;
            for (int k = 0; k < kPollEvery && rcap == EFGP_OK; ++k) rcap = enqueue();
            const hipError_t ee = hipStreamEndCapture(stream, &graph);
            ok = rcap == EFGP_OK && ee == hipSuccess && graph != nullptr;
        }
        if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) {
            (void)hipGetLastError();
            exec = nullptr;
            usable = false;            // this runtime cannot capture the sequence: enqueue directly
        } else {
            slots = slots_now;
            rows = rows_now;
        }
        return EFGP_OK;
    }

    // `burst` iterations of `slots_now` slots behind the row map `rows_now`: a full burst replays the graph (rebuilt when the state
    // changed); the tail of a solve, and every burst when graphs are not usable, is enqueued directly
    template <class Enqueue>
    int launch(int slots_now, const int* rows_now, int burst, Enqueue enqueue) {
        if (usable && burst == kPollEvery) {
            if (exec && (slots != slots_now || rows != rows_now)) {
                (void)hipGraphExecDestroy(exec);
                exec = nullptr;
            }
            if (!exec) {
                const int rc = build(slots_now, rows_now, enqueue);
                if (rc != EFGP_OK) return rc;
            }
            if (exec) {
                TraceSpan span_launch("hipGraphLaunch");
                EFGP_HIP_CHECK(hipGraphLaunch(exec, stream));
                return EFGP_OK;
            }
        }
        for (int k = 0; k < burst; ++k) {
            KernelTimer timer("cg_iteration", stream);
            const int rc = enqueue();
            if (rc != EFGP_OK) return rc;
        }
        return EFGP_OK;
    }
};

// The rows of one group that still iterate.  Until the first row leaves, slot i is row i and no map is used.
struct ActiveRows {
    int rows;
    int n_active;
    bool compacted = false;
    int last_active_it = 0;          // number of iterations in which at least one row was active
    std::vector<int> active;
    std::vector<CgRowScalars> hsc;   // the scalars as last polled
    explicit ActiveRows(int rows_) : rows(rows_), n_active(rows_), active(rows_), hsc(rows_) {
        for (int i = 0; i < rows; ++i) active[i] = i;
    }
    // FFT batch = number of slots (bucketed to a power of two to bound the number of plans)
    int slots() const {
        if (!compacted) return n_active;
        int p2 = 1;
        while (p2 < n_active) p2 <<= 1;
        return std::min(p2, rows);
    }
};

// Reads the scalars of every row (the wait orders the host behind the burst), rebuilds the active list and, when rows have left,
// uploads the slot -> row map to d_rows and points a.rows at it.  Returns the new active count, or a negative error.
static int poll_and_compact(ActiveRows& st, CgArgs& a, int* d_rows, int* host, hipStream_t stream) {
    {
        TraceSpan span_poll("poll (D2H scalars + stream synchronize)");
        // into the context's PINNED buffer (a pageable destination is staged by the runtime on every call)
        EFGP_HIP_CHECK(hipMemcpyAsync(host, a.sc, (size_t)st.rows * sizeof(CgRowScalars), hipMemcpyDeviceToHost, stream));
        EFGP_HIP_CHECK(stream_wait(stream));
        std::memcpy(st.hsc.data(), host, (size_t)st.rows * sizeof(CgRowScalars));
    }
    int new_active = 0;
    for (int i = 0; i < st.rows; ++i) {
        if (st.hsc[i].active) st.active[new_active++] = i;
        st.last_active_it = std::max(st.last_active_it, st.hsc[i].iters);
    }
    if ((new_active != st.n_active || !st.compacted) && new_active > 0 && new_active < st.rows) {
        int p2 = 1;
        while (p2 < new_active) p2 <<= 1;
        const int nslots = std::min(p2, st.rows);
        std::vector<int> map(nslots, -1);
        for (int i = 0; i < new_active; ++i) map[i] = st.active[i];
        std::memcpy(host, map.data(), nslots * sizeof(int));
        EFGP_HIP_CHECK(hipMemcpyAsync(d_rows, host, nslots * sizeof(int), hipMemcpyHostToDevice, stream));
        EFGP_HIP_CHECK(stream_wait(stream));
        a.rows = d_rows;
        st.compacted = true;
    }
    st.n_active = new_active;
    return new_active;
}

// One group of `rows` systems (from row r0 of the solve) whose padded grids fit the scratch: lay out the scratch, initialise, then
// bursts of iterations with a poll and a compaction behind each.  st->hsc holds the final scalars.  shape_rows: the size of a full
// group of this solve, which the launch shapes follow -- a short last group sums in the order of the full ones, so a system's
// bits do not depend on the group it falls into.
static int solve_group(efgp_toeplitz_s* op, const CgSolve& s, int64_t r0, ActiveRows* st, int shape_rows, hipStream_t stream) {
    DeviceCtx* ctx = op->ctx;
    const ToepGeom g = op->g;
    const int rows = st->rows;
    double2* pad = (double2*)scratch(ctx, SLOT_TOEP_PAD, (size_t)rows * (size_t)g.Ftot * sizeof(double2));
    double2* vec = (double2*)scratch(ctx, SLOT_CG_VEC, (size_t)3 * rows * (size_t)g.M * sizeof(double2));
    // scalars | status (64 B) + slot->row map | arrival counters | per-workgroup partial sums
    const size_t off_status = ((size_t)rows * sizeof(CgRowScalars) + 63) & ~size_t(63);
    const size_t off_counter = off_status + 64 + (((size_t)rows * sizeof(int) + 63) & ~size_t(63));
    const size_t off_partial = off_counter + (((size_t)2 * rows * sizeof(int) + 63) & ~size_t(63));
    const size_t sc_bytes = off_partial + (size_t)rows * 3 * kCgBlocksMax * sizeof(double);
    char* scb = (char*)scratch(ctx, SLOT_CG_SCALARS, sc_bytes);
    int* host = pinned_host(ctx, (size_t)rows * sizeof(CgRowScalars) + 64);
    if (!pad || !vec || !scb || !host) return EFGP_ENOMEM;
    CgArgs a;
    a.g = g;
    a.ws = s.ws;
    a.diag = s.diag;
    a.sigmasq = s.sigmasq;
    a.variant = s.variant;
    a.tol = s.tol;
    a.early_stop = s.early_stop;
    a.batched = s.batched;
    a.b = s.b + r0 * g.M;
    a.x = s.x + r0 * g.M;
    a.r = vec;
    a.p = vec + (int64_t)rows * g.M;
    a.ap = vec + (int64_t)2 * rows * g.M;
    a.pad = pad;
    a.pad_out = pad;
    a.rows = nullptr;
    a.hist = r0 == 0 ? cg_history().buf : nullptr;
    a.hist_cap = cg_history().capacity;
    a.sc = (CgRowScalars*)scb;
    a.status = (int*)(scb + off_status);
    int* d_rows = a.status + 16;
    a.counter = (int*)(scb + off_counter);
    a.partial = (double*)(scb + off_partial);
    a.v_off = 0;
    a.v_len = g.M;
    a.v_w1 = g.M;
    a.nblk = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(64 /* update kernels: measured optimum */, (g.M + kVecThreads - 1) / kVecThreads),
                                                        std::max<int64_t>(1, 1024 / shape_rows)));
    EFGP_HIP_CHECK(hipMemsetAsync(a.status, 0, off_partial - off_status, stream));      // status, map, counters

    // r0 = b - A x0
    hipLaunchKernelGGL(pad_scale_kernel, grid_for(g.Ftot, rows, kVecThreads), dim3(kVecThreads), 0, stream, g,
                       (const double2*)a.x, g.M, a.ws, (const int*)nullptr, (const int*)nullptr, pad, 1.0);
    EFGP_HIP_CHECK(hipGetLastError());
    int rc = circulant(op, pad, rows, stream);
    if (rc != EFGP_OK) return rc;
    hipLaunchKernelGGL(cg_init_kernel, dim3(a.nblk, rows), dim3(kVecThreads), 0, stream, a);
    EFGP_HIP_CHECK(hipGetLastError());

    OperatorApply ap;
    rc = setup_apply(op, s, a, rows, shape_rows, host, stream, &ap);
    if (rc != EFGP_OK) return rc;
    // iteration loop; active rows are compacted on the host whenever the status is polled
    BurstGraph graph(op, stream);
    for (int it = 0; it < s.max_iter && st->n_active > 0;) {
        const int burst = std::min(kPollEvery, s.max_iter - it);
        const int slots = st->slots();
        rc = graph.launch(slots, a.rows, burst, [&]() { return enqueue_iteration(op, ap, a, slots, stream); });
        if (rc != EFGP_OK) return rc;
        it += burst;
        rc = poll_and_compact(*st, a, d_rows, host, stream);
        if (rc < 0) return rc;
    }
    if (ap.kind == OperatorApply::kLines3H) {          // the planes k0 < 0 of the solutions
        CgArgs am = a;
        am.rows = nullptr;
        hipLaunchKernelGGL(cg3h_mirror_kernel, dim3(64, rows), dim3(kVecThreads), 0, stream, am);
        EFGP_HIP_CHECK(hipGetLastError());
        EFGP_HIP_CHECK(stream_wait(stream));
    }
    return EFGP_OK;
}

// The multi-launch solve of s.nbatch systems on any grid; returns when they are solved.  The counts follow the reference's two
// conventions (cg.py:152 single; cg.py:193-199,243 batched: +1 for the terminating pass).
int solve_multi_launch(efgp_toeplitz_s* op, const CgSolve& s, int* iters_out, int* row_iters_out, hipStream_t stream) {
    DeviceCtx* ctx = op->ctx;
    // The iteration bursts are replayed as hipGraphs, which cannot be captured on the legacy default stream:
    // run the multi-kernel solve on a side stream ordered after the caller's stream (the final poll of every group
    // synchronises the host with it, so later work on the caller's stream is ordered after the solve).
    if (!timing_enabled() && std::getenv("EFGP_NO_CG_GRAPH") == nullptr) {
        if (!ctx->aux_stream) {
            if (hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&ctx->aux_event, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                ctx->aux_stream = nullptr;
            }
        }
        if (ctx->aux_stream) {
            EFGP_HIP_CHECK(hipEventRecord(ctx->aux_event, stream));
            EFGP_HIP_CHECK(hipStreamWaitEvent(ctx->aux_stream, ctx->aux_event, 0));
            stream = ctx->aux_stream;
        }
    }
    // rows are processed in groups whose padded grids fit ~512 MB of scratch and whose systems fit gridDim.y
    const int64_t group_cap = std::max<int64_t>(1, std::min<int64_t>(kMaxGridRows, (int64_t)(512ll << 20) / (op->g.Ftot * (int64_t)sizeof(double2))));
    const int shape_rows = (int)std::min<int64_t>(group_cap, s.nbatch);
    int global_iters = 0;
    for (int64_t r0 = 0; r0 < s.nbatch; r0 += group_cap) {
        ActiveRows st((int)std::min<int64_t>(group_cap, s.nbatch - r0));
        const int rc = solve_group(op, s, r0, &st, shape_rows, stream);
        if (rc != EFGP_OK) return rc;
        int group_iters;
        if (!s.batched) {
            group_iters = st.hsc[0].iters;       // (max_iter >= 1 and rows >= 1: at least one burst ran and was polled)
        } else {
            group_iters = st.last_active_it;
            if (st.n_active == 0 && st.last_active_it < s.max_iter) group_iters = st.last_active_it + 1;
        }
        if (row_iters_out)
            for (int i = 0; i < st.rows; ++i) row_iters_out[r0 + i] = st.hsc[i].iters;
        global_iters = std::max(global_iters, group_iters);
    }
    if (iters_out) *iters_out = global_iters;
    return EFGP_OK;
}

}  // namespace efgp
