// d-dimensional Toeplitz mat-vec by circulant embedding (hipFFT/rocFFT) and the Jacobi-preconditioned
// CG solver of the EFGP normal equations, for gfx950.
//
// Replaces ToeplitzND (efgpnd.py:1239-1393), create_Gv/A_mean/A_var/jacobi (efgpnd.py:1572-1631) and
// ConjugateGradients.solve (cg.py:86-244).
//
// Data layout in HBM
//   vhat   [prod F]   complex: FFT of the zero-padded Toeplitz vector, pre-divided by prod F
//   pad    [rows][prod F] complex: zero-padded operand / FFT work buffer (library scratch)
//   x,r,p,Ap [rows][M] complex, M = prod n; per-row scalars (rz, |b|, flags) in a small scratch array
// The whole iteration state lives on the device; the host only launches kernels and polls a status
// word every few iterations.  Per iteration and row: one pad+scale kernel, two batched FFTs, one
// spectral multiply, one fused update kernel (crop, A p, <p,Ap>, x/r update, norms, p update).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

#include <cstdlib>

#include "cg_plan_host.hpp"
#include "common.hpp"
#include "line_fft.hpp"
#include "toeplitz_cg.hpp"
#include "toeplitz_line_dev.hpp"
#include "toeplitz_op.hpp"

namespace efgp {

// pad[row][:] = 0 except the leading n-box which receives scale .* src[rows[row]]
// (scale may be null), times the real `factor`.  One launch covers all rows: grid = (blocks, nrows).
__global__ void pad_scale_kernel(ToepGeom g, const double2* __restrict__ src, int64_t src_stride,
                                 const double2* __restrict__ scale, const int* __restrict__ rows,
                                 const int* __restrict__ row_active, double2* __restrict__ pad, double factor) {
    const int slot = blockIdx.y;
    const int row = rows ? rows[slot] : slot;
    if (row < 0) return;
    if (row_active && !row_active[row]) return;
    double2* P = pad + (int64_t)slot * g.Ftot;
    const double2* S = src + (int64_t)row * src_stride;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.Ftot; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t rem = t, flat = 0;
        bool inside = true;
        // decompose t over F (row-major) and test against n
        int64_t coords[3];
        for (int a = g.d - 1; a >= 0; --a) {
            coords[a] = rem % g.F[a];
            rem /= g.F[a];
            inside = inside && coords[a] < g.n[a];
        }
        double2 v = make_double2(0.0, 0.0);
        if (inside) {
            for (int a = 0; a < g.d; ++a) flat = flat * g.n[a] + coords[a];
            v = S[flat];
            if (scale) v = cmul(v, scale[flat]);
            v.x *= factor;
            v.y *= factor;
        }
        P[t] = v;
    }
}

__global__ void spectral_mul_kernel(int64_t Ftot, const double2* __restrict__ vhat, double2* __restrict__ pad) {
    double2* P = pad + (int64_t)blockIdx.y * Ftot;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < Ftot; t += (int64_t)gridDim.x * blockDim.x)
        P[t] = cmul(P[t], vhat[t]);
}

// y[row][flat] = pad[row][flat index shifted by n-1]
__global__ void crop_kernel(ToepGeom g, const double2* __restrict__ pad, double2* __restrict__ y) {
    const int row = blockIdx.y;
    const double2* P = pad + (int64_t)row * g.Ftot;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.M; t += (int64_t)gridDim.x * blockDim.x)
        y[(int64_t)row * g.M + t] = P[pad_index(g, t, 1)];
}

// efgp_toeplitz_apply_scaled on grids without the single-launch kernel: the diagonals ride in the pad and crop passes
// pad[row] = 0 except the leading n-box = pre .* x[row] (x real or complex)
template <bool REAL>
__global__ void pad_pre_kernel(ToepGeom g, const void* __restrict__ src, const double2* __restrict__ pre, double2* __restrict__ pad) {
    const int row = blockIdx.y;
    double2* P = pad + (int64_t)row * g.Ftot;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.Ftot; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t rem = t, flat = 0, coords[3];
        bool inside = true;
        for (int a = g.d - 1; a >= 0; --a) {
            coords[a] = rem % g.F[a];
            rem /= g.F[a];
            inside = inside && coords[a] < g.n[a];
        }
        double2 v = make_double2(0.0, 0.0);
        if (inside) {
            for (int a = 0; a < g.d; ++a) flat = flat * g.n[a] + coords[a];
            if (REAL) v = make_double2(((const double*)src)[(int64_t)row * g.M + flat], 0.0);
            else v = ((const double2*)src)[(int64_t)row * g.M + flat];
            if (pre) v = cmul(v, pre[flat]);
        }
        P[t] = v;
    }
}
// y[row] = post .* window of pad[row]
__global__ void crop_post_kernel(ToepGeom g, const double2* __restrict__ pad, const double2* __restrict__ post, double2* __restrict__ y) {
    const int row = blockIdx.y;
    const double2* P = pad + (int64_t)row * g.Ftot;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < g.M; t += (int64_t)gridDim.x * blockDim.x) {
        double2 v = P[pad_index(g, t, 1)];
        if (post) v = cmul(v, post[t]);
        y[(int64_t)row * g.M + t] = v;
    }
}

// vhat_c[f] = vhat[f] e^(2 pi i (f0 (n0-1)/F0 + f1 (n1-1)/F1)): the spectrum of the Toeplitz vector circularly shifted so that the
// crop window of the product sits at [0, n) -- real for the Hermitian vectors of EFGP; the cooperative solve multiplies by it
// and reads <w, T w> = sum_f Re(vhat_c) |w^|^2 off the forward transform (Parseval)
__global__ __launch_bounds__(256) void center_spectrum_kernel(const double2* __restrict__ vhat, const double2* __restrict__ tw0,
                                                              const double2* __restrict__ tw1, int n0, int n1, int F0, int F1,
                                                              double2* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)F0 * F1) return;
    const int f0 = (int)(t / F1), f1 = (int)(t - (int64_t)f0 * F1);
    const double2 a = tw0[((int64_t)(n0 - 1) * f0) % F0], b = tw1[((int64_t)(n1 - 1) * f1) % F1];
    const double2 ph = make_double2(a.x * b.x - a.y * b.y, -(a.x * b.y + a.y * b.x));      // conj(a b)
    out[t] = cmul(vhat[t], ph);
}

template <bool AC, bool BC>
__global__ void vdot_real_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                 double* __restrict__ partial) {
    __shared__ double red[kVecThreads / 64];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double ar, ai = 0.0, br, bi = 0.0;
        if (AC) {
            double2 u = reinterpret_cast<const double2*>(a)[i];
            ar = u.x;
            ai = u.y;
        } else {
            ar = a[i];
        }
        if (BC) {
            double2 v = reinterpret_cast<const double2*>(b)[i];
            br = v.x;
            bi = v.y;
        } else {
            br = b[i];
        }
        acc += ar * br + ai * bi;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

}  // namespace efgp

using namespace efgp;

// exp(-2 pi i q / n), q < n, on the device (cached per context)
static double2* twiddle_table_for(DeviceCtx* ctx, int64_t n, hipStream_t stream) {
    auto it = ctx->twiddles.find(n);
    if (it != ctx->twiddles.end()) return (double2*)it->second;
    std::vector<double2> tw((size_t)n);
    const long double two_pi = 2.0L * acosl(-1.0L);
    for (int64_t q = 0; q < n; ++q) {
        long double ang = -two_pi * (long double)q / (long double)n;
        tw[(size_t)q] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    double2* dtw = nullptr;
    if (hipMalloc((void**)&dtw, (size_t)n * sizeof(double2)) != hipSuccess ||
        hipMemcpyAsync(dtw, tw.data(), (size_t)n * sizeof(double2), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        if (dtw) (void)hipFree(dtw);
        (void)hipGetLastError();
        return nullptr;
    }
    ctx->twiddles[n] = dtw;
    return dtw;
}

// a deferred operator's spectra, made on first use by any entry other than the fused mean solve: the 64 x 64 one, and the 48 x 48
// one in the same launch unless the fused solve has made it.  On the caller's stream: its DeviceGuard has handed the context over
// from the stream the operator was made on (stream_handover), as for the deferred reference-grid spectrum below.
static int ensure_deferred_spectra(efgp_toeplitz_s* op, hipStream_t stream) {
    if (!op->pair_pending) return EFGP_OK;
    const int L0 = (int)op->Ls[0], L1 = (int)op->Ls[1];
    const int rc = op->vhat48_ready ? toeplitz_vhat_fused_launch(op->v_ref, L0, L1, 1.0 / (double)kCells64, op->pair_target, stream)
                                    : toeplitz_vhat_pair_launch(op->v_ref, L0, L1, op->pair_target, op->vhat48, stream);
    if (rc != EFGP_OK) return rc;
    op->pair_pending = false;
    op->vhat48_ready = true;
    op->v_ref = nullptr;
    return EFGP_OK;
}

// geometry, twiddles and spectrum the single-launch kernels use for this operator: the 64 x 64 embedding where there is one
struct CgGrid {
    const ToepGeom& g;
    const double2* const* tw;
    const double2* vhat;
};
static CgGrid cg_grid(const efgp_toeplitz_s* op) {
    if (op->cg64) return {op->g_cg, (const double2* const*)op->tw_cg, op->vhat_cg};
    return {op->g, (const double2* const*)op->tw, op->vhat};
}

// the two single-launch solves an operator may offer, each with its test hooks
static bool persistent_usable(const efgp_toeplitz_s* op) { return op->persistent_ok && std::getenv("EFGP_NO_PERSISTENT_CG") == nullptr; }
static bool coop_usable(const efgp_toeplitz_s* op) {
    return op->lines_ok && std::getenv("EFGP_NO_CG_COOP") == nullptr && std::getenv("EFGP_NO_CG_LINES") == nullptr;
}

// the arguments every exported solve shares, in the C ABI's order, with the default iteration cap
static CgSolve make_solve(const efgp_toeplitz_s* op, const void* ws, double sigmasq, int variant, const double* diag, const void* b, void* x,
                          int nbatch, double tol, int max_iter, int early_stop, int batched) {
    CgSolve s;
    s.ws = (const double2*)ws;
    s.sigmasq = sigmasq;
    s.variant = variant;
    s.diag = diag;
    s.b = (const double2*)b;
    s.x = (double2*)x;
    s.nbatch = nbatch;
    s.tol = tol;
    s.max_iter = max_iter;
    s.early_stop = early_stop;
    s.batched = batched;
    s.default_max_iter(op->g.M);
    return s;
}

// Enqueues the persistent single-launch solve of `s` on the operator's CG grid (persistent_usable(op)); counts go to d_iters
// (device, s.nbatch ints).  lz: Lanczos mode.  fuse: the fused mean solve, which makes the 48 x 48 spectrum itself and reads no
// other -- what is deferred stays deferred.
static int enqueue_persistent(efgp_toeplitz_s* op, const CgSolve& s, int* d_iters, hipStream_t stream, const LanczosOut* lz = nullptr,
                              const MeanFusedOperands* fuse = nullptr) {
    KernelTimer timer("cg_persistent", stream);
    if (!fuse) {
        const int rc = ensure_deferred_spectra(op, stream);
        if (rc != EFGP_OK) return rc;
    }
    const CgGrid q = cg_grid(op);
    return persistent_cg_launch(q.g, q.tw, fuse ? nullptr : q.vhat, op->h48.vhat ? &op->h48 : nullptr, s, d_iters, stream, lz, fuse);
}

namespace efgp {

// out = FFT(zero-padded v) / Ftot on grid g: the pad kernel with the lag box as its block (n := L; the inverse transform's 1 / Ftot
// folded in before the FFT), then the transform
static int make_spectrum(efgp_toeplitz_s* op, const ToepGeom& g, const double2* v, double2* out, hipStream_t stream) {
    const ToepGeom gv = lag_geometry(g, op->Ls);
    hipLaunchKernelGGL(pad_scale_kernel, grid_for(g.Ftot, 1, kVecThreads), dim3(kVecThreads), 0, stream, gv, v, gv.M, (const double2*)nullptr,
                       (const int*)nullptr, (const int*)nullptr, out, 1.0 / (double)g.Ftot);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("Toeplitz spectrum: pad launch failed: %s", hipGetErrorString(e));
        return EFGP_EHIP;
    }
    return fft_c2c(op->ctx, g.d, g.F, 1, out, true, stream);
}

// the spectrum on the reference's grid, made on first use when the operator was created with a smaller cooperative grid
// (efgp_toeplitz_create_ex)
int ensure_reference_spectrum(efgp_toeplitz_s* op, hipStream_t stream) {
    const int rcd = ensure_deferred_spectra(op, stream);
    if (rcd != EFGP_OK) return rcd;
    if (op->vhat_ready) return EFGP_OK;
    const int rc = make_spectrum(op, op->g, op->v_keep, op->vhat, stream);
    if (rc != EFGP_OK) return rc;
    op->vhat_ready = true;
    pool_free(op->ctx, op->v_keep, op->v_keep_bytes);        // stream-ordered reuse: the pad launch above read it on this stream
    op->v_keep = nullptr;
    return EFGP_OK;
}

// pad = FFT^-1( FFT(pad) .* vhat ) for `slots` rows
int circulant(efgp_toeplitz_s* op, double2* pad, int slots, hipStream_t stream) {
    // in-house transforms know the padding: the input is non-zero on [0, n) per axis, the product is read on [n - 1, 2 n - 1)
    const bool own = own_fft_supported(op->g.d, op->g.F) && std::getenv("EFGP_NO_PRUNED_FFT") == nullptr;
    int64_t lo_in[3] = {0, 0, 0}, lo_out[3], cnt[3];
    for (int a = 0; a < 3; ++a) {
        cnt[a] = a < op->g.d ? op->g.n[a] : 1;
        lo_out[a] = a < op->g.d ? std::min(op->g.n[a] - 1, op->g.F[a] - op->g.n[a]) : 0;
    }
    int rc = ensure_reference_spectrum(op, stream);
    if (rc != EFGP_OK) return rc;
    rc = own ? own_fft_exec_windowed(op->ctx, op->g.d, op->g.F, slots, pad, true, lo_in, cnt, false, stream)
             : fft_c2c(op->ctx, op->g.d, op->g.F, slots, pad, true, stream);
    if (rc != EFGP_OK) return rc;
    hipLaunchKernelGGL(spectral_mul_kernel, grid_for(op->g.Ftot, slots, kVecThreads), dim3(kVecThreads), 0, stream,
                       op->g.Ftot, (const double2*)op->vhat, pad);
    EFGP_HIP_CHECK(hipGetLastError());
    return own ? own_fft_exec_windowed(op->ctx, op->g.d, op->g.F, slots, pad, false, lo_out, cnt, true, stream)
               : fft_c2c(op->ctx, op->g.d, op->g.F, slots, pad, false, stream);
}

// vhat_c = vhat rotated so that the circular convolution has its crop window at [0, n) (cooperative solve on the reference's grid)
bool ensure_centred_spectrum(efgp_toeplitz_s* op, hipStream_t stream) {
    if (op->vhat_c) return true;
    if (ensure_reference_spectrum(op, stream) != EFGP_OK) return false;
    op->vhat_c = (double2*)pool_alloc(op->ctx, spectrum_bytes(op->g));
    if (!op->vhat_c) return false;
    hipLaunchKernelGGL(center_spectrum_kernel, dim3((unsigned)((op->g.Ftot + 255) / 256)), dim3(256), 0, stream, op->vhat, op->tw[0],
                       op->tw[1], (int)op->g.n[0], (int)op->g.n[1], (int)op->g.F[0], (int)op->g.F[1], op->vhat_c);
    if (hipGetLastError() != hipSuccess) {
        pool_free(op->ctx, op->vhat_c, spectrum_bytes(op->g));
        op->vhat_c = nullptr;
        return false;
    }
    return true;
}

// ---- operator creation: the steps of efgp_toeplitz_create_ex, in its order -------------------------------------------------------
// A step that cannot be taken (no twiddle table, no pooled block, a failed launch) takes back what the plan decided on it.

// block and twiddles of the 48 x 48 spectrum
static void take_spectrum48(efgp_toeplitz_s* op, hipStream_t stream) {
    const double2* tw48 = twiddle_table_for(op->ctx, 48, stream);
    op->vhat48 = tw48 ? (double2*)pool_alloc(op->ctx, kSpectrum48Bytes) : nullptr;
    if (op->vhat48) op->h48.tw = tw48;
}

// a copy of the lags, for the reference grid's spectrum on first use; false (nothing kept) when it cannot be made
static bool keep_lags(efgp_toeplitz_s* op, size_t bytes, const void* v, hipStream_t stream) {
    op->v_keep_bytes = bytes;
    op->v_keep = (double2*)pool_alloc(op->ctx, bytes);
    const bool ok = op->v_keep != nullptr && hipMemcpyAsync(op->v_keep, v, bytes, hipMemcpyDeviceToDevice, stream) == hipSuccess;
    if (!ok && op->v_keep) {
        pool_free(op->ctx, op->v_keep, bytes);
        op->v_keep = nullptr;
    }
    op->vhat_ready = !ok;
    return ok;
}

// The spectrum of a 64 x 64 grid (`target`: the own grid's, or the embedding's) in one launch.  While the 48 x 48 spectrum has a
// block and is still to be made, the same launch carries it -- or, deferred, both are left pending (ensure_deferred_spectra).
static int make_spectrum64(efgp_toeplitz_s* op, double2* target, const double2* v, bool defer_pair, bool* made48, hipStream_t stream) {
    const int L0 = (int)op->Ls[0], L1 = (int)op->Ls[1];
    if (!op->vhat48 || *made48) return toeplitz_vhat_fused_launch(v, L0, L1, 1.0 / (double)kCells64, target, stream);
    if (defer_pair) {
        op->pair_pending = true;
        op->pair_target = target;
        *made48 = true;
        return EFGP_OK;
    }
    const int rc = toeplitz_vhat_pair_launch(v, L0, L1, target, op->vhat48, stream);
    *made48 = rc == EFGP_OK;
    return rc;
}

// twiddle tables of the own grid; without one, none of the kernels that transform in LDS runs
static void take_twiddles(efgp_toeplitz_s* op, const OperatorPlan& pl, hipStream_t stream) {
    op->persistent_ok = pl.eligible;
    op->lines_ok = pl.lines_ok;
    op->lines3_ok = pl.lines3_ok;
    if (!op->persistent_ok && !op->lines_ok && !op->lines3_ok) return;
    for (int a = 0; a < op->g.d; ++a) {
        op->tw[a] = twiddle_table_for(op->ctx, op->g.F[a], stream);
        if (op->tw[a]) continue;
        op->persistent_ok = op->lines_ok = op->lines3_ok = false;
        return;
    }
}

// the cooperative solve's smaller grid: twiddles, block, and the spectrum there with the centring rotation in place
static void make_small_coop_grid(efgp_toeplitz_s* op, const OperatorPlan& pl, const double2* v, hipStream_t stream) {
    DeviceCtx* ctx = op->ctx;
    op->g_co = pl.g_co;
    op->tw_co[0] = twiddle_table_for(ctx, op->g_co.F[0], stream);
    op->tw_co[1] = twiddle_table_for(ctx, op->g_co.F[1], stream);
    op->vhat_co = (op->tw_co[0] && op->tw_co[1]) ? (double2*)pool_alloc(ctx, pl.vhat_co_bytes) : nullptr;
    if (!op->vhat_co) return;
    bool ok = make_spectrum(op, op->g_co, v, op->vhat_co, stream) == EFGP_OK;
    if (ok) {
        hipLaunchKernelGGL(center_spectrum_kernel, dim3((unsigned)((op->g_co.Ftot + 255) / 256)), dim3(256), 0, stream, op->vhat_co,
                           op->tw_co[0], op->tw_co[1], (int)op->g.n[0], (int)op->g.n[1], (int)op->g_co.F[0], (int)op->g_co.F[1],
                           op->vhat_co);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok) {
        op->coop_small = true;
        return;
    }
    (void)hipGetLastError();
    pool_free(ctx, op->vhat_co, pl.vhat_co_bytes);
    op->vhat_co = nullptr;
}

// the 64 x 64 embedding of the single-launch solves: block, twiddles, spectrum (any of them missing: they stay on the own grid)
static void make_embedding64(efgp_toeplitz_s* op, const OperatorPlan& pl, const double2* v, bool defer_pair, bool* made48, hipStream_t stream) {
    DeviceCtx* ctx = op->ctx;
    op->g_cg = pl.g_cg;
    op->vhat_cg = (double2*)pool_alloc(ctx, kSpectrum64Bytes);
    bool ok = op->vhat_cg != nullptr;
    if (ok) {
        op->tw_cg[0] = op->tw_cg[1] = twiddle_table_for(ctx, 64, stream);
        ok = op->tw_cg[0] != nullptr;
    }
    if (ok) ok = make_spectrum64(op, op->vhat_cg, v, defer_pair, made48, stream) == EFGP_OK;
    if (ok) {
        op->cg64 = true;
        return;
    }
    (void)hipGetLastError();
    if (op->vhat_cg) pool_free(ctx, op->vhat_cg, kSpectrum64Bytes);
    op->vhat_cg = nullptr;
}

// pending spectra read the caller's lags on first use; a 48 x 48 block that no 64 x 64 launch carries (grid not on the fused path)
// goes back: the Hermitian solves keep 64 x 64
static void settle_spectrum48(efgp_toeplitz_s* op, const double2* v, bool made48) {
    if (op->pair_pending) {
        op->v_ref = v;
        op->vhat48_ready = false;
    }
    if (op->vhat48 && made48) {
        op->h48.vhat = op->vhat48;
    } else if (op->vhat48) {
        pool_free(op->ctx, op->vhat48, kSpectrum48Bytes);
        op->vhat48 = nullptr;
    }
}

}  // namespace efgp

extern "C" {

int efgp_toeplitz_create(efgp_toeplitz_t** op_out, int device, int dim, const int64_t* Ls, const void* v,
                         int force_pow2, void* stream_) {
    return efgp_toeplitz_create_ex(op_out, device, dim, Ls, v, force_pow2, 0, stream_);
}

int efgp_toeplitz_create_ex(efgp_toeplitz_t** op_out, int device, int dim, const int64_t* Ls, const void* v_, int force_pow2, int flags,
                            void* stream_) {
    EFGP_REQUIRE(op_out && Ls && v_, "efgp_toeplitz_create: null argument");
    EFGP_REQUIRE((flags & ~EFGP_TOEPLITZ_DEFER_SPECTRA) == 0, "efgp_toeplitz_create_ex: unknown flags %d", flags);
    EFGP_REQUIRE(dim >= 1 && dim <= 3, "efgp_toeplitz_create: dim must be 1, 2 or 3 (got %d)", dim);
    for (int a = 0; a < dim; ++a) EFGP_REQUIRE(Ls[a] >= 1, "efgp_toeplitz_create: Ls[%d] < 1", a);
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    hipStream_t stream = (hipStream_t)stream_;
    const double2* v = (const double2*)v_;
    DeviceGuard guard(device, stream);
    const OperatorPlan pl = plan_operator(dim, Ls, force_pow2, flags);
    auto* op = new efgp_toeplitz_s();
    op->device = device;
    op->ctx = ctx;
    op->g = pl.g;
    for (int a = 0; a < 3; ++a) op->Ls[a] = pl.Ls[a];
    auto fail = [op](int rc) {          // every failure frees what was taken so far
        efgp_toeplitz_destroy(op);
        return rc;
    };
    op->vhat = (double2*)pool_alloc(ctx, pl.vhat_bytes);
    if (!op->vhat) return fail(EFGP_ENOMEM);
    if (pl.want48) take_spectrum48(op, stream);
    const bool defer_pair = pl.defer_pair && op->vhat48 != nullptr;
    bool made48 = false;
    int rc = EFGP_OK;
    if (pl.defer_ref && keep_lags(op, pl.v_keep_bytes, v, stream)) {
        // nothing now: ensure_reference_spectrum
    } else if (pl.vhat_fused) {
        rc = make_spectrum64(op, op->vhat, v, defer_pair, &made48, stream);
    } else {
        rc = make_spectrum(op, op->g, v, op->vhat, stream);
    }
    if (rc != EFGP_OK) return fail(rc);
    take_twiddles(op, pl, stream);
    if (op->lines_ok && pl.coop_small) make_small_coop_grid(op, pl, v, stream);
    // the centred spectrum on the reference's grid: needed by the cooperative solve only when it runs there (no smaller grid, or
    // EFGP_NO_COOP_SMALL later on: built on first use then)
    if (!op->vhat_ready && !op->coop_small && (rc = ensure_reference_spectrum(op, stream)) != EFGP_OK) return fail(rc);
    if (op->lines_ok && !op->coop_small) (void)ensure_centred_spectrum(op, stream);
    if (pl.embed64 && op->persistent_ok) make_embedding64(op, pl, v, defer_pair, &made48, stream);
    // a grid of one cell without the embedding: no transform stage for the single-launch kernels (plan_operator)
    if (op->g.Ftot == 1 && !op->cg64) op->persistent_ok = false;
    settle_spectrum48(op, v, made48);
    *op_out = op;
    return EFGP_OK;
}

int efgp_toeplitz_destroy(efgp_toeplitz_t* op) {
    if (!op) return EFGP_OK;
    DeviceGuard guard(op->device);
    // the spectrum block goes back to the pool; work already enqueued on the caller's stream that reads it
    // finishes before any later enqueue on that stream can overwrite a recycled block (single stream)
    if (op->vhat) pool_free(op->ctx, op->vhat, spectrum_bytes(op->g));
    if (op->vhat_cg) pool_free(op->ctx, op->vhat_cg, kSpectrum64Bytes);
    if (op->vhat48) pool_free(op->ctx, op->vhat48, kSpectrum48Bytes);
    if (op->vhat_c) pool_free(op->ctx, op->vhat_c, spectrum_bytes(op->g));
    if (op->vhat_co) pool_free(op->ctx, op->vhat_co, spectrum_bytes(op->g_co));
    if (op->v_keep) pool_free(op->ctx, op->v_keep, op->v_keep_bytes);
    if (op->vc3) pool_free(op->ctx, op->vc3, real_spectrum_bytes(op->g));
    delete op;
    return EFGP_OK;
}

int efgp_toeplitz_fft_shape(efgp_toeplitz_t* op, int64_t* shape_out) {
    EFGP_REQUIRE(op && shape_out, "efgp_toeplitz_fft_shape: null argument");
    for (int a = 0; a < op->g.d; ++a) shape_out[a] = op->g.F[a];
    return EFGP_OK;
}

int efgp_toeplitz_single_launch_solves(efgp_toeplitz_t* op) {
    EFGP_REQUIRE(op, "efgp_toeplitz_single_launch_solves: null argument");
    return persistent_usable(op) ? 1 : 0;
}

int efgp_toeplitz_cg_shape(efgp_toeplitz_t* op, int hermitian, int64_t* shape_out) {
    EFGP_REQUIRE(op && shape_out, "efgp_toeplitz_cg_shape: null argument");
    cg_solve_shape(op->g, op->persistent_ok, op->h48.vhat != nullptr, op->cg64, op->coop_small ? &op->g_co : nullptr, hermitian, shape_out);
    return EFGP_OK;
}

int efgp_toeplitz_apply(efgp_toeplitz_t* op, const void* x, int nbatch, void* y, void* stream_) {
    EFGP_REQUIRE(op && x && y, "efgp_toeplitz_apply: null argument");
    EFGP_REQUIRE(nbatch >= 1, "efgp_toeplitz_apply: nbatch must be >= 1");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, (hipStream_t)stream_);
    // bound the scratch: process rows in chunks of at most ~256 MB of padded grid, and of at most the rows gridDim.y holds
    const int64_t max_rows = std::max<int64_t>(1, std::min<int64_t>(kMaxGridRows, (int64_t)(256ll << 20) / (op->g.Ftot * (int64_t)sizeof(double2))));
    for (int64_t r0 = 0; r0 < nbatch; r0 += max_rows) {
        const int rows = (int)std::min<int64_t>(max_rows, nbatch - r0);
        double2* pad = (double2*)scratch(op->ctx, SLOT_TOEP_PAD, (size_t)rows * (size_t)op->g.Ftot * sizeof(double2));
        if (!pad) return EFGP_ENOMEM;
        hipLaunchKernelGGL(pad_scale_kernel, grid_for(op->g.Ftot, rows, kVecThreads), dim3(kVecThreads), 0, stream, op->g,
                           (const double2*)x + r0 * op->g.M, op->g.M, (const double2*)nullptr, (const int*)nullptr,
                           (const int*)nullptr, pad, 1.0);
        EFGP_HIP_CHECK(hipGetLastError());
        int rc = circulant(op, pad, rows, stream);
        if (rc != EFGP_OK) return rc;
        hipLaunchKernelGGL(crop_kernel, grid_for(op->g.M, rows, kVecThreads), dim3(kVecThreads), 0, stream, op->g,
                           (const double2*)pad, (double2*)y + r0 * op->g.M);
        EFGP_HIP_CHECK(hipGetLastError());
    }
    return EFGP_OK;
}

int efgp_toeplitz_apply_scaled(efgp_toeplitz_t* op, const void* x, int x_is_real, int nbatch, const void* pre, const void* post,
                               void* y, void* stream_) {
    EFGP_REQUIRE(op && x && y, "efgp_toeplitz_apply_scaled: null argument");
    EFGP_REQUIRE(nbatch >= 1, "efgp_toeplitz_apply_scaled: nbatch must be >= 1");
    EFGP_REQUIRE(x != y, "efgp_toeplitz_apply_scaled: x and y must not alias");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, (hipStream_t)stream_);
    if (const int rc_ops = ensure_deferred_spectra(op, stream)) return rc_ops;
    const CgGrid q = cg_grid(op);
    if (toeplitz_apply_fused_eligible(q.g))
        return toeplitz_apply_fused_launch(q.g, q.tw[0], q.vhat, (const double2*)pre, (const double2*)post, x, x_is_real, (double2*)y, nbatch,
                                           stream);
    const int64_t max_rows = std::max<int64_t>(1, std::min<int64_t>(kMaxGridRows, (int64_t)(256ll << 20) / (op->g.Ftot * (int64_t)sizeof(double2))));
    for (int64_t r0 = 0; r0 < nbatch; r0 += max_rows) {
        const int rows = (int)std::min<int64_t>(max_rows, nbatch - r0);
        double2* pad = (double2*)scratch(op->ctx, SLOT_TOEP_PAD, (size_t)rows * (size_t)op->g.Ftot * sizeof(double2));
        if (!pad) return EFGP_ENOMEM;
        if (x_is_real)
            hipLaunchKernelGGL(pad_pre_kernel<true>, grid_for(op->g.Ftot, rows, kVecThreads), dim3(kVecThreads), 0, stream, op->g,
                               (const void*)((const double*)x + r0 * op->g.M), (const double2*)pre, pad);
        else
            hipLaunchKernelGGL(pad_pre_kernel<false>, grid_for(op->g.Ftot, rows, kVecThreads), dim3(kVecThreads), 0, stream, op->g,
                               (const void*)((const double2*)x + r0 * op->g.M), (const double2*)pre, pad);
        EFGP_HIP_CHECK(hipGetLastError());
        int rc = circulant(op, pad, rows, stream);
        if (rc != EFGP_OK) return rc;
        hipLaunchKernelGGL(crop_post_kernel, grid_for(op->g.M, rows, kVecThreads), dim3(kVecThreads), 0, stream, op->g,
                           (const double2*)pad, (const double2*)post, (double2*)y + r0 * op->g.M);
        EFGP_HIP_CHECK(hipGetLastError());
    }
    return EFGP_OK;
}

int efgp_internal_apply_scaled(efgp_toeplitz_s* op, const void* x, int x_is_real, int nbatch, const void* pre, int pre_stride,
                               const void* post, void* y, hipStream_t stream) {
    if (pre == nullptr || pre_stride == 1) return efgp_toeplitz_apply_scaled(op, x, x_is_real, nbatch, pre, post, y, stream);
    EFGP_REQUIRE(op && x && y && nbatch >= 1 && x != y && pre_stride >= 1, "efgp_internal_apply_scaled: bad argument");
    DeviceGuard guard(op->device, stream);
    if (const int rc_ops = ensure_deferred_spectra(op, stream)) return rc_ops;
    const CgGrid q = cg_grid(op);
    if (!toeplitz_apply_fused_eligible(q.g)) return EFGP_EUNSUPPORTED;
    return toeplitz_apply_fused_launch(q.g, q.tw[0], q.vhat, (const double2*)pre, (const double2*)post, x, x_is_real, (double2*)y, nbatch, stream,
                                       pre_stride);
}

int efgp_internal_cg_single_launch(efgp_toeplitz_s* op, const void* ws, double sigmasq, int variant, const double* diag,
                                   const double* diag_scale, const void* b, int b_times_ws, void* x, int zero_x0, int nbatch, double tol,
                                   int max_iter, int early_stop, int batched_semantics, int* row_iters_dev, hipStream_t stream,
                                   int hermitian, const void* x0) {
    EFGP_REQUIRE(op && ws && b && x && row_iters_dev && nbatch >= 1, "efgp_internal_cg_single_launch: bad argument");
    EFGP_REQUIRE(batched_semantics || nbatch == 1, "efgp_internal_cg_single_launch: single-system semantics need nbatch == 1");
    if (!persistent_usable(op)) return EFGP_EUNSUPPORTED;
    DeviceGuard guard(op->device, stream);
    CgSolve s = make_solve(op, ws, sigmasq, variant, diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics);
    s.diag_scale = diag ? nullptr : diag_scale;
    s.b_times_ws = b_times_ws;
    s.zero_x0 = zero_x0;
    s.hermitian = hermitian;
    s.x0 = (const double2*)x0;
    return enqueue_persistent(op, s, row_iters_dev, stream);
}

// ---- the synchronous entries: read-back of the single-launch solves -------------------------------------------------------------
// per-row counts and the total of a finished solve.  The one place where the batched count becomes max + 1 unless capped (the
// terminating pass, cg.py:193-199,243; cg.py:152 counts a single system as it is)
static void report_counts(const int* its, const CgSolve& s, int* iters_out, int* row_iters_out) {
    int mx = 0;
    for (int i = 0; i < s.nbatch; ++i) {
        mx = std::max(mx, its[i]);
        if (row_iters_out) row_iters_out[i] = its[i];
    }
    if (iters_out) *iters_out = (s.batched && mx < s.max_iter) ? mx + 1 : mx;
}

// Ends a single-launch solve on the host: d_iters (and the cooperative solve's status word, d_status, where there is one) come back
// through the context's pinned buffer, the stream is waited for and the counts are reported.  With a status word, *its keeps the
// counts and *any_dead says whether a grid barrier died (the word is set, or a row reports a negative count).
static int read_back_counts(DeviceCtx* ctx, const CgSolve& s, const int* d_iters, const int* d_status, hipStream_t stream, int* iters_out,
                            int* row_iters_out, std::vector<int>* its = nullptr, bool* any_dead = nullptr) {
    int* host = pinned_host(ctx, (size_t)s.nbatch * sizeof(int) + 128);
    if (!host) return EFGP_ENOMEM;
    const int* hit = host + 16;
    if (d_status) EFGP_HIP_CHECK(hipMemcpyAsync(host, d_status, sizeof(int), hipMemcpyDeviceToHost, stream));
    EFGP_HIP_CHECK(hipMemcpyAsync(host + 16, d_iters, (size_t)s.nbatch * sizeof(int), hipMemcpyDeviceToHost, stream));
    EFGP_HIP_CHECK(stream_wait(stream));
    if (d_status) {
        bool dead = host[0] != 0;
        for (int i = 0; i < s.nbatch; ++i) dead = dead || hit[i] < 0;
        *any_dead = dead;
        its->assign(hit, hit + s.nbatch);
    }
    report_counts(hit, s, iters_out, row_iters_out);
    return EFGP_OK;
}

// a grid barrier ran out of polls (the workgroups were not co-resident): the systems it hit still hold x0 in x (a solution is
// written only by a system that finished) and go through the multi-launch path one by one
static int resolve_dead_rows(efgp_toeplitz_s* op, const CgSolve& s, std::vector<int>& its, hipStream_t stream) {
    std::fprintf(stderr, "[efgp_hip] cooperative CG: grid barrier timed out, falling back to the multi-launch iteration\n");
    for (int i = 0; i < s.nbatch; ++i) {
        if (its[i] >= 0) continue;
        CgSolve one = s;
        one.b = s.b + (int64_t)i * op->g.M;
        one.x = s.x + (int64_t)i * op->g.M;
        one.nbatch = 1;
        const int rc = solve_multi_launch(op, one, nullptr, &its[i], stream);
        if (rc != EFGP_OK) return rc;
    }
    return EFGP_OK;
}

// efgp_cg_solve / efgp_cg_solve_hermitian: the persistent kernel, the cooperative launches or the multi-launch solver, whichever
// the grid allows first, and the counts on the host
static int cg_solve_sync(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                         const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop,
                         int batched_semantics, int* iters_out, int* row_iters_out, void* stream_, int hermitian) {
    EFGP_REQUIRE(op && ws && b && x, "efgp_cg_solve: null argument");
    EFGP_REQUIRE(nbatch >= 1, "efgp_cg_solve: nbatch must be >= 1");
    EFGP_REQUIRE(variant == 0 || variant == 1, "efgp_cg_solve: variant must be 0 or 1");
    EFGP_REQUIRE(batched_semantics || nbatch == 1, "efgp_cg_solve: single-system semantics need nbatch == 1");
    EFGP_REQUIRE(sigmasq > 0.0 || variant == 0, "efgp_cg_solve: sigmasq must be positive for A_var");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, stream);
    DeviceCtx* ctx = op->ctx;
    // Only the multi-launch 3-D iteration honours the Hermitian promise here: the persistent kernel is given neither `hermitian`
    // nor a use for the 48 x 48 operands, and the cooperative kernel runs with hermitian = 0 (the asynchronous entries pass the
    // promise on).  Which kernel runs is behaviour: kept as it is.
    CgSolve s = make_solve(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics);
    CgSolve promised = s;
    promised.hermitian = hermitian;

    // small circulant grids: the whole solve in one persistent kernel, one workgroup per system
    if (persistent_usable(op)) {
        int* d_iters = (int*)scratch(ctx, SLOT_CG_SCALARS, (size_t)nbatch * sizeof(int) + 64);
        if (!d_iters) return EFGP_ENOMEM;
        const int rc = enqueue_persistent(op, s, d_iters, stream);
        if (rc != EFGP_OK) return rc;
        return read_back_counts(ctx, s, d_iters, nullptr, stream, iters_out, row_iters_out);
    }
    // 2-D grids of 128..512 per dimension: the whole solve in cooperative launches (coop_enqueue)
    if (coop_usable(op)) {
        int* d_iters = (int*)scratch(ctx, SLOT_CG_SCALARS, (size_t)nbatch * sizeof(int) + 64);
        if (!d_iters) return EFGP_ENOMEM;
        CoopInfo ci;
        int rc = coop_enqueue(op, s, d_iters, stream, &ci, /*nan_on_dead: this entry re-solves dead systems from x0*/ 0);
        if (rc != EFGP_OK && rc != EFGP_EUNSUPPORTED) return rc;
        if (rc == EFGP_OK) {
            std::vector<int> its;
            bool any_dead = false;
            rc = read_back_counts(ctx, s, d_iters, ci.d_status, stream, iters_out, row_iters_out, &its, &any_dead);
            if (rc == EFGP_OK && ci.dbg == 2) rc = coop_print_stamps(ci, its[0]);
            if (rc != EFGP_OK || !any_dead) return rc;
            rc = resolve_dead_rows(op, s, its, stream);
            if (rc == EFGP_OK) report_counts(its.data(), s, iters_out, row_iters_out);
            return rc;
        }
    }
    return solve_multi_launch(op, promised, iters_out, row_iters_out, stream);
}

int efgp_cg_solve(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                  const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop,
                  int batched_semantics, int* iters_out, int* row_iters_out, void* stream_) {
    return cg_solve_sync(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics, iters_out,
                         row_iters_out, stream_, 0);
}

int efgp_cg_solve_hermitian(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                            const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop,
                            int batched_semantics, int* iters_out, int* row_iters_out, void* stream_) {
    return cg_solve_sync(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics, iters_out,
                         row_iters_out, stream_, 1);
}

// the asynchronous entries: the persistent kernel, else the cooperative launches -- neither needs the host (a row whose grid barrier
// died -- workgroups not co-resident -- reports -3 iterations and keeps x0; the synchronous entry retries those through the
// multi-launch path)
static int cg_solve_async(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                          const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop,
                          int batched_semantics, int* row_iters_dev, void* stream_, int hermitian, int zero_x0) {
    EFGP_REQUIRE(op && ws && b && x && row_iters_dev, "efgp_cg_solve_async: null argument");
    EFGP_REQUIRE(nbatch >= 1, "efgp_cg_solve_async: nbatch must be >= 1");
    EFGP_REQUIRE(variant == 0 || variant == 1, "efgp_cg_solve_async: variant must be 0 or 1");
    EFGP_REQUIRE(batched_semantics || nbatch == 1, "efgp_cg_solve_async: single-system semantics need nbatch == 1");
    EFGP_REQUIRE(sigmasq > 0.0 || variant == 0, "efgp_cg_solve_async: sigmasq must be positive for A_var");
    if (!persistent_usable(op) && !coop_usable(op)) {
        set_error("efgp_cg_solve_async: grid does not fit the persistent kernel");
        return EFGP_EUNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, stream);
    CgSolve s = make_solve(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics);
    s.hermitian = hermitian;
    s.zero_x0 = zero_x0;
    if (persistent_usable(op)) return enqueue_persistent(op, s, row_iters_dev, stream);
    return coop_enqueue(op, s, row_iters_dev, stream, nullptr, /*nan_on_dead*/ 1);
}

int efgp_cg_solve_async(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                        const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop,
                        int batched_semantics, int* row_iters_dev, void* stream_) {
    return cg_solve_async(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics,
                          row_iters_dev, stream_, 0, 0);
}

int efgp_cg_solve_hermitian_async(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                                  const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop,
                                  int batched_semantics, int* row_iters_dev, void* stream_) {
    return cg_solve_async(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics,
                          row_iters_dev, stream_, 1, 0);
}

int efgp_cg_solve_from_zero_async(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const double* precond_diag,
                                  const void* b, void* x, int nbatch, double tol, int max_iter, int early_stop, int batched_semantics,
                                  int hermitian, int* row_iters_dev, void* stream_) {
    return cg_solve_async(op, ws, sigmasq, variant, precond_diag, b, x, nbatch, tol, max_iter, early_stop, batched_semantics,
                          row_iters_dev, stream_, hermitian ? 1 : 0, 1);
}

int efgp_lanczos(efgp_toeplitz_t* op, const void* ws, double sigmasq, int variant, const void* z, int nprobes, int steps,
                 double* alpha_dev, double* beta_dev, double* norm2_dev, int* steps_taken_dev, void* stream_) {
    EFGP_REQUIRE(op && ws && z && alpha_dev && beta_dev && steps_taken_dev, "efgp_lanczos: null argument");
    EFGP_REQUIRE(nprobes >= 1 && steps >= 1, "efgp_lanczos: nprobes and steps must be >= 1");
    EFGP_REQUIRE(variant == 0 || variant == 1, "efgp_lanczos: variant must be 0 or 1");
    EFGP_REQUIRE(sigmasq > 0.0 || variant == 0, "efgp_lanczos: sigmasq must be positive for A_var");
    if (!persistent_usable(op)) {
        set_error("efgp_lanczos: grid does not fit the persistent kernel");
        return EFGP_EUNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, stream);
    const LanczosOut lz{steps, alpha_dev, beta_dev, norm2_dev};
    // `steps` recurrences from z with a zero start, no stopping test, no solution written
    CgSolve s = make_solve(op, ws, sigmasq, variant, nullptr, z, nullptr, nprobes, 0.0, steps, 0, 1);
    s.zero_x0 = 1;
    return enqueue_persistent(op, s, steps_taken_dev, stream, &lz);
}

// The mean system of a fit: variant 0, one system, single-system stopping rule; the kernel forms the right-hand side ws .* fy, the
// Jacobi diagonal (*diag_scale_dev) |ws|^2 + sigmasq and the zero start itself.  Hermitian: F*y of a real y, Toeplitz vector of
// real weights.
static CgSolve mean_solve(efgp_toeplitz_s* op, const void* ws, double sigmasq, const double* diag_scale_dev, const void* fy, void* x,
                          double tol, int max_iter, int early_stop) {
    CgSolve s = make_solve(op, ws, sigmasq, 0, nullptr, fy, x, 1, tol, max_iter, early_stop, 0);
    s.diag_scale = diag_scale_dev;
    s.b_times_ws = 1;
    s.zero_x0 = 1;
    s.hermitian = 1;
    return s;
}

int efgp_cg_solve_mean_async(efgp_toeplitz_t* op, const void* ws, double sigmasq, const double* diag_scale_dev, const void* fy,
                             void* x, double tol, int max_iter, int early_stop, int* iters_dev, void* stream_) {
    EFGP_REQUIRE(op && ws && fy && x && iters_dev, "efgp_cg_solve_mean_async: null argument");
    if (!persistent_usable(op) && !coop_usable(op)) {
        set_error("efgp_cg_solve_mean_async: grid does not fit the persistent kernel");
        return EFGP_EUNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, stream);
    const CgSolve s = mean_solve(op, ws, sigmasq, diag_scale_dev, fy, x, tol, max_iter, early_stop);
    if (persistent_usable(op)) return enqueue_persistent(op, s, iters_dev, stream);
    // 2-D 128^2..512^2: no prepare launch, no fill, no initial operator application; a dead grid barrier leaves iters = -3 and NaN
    return coop_enqueue(op, s, iters_dev, stream, nullptr, /*nan_on_dead*/ 1);
}

int efgp_cg_solve_mean_fused(efgp_toeplitz_t* op, int kind, double nu, double lengthscale, double c0, double h, int mtot, void* ws_out,
                             double sigmasq, const double* diag_scale_dev, const void* fy, void* x, double tol, int max_iter, int early_stop,
                             int* iters_dev, void* stream_) {
    EFGP_REQUIRE(op && ws_out && fy && x && iters_dev, "efgp_cg_solve_mean_fused: null argument");
    EFGP_REQUIRE(kind == 0 || kind == 1, "efgp_cg_solve_mean_fused: kernel kind %d not built in", kind);
    // only an operator whose 48 x 48 spectrum is still to be made (efgp_toeplitz_create_ex, deferred) on a block of mtot^2 modes
    if (!op->pair_pending || op->vhat48_ready || op->h48.vhat == nullptr || !persistent_usable(op) || op->g.d != 2 || op->g.n[0] != mtot ||
        op->g.n[1] != mtot || std::getenv("EFGP_NO_CG_FUSED_MEAN") != nullptr) {
        set_error("efgp_cg_solve_mean_fused: the operator is not a deferred 48 x 48 Hermitian one of this grid");
        return EFGP_EUNSUPPORTED;
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(op->device, stream);
    const MeanFusedOperands fuse{kind, mtot, nu, lengthscale, c0, h, (double2*)ws_out, op->v_ref, (int)op->Ls[0], (int)op->Ls[1], op->vhat48};
    const int rc = enqueue_persistent(op, mean_solve(op, ws_out, sigmasq, diag_scale_dev, fy, x, tol, max_iter, early_stop), iters_dev, stream,
                                      nullptr, &fuse);
    if (rc == EFGP_OK) op->vhat48_ready = true;        // the 64 x 64 spectrum stays deferred: nothing on the fit path reads it
    return rc;
}

int efgp_vdot_real(int device, const void* a, int a_is_complex, const void* b, int b_is_complex, int64_t count,
                   double* out_host, void* stream_) {
    EFGP_REQUIRE(out_host, "efgp_vdot_real: null out");
    EFGP_REQUIRE(count >= 0, "efgp_vdot_real: negative count");
    *out_host = 0.0;
    if (count == 0) return EFGP_OK;
    EFGP_REQUIRE(a && b, "efgp_vdot_real: null input");
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(device, (hipStream_t)stream_);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((count + kVecThreads - 1) / kVecThreads, 2048));
    double* partial = (double*)scratch(ctx, SLOT_MISC, (size_t)blocks * sizeof(double));
    double* host = (double*)pinned_host(ctx, (size_t)blocks * sizeof(double));
    if (!partial || !host) return EFGP_ENOMEM;
    const double* pa = (const double*)a;
    const double* pb = (const double*)b;
    if (a_is_complex && b_is_complex)
        hipLaunchKernelGGL((vdot_real_kernel<true, true>), dim3(blocks), dim3(kVecThreads), 0, stream, pa, pb, count, partial);
    else if (a_is_complex)
        hipLaunchKernelGGL((vdot_real_kernel<true, false>), dim3(blocks), dim3(kVecThreads), 0, stream, pa, pb, count, partial);
    else if (b_is_complex)
        hipLaunchKernelGGL((vdot_real_kernel<false, true>), dim3(blocks), dim3(kVecThreads), 0, stream, pa, pb, count, partial);
    else
        hipLaunchKernelGGL((vdot_real_kernel<false, false>), dim3(blocks), dim3(kVecThreads), 0, stream, pa, pb, count, partial);
    EFGP_HIP_CHECK(hipGetLastError());
    EFGP_HIP_CHECK(hipMemcpyAsync(host, partial, (size_t)blocks * sizeof(double), hipMemcpyDeviceToHost, stream));
    EFGP_HIP_CHECK(stream_wait(stream));
    double acc = 0.0;
    for (int i = 0; i < blocks; ++i) acc += host[i];
    *out_host = acc;
    return EFGP_OK;
}

}  // extern "C"
