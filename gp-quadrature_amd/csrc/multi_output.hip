// M-scale tail of the JOINT hyper-parameter gradient of a multi-output model (EFGPNDMulti, efgpnd_multi.py): nrows outputs observed
// at the same points under one kernel and one noise level.
//   efgp_gradient_assemble_multi   the inner products of efgp_gradient_assemble (gradient_ops.hip) for nrows rows of (fy, tg, beta)
//                                  and ONE set of trace probes, summed to the gradient of the sum of the negative log marginals
// What depends on the data is a row: term2, y.z, |z|^2, |alpha|^2, y.alpha.  What does not (term1: the trace estimates) is computed
// once and counts nrows times.  Rows arrive scaled by exact powers of two (row b holds y_b / row_scale[b], so do fy, tg, beta and
// yy[b] = |y_b|^2 / row_scale[b]^2); every per-row sum is scaled back by two exact multiplications before rows are added, so the
// result is bitwise what unscaled rows give.
//
// Shape: a reduction over nrows * M entries behind a launch -- bound by launch latency, not by bandwidth -- so: one launch when
// nrows * M <= 4096, two otherwise; no atomics; rows and partial sums added in a fixed order (bitwise repeatable).
//   partial  job j < nrows is row j, job nrows is the trace estimate; workgroup (x, y) sums the entries x, x + gridDim.x, .. of the
//            jobs y, y + gridDim.y, ..: the jobs are strided over gridDim.y in the kernel, so no row count rides there unchunked
//   finish   one workgroup: thread t takes the rows t, t + THREADS, .. in order, adds their partial sums in order, scales back,
//            writes rows_out and accumulates; a shuffle + LDS tree adds the threads; thread 0 does the scalar algebra
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.hpp"

namespace efgp {

namespace gradm {

constexpr int kMaxH = 4;                 // kernel hyper-parameters, as efgp_gradient_assemble
constexpr int kMaxK = 4;                 // of which need a trace estimate
constexpr int kSlots = 8;                // sums per job -- a row: term2[0..3], y.z, |z|^2; the trace job: trace[0..3], noise
constexpr int kThreads = 256;
constexpr int kSmallThreads = 1024;
constexpr int kMaxBlocks = 64;           // workgroups along M per job
constexpr int64_t kMaxPartialSums = int64_t(1) << 22;       // (jobs * workgroups along M): 256 MB of partial sums at most

struct Args {
    int64_t M;
    int nrows, T, H, K;
    int trace_idx[kMaxK];
    const double2* fy;         // (nrows, M)
    const double2* tg;         // (nrows, M)
    const double2* beta;       // (nrows, M)
    const double2* ws;         // (M)
    const double2* dprime;     // (M, H)
    const double2* fz;         // (T, M)
    const double2* beta_k;     // (K*T, M)
    const double* v;           // (T, M)
    const double2* beta_n;     // (T, M)
    double sig;
    double* partial;           // [nrows + 1][nbx][kSlots]
};

// The kSlots sums of job `job` over the entries xb * THREADS + threadIdx.x, stride nbx * THREADS -> partial[job][xb][:]
template <int THREADS>
__device__ __forceinline__ void job_body(const Args& a, int64_t job, int xb, int nbx) {
    double acc[kSlots];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) acc[q] = 0.0;
    if (job < a.nrows) {
        const double2* fyr = a.fy + job * a.M;
        const double2* tgr = a.tg + job * a.M;
        const double2* ber = a.beta + job * a.M;
        for (int64_t m = (int64_t)xb * THREADS + threadIdx.x; m < a.M; m += (int64_t)nbx * THREADS) {
            const double2 fy = fyr[m], tg = tgr[m], w = a.ws[m], be = ber[m];
            const double2 g = make_double2(w.x * be.x - w.y * be.y, w.x * be.y + w.y * be.x);
            const double far = (fy.x - tg.x) / a.sig, fai = (fy.y - tg.y) / a.sig;
            const double fa2 = far * far + fai * fai;
#pragma unroll
            for (int i = 0; i < kMaxH; ++i)
                if (i < a.H) acc[i] += a.dprime[m * a.H + i].x * fa2;
            acc[kMaxH] += fy.x * g.x + fy.y * g.y;
            acc[kMaxH + 1] += g.x * tg.x + g.y * tg.y;
        }
    } else {
        for (int64_t m = (int64_t)xb * THREADS + threadIdx.x; m < a.M; m += (int64_t)nbx * THREADS) {
            const double2 w = a.ws[m];
            double2 dp[kMaxH];
#pragma unroll
            for (int i = 0; i < kMaxH; ++i) dp[i] = i < a.H ? a.dprime[m * a.H + i] : make_double2(0.0, 0.0);
            for (int t = 0; t < a.T; ++t) {
                const int64_t o = (int64_t)t * a.M + m;
                if (a.K > 0) {
                    const double2 z = a.fz[o];
#pragma unroll
                    for (int s = 0; s < kMaxK; ++s) {
                        if (s < a.K) {
                            double2 d = make_double2(0.0, 0.0);
#pragma unroll
                            for (int i = 0; i < kMaxH; ++i)
                                if (i == a.trace_idx[s]) d = dp[i];
                            const double2 b = a.beta_k[((int64_t)s * a.T + t) * a.M + m];
                            const double dr = (d.x * z.x - d.y * z.y) - (w.x * b.x - w.y * b.y);
                            const double di = (d.x * z.y + d.y * z.x) - (w.x * b.y + w.y * b.x);
                            acc[s] += z.x * dr + z.y * di;
                        }
                    }
                }
                acc[kMaxK] += a.v[o] * a.beta_n[o].x;
            }
        }
    }
    __shared__ double red[THREADS / 64][kSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) v += red[w][threadIdx.x];
        a.partial[(job * nbx + xb) * kSlots + threadIdx.x] = v;
    }
    __syncthreads();                       // `red` is free for the workgroup's next job
}

struct FinishArgs {
    int nrows, nbx, T, H, K, variance_idx;
    int trace_idx[kMaxK];
    const double* partial;
    const double* yy;          // (nrows) |y_b|^2 of the rows as stored (scaled)
    const double* row_scale;   // (nrows) exact powers of two
    double sig, n_obs, variance;
    double* out;               // grad[H+1] | term1[H+1] | term2[H+1] | y.alpha, of the joint objective
    double* rows_out;          // (nrows, 4): y.z, |z|^2, y.alpha, |alpha|^2
};

constexpr int kTot = kMaxH + 2;          // what the rows add up to: term2[0..3], |alpha|^2, y.alpha

template <int THREADS>
__device__ __forceinline__ void finish_body(const FinishArgs& a) {
    __shared__ double tot[THREADS / 64][kSlots];
    __shared__ double trace[kSlots];
    double acc[kTot];
#pragma unroll
    for (int q = 0; q < kTot; ++q) acc[q] = 0.0;
    for (int64_t b = threadIdx.x; b < a.nrows; b += THREADS) {
        double s[kTot];
#pragma unroll
        for (int q = 0; q < kTot; ++q) {
            double v = 0.0;
            for (int xb = 0; xb < a.nbx; ++xb) v += a.partial[(b * a.nbx + xb) * kSlots + q];
            s[q] = v;
        }
        // back to the units of y_b: two multiplications by a power of two, each exact (row_scale^2 itself may overflow)
        const double sc = a.row_scale[b];
        const double y_z = s[kMaxH] * sc * sc, z_z = s[kMaxH + 1] * sc * sc, yy = a.yy[b] * sc * sc;
        const double a_norm = (yy - 2.0 * y_z + z_z) / (a.sig * a.sig);
        const double y_alpha = (yy - y_z) / a.sig;
        a.rows_out[4 * b] = y_z;
        a.rows_out[4 * b + 1] = z_z;
        a.rows_out[4 * b + 2] = y_alpha;
        a.rows_out[4 * b + 3] = a_norm;
#pragma unroll
        for (int i = 0; i < kMaxH; ++i)
            if (i < a.H) acc[i] += s[i] * sc * sc;
        acc[kMaxH] += a_norm;
        acc[kMaxH + 1] += y_alpha;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kTot; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) tot[wave][q] = v;
    }
    if (threadIdx.x < kSlots) {
        double v = 0.0;
        for (int xb = 0; xb < a.nbx; ++xb) v += a.partial[((int64_t)a.nrows * a.nbx + xb) * kSlots + threadIdx.x];
        trace[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum[kTot];
    for (int q = 0; q < kTot; ++q) {
        double v = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) v += tot[w][q];
        sum[q] = v;
    }
    const int nh = a.H + 1;
    const double rows = (double)a.nrows;
    double* grad = a.out;
    double* term1 = a.out + nh;
    double* term2 = a.out + 2 * nh;
    const double a_norm = sum[kMaxH], y_alpha = sum[kMaxH + 1];
    for (int i = 0; i < a.H; ++i) {
        term2[i] = sum[i];
        term1[i] = 0.0;
    }
    term2[a.H] = a_norm;
    for (int s = 0; s < a.K; ++s) term1[a.trace_idx[s]] = rows * (trace[s] / a.sig / (double)a.T);
    const double t1_noise = a.n_obs / a.sig - trace[kMaxK] / a.sig / (double)a.T;      // of ONE output
    term1[a.H] = rows * t1_noise;
    if (a.variance_idx >= 0) {
        term2[a.variance_idx] = (y_alpha - a.sig * a_norm) / a.variance;
        term1[a.variance_idx] = rows * ((a.n_obs - a.sig * t1_noise) / a.variance);
    }
    for (int i = 0; i < nh; ++i) grad[i] = 0.5 * (term1[i] - term2[i]);
    a.out[3 * nh] = y_alpha;
}

__global__ __launch_bounds__(kThreads) void partial_multi_kernel(Args a) {
    for (int64_t job = blockIdx.y; job <= a.nrows; job += gridDim.y) job_body<kThreads>(a, job, (int)blockIdx.x, (int)gridDim.x);
}
__global__ __launch_bounds__(kThreads) void finish_multi_kernel(FinishArgs a) { finish_body<kThreads>(a); }
// nrows * M <= 4096: one workgroup goes through the jobs and finishes -- a dependent launch costs more than these sums
__global__ __launch_bounds__(kSmallThreads) void assemble_multi_small_kernel(Args a, FinishArgs f) {
    for (int64_t job = 0; job <= a.nrows; ++job) job_body<kSmallThreads>(a, job, 0, 1);
    __threadfence_block();
    __syncthreads();
    finish_body<kSmallThreads>(f);
}

}  // namespace gradm
}  // namespace efgp

using namespace efgp;

extern "C" {

int efgp_gradient_assemble_multi(int device, int64_t nmodes, int nrows, int nprobes, int n_kernel_hypers, int variance_idx, int n_trace,
                                 const int* trace_idx, const void* fy, const void* tg, const void* ws, const void* beta,
                                 const void* dprime, const void* fz, const double* v, const void* beta_all, double sigmasq, double n_obs,
                                 const double* yy, const double* row_scale, double variance, double* out, double* rows_out,
                                 void* stream_) {
    using namespace gradm;
    EFGP_REQUIRE(fy && tg && ws && beta && out && rows_out && yy && row_scale && nmodes >= 1,
                 "efgp_gradient_assemble_multi: null / empty argument");
    EFGP_REQUIRE(nrows >= 1, "efgp_gradient_assemble_multi: nrows must be at least 1 (got %d)", nrows);
    EFGP_REQUIRE(n_kernel_hypers >= 0 && n_kernel_hypers <= kMaxH, "efgp_gradient_assemble_multi: %d kernel hyper-parameters (at most %d)",
                 n_kernel_hypers, kMaxH);
    EFGP_REQUIRE(n_trace >= 0 && n_trace <= kMaxK && n_trace <= n_kernel_hypers, "efgp_gradient_assemble_multi: bad n_trace %d", n_trace);
    EFGP_REQUIRE(n_kernel_hypers == 0 || dprime, "efgp_gradient_assemble_multi: dprime is null");
    // nprobes = 0: the data terms only (a fit's log marginal) -- no trace estimate, term1's estimated entries come out NaN
    EFGP_REQUIRE(nprobes >= 0 && (nprobes == 0 || (v && beta_all)), "efgp_gradient_assemble_multi: probes given without their solves");
    EFGP_REQUIRE(n_trace == 0 || nprobes == 0 || (fz && trace_idx), "efgp_gradient_assemble_multi: trace probes missing");
    EFGP_REQUIRE(n_trace == 0 || trace_idx, "efgp_gradient_assemble_multi: trace_idx is null");
    EFGP_REQUIRE(variance_idx >= -1 && variance_idx < n_kernel_hypers, "efgp_gradient_assemble_multi: bad variance_idx %d", variance_idx);
    EFGP_REQUIRE(sigmasq > 0.0 && (variance_idx < 0 || variance != 0.0),
                 "efgp_gradient_assemble_multi: sigmasq / variance must be positive");
    for (int s = 0; s < n_trace; ++s)
        EFGP_REQUIRE(trace_idx[s] >= 0 && trace_idx[s] < n_kernel_hypers && trace_idx[s] != variance_idx,
                     "efgp_gradient_assemble_multi: bad trace_idx[%d] = %d", s, trace_idx[s]);
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t jobs = (int64_t)nrows + 1;
    const bool small = (int64_t)nrows * nmodes <= 4096 && std::getenv("EFGP_ASSEMBLE_TWO_LAUNCHES") == nullptr;
    int nbx = 1;
    if (!small) {
        const int64_t want = std::min<int64_t>(kMaxBlocks, (nmodes + kThreads - 1) / kThreads);
        nbx = (int)std::max<int64_t>(1, std::min<int64_t>(want, kMaxPartialSums / jobs));
    }
    double* partial = (double*)scratch(ctx, SLOT_MISC, (size_t)jobs * nbx * kSlots * sizeof(double));
    if (!partial) return EFGP_ENOMEM;
    Args a;
    a.M = nmodes;
    a.nrows = nrows;
    a.T = nprobes;
    a.H = n_kernel_hypers;
    a.K = n_trace;
    for (int s = 0; s < kMaxK; ++s) a.trace_idx[s] = s < n_trace ? trace_idx[s] : -1;
    a.fy = (const double2*)fy;
    a.tg = (const double2*)tg;
    a.beta = (const double2*)beta;
    a.ws = (const double2*)ws;
    a.dprime = (const double2*)dprime;
    a.fz = (const double2*)fz;
    a.beta_k = (const double2*)beta_all;
    a.v = v;
    a.beta_n = beta_all ? (const double2*)beta_all + (int64_t)n_trace * nprobes * nmodes : nullptr;
    a.sig = sigmasq;
    a.partial = partial;
    FinishArgs f;
    f.nrows = nrows;
    f.nbx = nbx;
    f.T = nprobes;
    f.H = n_kernel_hypers;
    f.K = n_trace;
    f.variance_idx = variance_idx;
    for (int s = 0; s < kMaxK; ++s) f.trace_idx[s] = a.trace_idx[s];
    f.partial = partial;
    f.yy = yy;
    f.row_scale = row_scale;
    f.sig = sigmasq;
    f.n_obs = n_obs;
    f.variance = variance;
    f.out = out;
    f.rows_out = rows_out;
    if (small) {
        hipLaunchKernelGGL(assemble_multi_small_kernel, dim3(1), dim3(kSmallThreads), 0, stream, a, f);
    } else {
        const unsigned gy = (unsigned)std::min<int64_t>(jobs, kMaxGridRows);      // further jobs: strided inside the kernel
        hipLaunchKernelGGL(partial_multi_kernel, dim3((unsigned)nbx, gy), dim3(kThreads), 0, stream, a);
        EFGP_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(finish_multi_kernel, dim3(1), dim3(kThreads), 0, stream, f);
    }
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

}  // extern "C"
