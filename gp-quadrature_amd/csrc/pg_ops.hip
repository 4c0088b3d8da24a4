// N-scale and M-scale passes of the Polya-Gamma (PG) GP estimators behind the C ABI
// (reference: polyagamma_classification/pg_classifier.py):
//   efgp_pg_estep_update         one pass over the N points after the E-step solves, Bernoulli likelihood (:552-569, :252-257,
//                                :129-138)
//   efgp_pg_nb_estep_update      the same pass for the negative-binomial likelihood, b = y + r and the mean-count error
//                                (:142-171, :194-201)
//   efgp_pg_nb_total_count_grad  d/dr of the negative-binomial ELBO by Gauss-Hermite quadrature (:204-249)
//   efgp_pg_weight_rows          omega .* z for the M-step's R = F*(omega z) right-hand rows (:616)
//   efgp_pg_mstep_terms          term1 / term2 / gradient of the M-step in feature space (:616-623)
// Every reduction is two launches: per-workgroup partials over a grid whose size depends only on the problem size, then one
// workgroup that adds them in a fixed order -- a seeded fit is bit-reproducible run to run (no floating-point atomics).
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "nufft_dev.hpp"

namespace efgp {

constexpr int kPgThreads = 256;          // four wave64 per workgroup
constexpr int kPgMaxBlocks = 1024;
constexpr int kPgMaxHypers = 4;
constexpr int kPgMaxNodes = 128;         // Gauss-Hermite nodes of the total-count gradient

template <typename T>
__device__ __forceinline__ T pg_wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// A NaN stays a NaN, as in torch's clamp_min / clamp(min=) / max(), which the reference uses (fmax would return the other
// operand): a non-finite solve shows in delta, in the residual and in the metric instead of passing for a converged one.
__device__ __forceinline__ double pg_clamp_min(double x, double lo) { return x < lo ? lo : x; }

__device__ __forceinline__ double pg_max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double pg_wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = pg_max_nan(v, __shfl_down(v, off, 64));
    return v;
}

// The likelihood-specific part of the E-step pass: the PG shape b of a point and its term of the training metric, with the
// metric's accumulator type (Acc) and the type the finish kernel writes (Out).
struct PgBernoulli {
    using Acc = unsigned long long;
    using Out = int64_t;
    const double* pg_b;                  // N doubles, or null for b = 1
    __device__ double shape(int64_t n, double) const { return pg_b ? pg_b[n] : 1.0; }
    // hit of the logistic-Gaussian approximation (:129-138, :173-191)
    __device__ Acc metric(double m, double sd, double y) const {
        const double den = sqrt(__dadd_rn(1.0, __dmul_rn(M_PI / 8.0, pg_clamp_min(sd, 0.0))));
        const double p = 1.0 / (1.0 + exp(-__ddiv_rn(m, den)));
        return ((p > 0.5) == (y != 0.0)) ? 1ull : 0ull;
    }
};

struct PgNegativeBinomial {
    using Acc = double;
    using Out = double;
    double r;                            // total_count
    __device__ double shape(int64_t, double y) const { return __dadd_rn(y, r); }
    // |r exp(mean + max(sigma_diag, 0) / 2) - y|: the absolute error of the predicted mean count (:166-168, :194-201)
    __device__ Acc metric(double m, double sd, double y) const {
        return fabs(__dsub_rn(__dmul_rn(r, exp(__dadd_rn(m, __dmul_rn(0.5, pg_clamp_min(sd, 0.0))))), y));
    }
};

// One thread per point (grid-stride).  Explicit _rn operations keep the compiler from contracting the reference's separate
// multiplies and adds into FMAs, so the per-point values round as the reference's torch expressions do.
template <class L>
__global__ __launch_bounds__(kPgThreads) void pg_estep_update_kernel(int64_t N, int J, const double* __restrict__ S,
                                                                     const double* __restrict__ probes, unsigned long long seed, L lik,
                                                                     const double* __restrict__ y, double rho, double* __restrict__ delta,
                                                                     double* __restrict__ mean_out, double* __restrict__ sdiag_out,
                                                                     double* __restrict__ part_max, typename L::Acc* __restrict__ part_metric) {
    using Acc = typename L::Acc;
    __shared__ double smax[kPgThreads / 64];
    __shared__ Acc smet[kPgThreads / 64];
    double lmax = 0.0;
    Acc lmet = 0;
    const double one_m_rho = 1.0 - rho;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const double m = S[n];
        double sd = 0.0;
        if (J > 0) {
            double acc = 0.0;
            for (int j = 0; j < J; ++j) {
                const double z = probes ? probes[(int64_t)j * N + n] : efgp_rademacher(seed, j, n);
                acc = __dadd_rn(acc, __dmul_rn(z, S[(int64_t)(j + 1) * N + n]));
            }
            sd = __ddiv_rn(acc, (double)J);                               // (probes * Sz).mean(dim=0)
        }
        const double yn = y[n];
        const double b = lik.shape(n, yn);
        // c2 = clamp_min(sigma_diag + mean^2, 1e-12); Lambda = E[omega] of PG(b, c)  (:557-559, :252-257)
        const double c2 = pg_clamp_min(__dadd_rn(sd, __dmul_rn(m, m)), 1e-12);
        const double c = sqrt(c2);
        const double sc = pg_clamp_min(c, 1e-12);
        const double lam = c > 1e-8 ? __ddiv_rn(__dmul_rn(__dmul_rn(0.5, b), tanh(__dmul_rn(0.5, sc))), sc) : __dmul_rn(0.25, b);
        // damped update and clamp (:561-563)
        const double dn = pg_clamp_min(__dadd_rn(__dmul_rn(delta[n], one_m_rho), __dmul_rn(rho, lam)), 0.0);
        delta[n] = dn;
        mean_out[n] = m;
        sdiag_out[n] = sd;
        lmax = pg_max_nan(lmax, fabs(__dsub_rn(dn, lam)));
        lmet += lik.metric(m, sd, yn);
    }
    lmax = pg_wave_max(lmax);
    lmet = pg_wave_sum(lmet);
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = lmax;
        smet[threadIdx.x >> 6] = lmet;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bm = smax[0];
        Acc bc = smet[0];
        for (int w = 1; w < kPgThreads / 64; ++w) {
            bm = pg_max_nan(bm, smax[w]);
            bc += smet[w];
        }
        part_max[blockIdx.x] = bm;
        part_metric[blockIdx.x] = bc;
    }
}

template <class L>
__global__ __launch_bounds__(kPgThreads) void pg_estep_finish_kernel(int nparts, const double* __restrict__ part_max,
                                                                     const typename L::Acc* __restrict__ part_metric,
                                                                     double* __restrict__ resid_out, typename L::Out* __restrict__ metric_out) {
    using Acc = typename L::Acc;
    __shared__ double smax[kPgThreads / 64];
    __shared__ Acc smet[kPgThreads / 64];
    double m = 0.0;
    Acc c = 0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        m = pg_max_nan(m, part_max[i]);
        c += part_metric[i];
    }
    m = pg_wave_max(m);
    c = pg_wave_sum(c);
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = m;
        smet[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bm = smax[0];
        Acc bc = smet[0];
        for (int w = 1; w < kPgThreads / 64; ++w) {
            bm = pg_max_nan(bm, smax[w]);
            bc += smet[w];
        }
        if (resid_out) resid_out[0] = bm;
        if (metric_out) metric_out[0] = (typename L::Out)bc;
    }
}

// digamma(x) for x > 0, NaN for every other argument (zero, negative, NaN: the estimators refuse such targets, and the
// recurrence below would not end for x <= -2^53): the recurrence psi(x) = psi(x + 1) - 1/x up to x >= 10, then the asymptotic series
// psi(x) = ln x - 1/(2x) - sum_{k=1..7} B_2k / (2k x^2k); the first omitted term is 0.443 / x^16 <= 4.5e-17.
__device__ double pg_digamma(double x) {
    if (!(x > 0.0)) return __builtin_nan("");
    double acc = 0.0;
    while (x < 10.0) {
        acc -= 1.0 / x;
        x += 1.0;
    }
    const double z = 1.0 / (x * x);
    // B_2k / (2k) = 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
    const double tail =
        z * (1.0 / 12.0 - z * (1.0 / 120.0 - z * (1.0 / 252.0 - z * (1.0 / 240.0 - z * (1.0 / 132.0 - z * (691.0 / 32760.0 - z / 12.0))))));
    return acc + (log(x) - 0.5 / x - tail);
}

// Per point: digamma(y + r) - digamma(r) + sum_q w_q logsigmoid(-(mean + sqrt(max(sd, 0)) x_q)), the three terms in the
// reference's order (:229-249); logsigmoid(t) = min(t, 0) - log1p(exp(-|t|)).  Per-workgroup partial sums.
__global__ __launch_bounds__(kPgThreads) void pg_nb_total_count_grad_kernel(int64_t N, const double* __restrict__ y,
                                                                            const double* __restrict__ mean,
                                                                            const double* __restrict__ sdiag, double r, int Q,
                                                                            const double* __restrict__ nodes,
                                                                            const double* __restrict__ weights,
                                                                            double* __restrict__ part) {
    __shared__ double sx[kPgMaxNodes], sw[kPgMaxNodes];
    __shared__ double ssum[kPgThreads / 64];
    for (int q = threadIdx.x; q < Q; q += blockDim.x) {
        sx[q] = nodes[q];
        sw[q] = weights[q];
    }
    __syncthreads();
    const double psi_r = pg_digamma(r);
    double lsum = 0.0;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const double m = mean[n];
        const double s = sqrt(pg_clamp_min(sdiag[n], 0.0));
        double e = 0.0;
        for (int q = 0; q < Q; ++q) {
            const double t = -__dadd_rn(m, __dmul_rn(s, sx[q]));
            const double ls = __dsub_rn(fmin(t, 0.0), log1p(exp(-fabs(t))));
            e = __dadd_rn(e, __dmul_rn(ls, sw[q]));
        }
        lsum += __dadd_rn(__dsub_rn(pg_digamma(__dadd_rn(y[n], r)), psi_r), e);
    }
    lsum = pg_wave_sum(lsum);
    if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = ssum[0];
        for (int w = 1; w < kPgThreads / 64; ++w) v += ssum[w];
        part[blockIdx.x] = v;
    }
}

// one workgroup: the partials added in a fixed order (strided per thread, then the wave tree, then the waves in order)
__global__ __launch_bounds__(kPgThreads) void pg_sum_finish_kernel(int nparts, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double ssum[kPgThreads / 64];
    double v = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) v += part[i];
    v = pg_wave_sum(v);
    if ((threadIdx.x & 63) == 0) ssum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = ssum[0];
        for (int w = 1; w < kPgThreads / 64; ++w) t += ssum[w];
        out[0] = t;
    }
}

__global__ __launch_bounds__(kPgThreads) void pg_weight_rows_kernel(int64_t N, const double* __restrict__ probes, unsigned long long seed,
                                                                    const double* __restrict__ omega, double* __restrict__ out) {
    const int j = blockIdx.y;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const double z = probes ? probes[(int64_t)j * N + n] : efgp_rademacher(seed, j, n);
        out[(int64_t)j * N + n] = omega[n] * z;
    }
}

// per-workgroup partial sums of  D'[k,p] |bx_k|^2  and  D'[k,p] sum_j Re(conj(R_jk) b_jk)  (P <= 4 hypers)
__global__ __launch_bounds__(kPgThreads) void pg_mstep_partial_kernel(int64_t M, int J, int P, const double2* __restrict__ bx,
                                                                      const double2* __restrict__ bj, const double2* __restrict__ R,
                                                                      const double* __restrict__ dp, int dp_stride, double* __restrict__ part) {
    __shared__ double sp[kPgThreads / 64][2 * kPgMaxHypers];
    double t1[kPgMaxHypers] = {0.0, 0.0, 0.0, 0.0};
    double t2[kPgMaxHypers] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < M; k += (int64_t)gridDim.x * blockDim.x) {
        const double2 b = bx[k];
        const double a = b.x * b.x + b.y * b.y;
        double s = 0.0;
        for (int j = 0; j < J; ++j) {
            const double2 r = R[(int64_t)j * M + k], q = bj[(int64_t)j * M + k];
            s += r.x * q.x + r.y * q.y;                                   // Re(conj(r) q)
        }
#pragma unroll
        for (int p = 0; p < kPgMaxHypers; ++p) {
            if (p < P) {
                const double d = dp[(k * P + p) * dp_stride];
                t1[p] += d * a;
                t2[p] += d * s;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < kPgMaxHypers; ++p) {
        t1[p] = pg_wave_sum(t1[p]);
        t2[p] = pg_wave_sum(t2[p]);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int p = 0; p < kPgMaxHypers; ++p) {
            sp[threadIdx.x >> 6][p] = t1[p];
            sp[threadIdx.x >> 6][kPgMaxHypers + p] = t2[p];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * kPgMaxHypers) {
        double v = 0.0;
        for (int w = 0; w < kPgThreads / 64; ++w) v += sp[w][threadIdx.x];
        part[(int64_t)blockIdx.x * 2 * kPgMaxHypers + threadIdx.x] = v;
    }
}

// out = term1 (P) | term2 (P) | grad = (term1 - term2) / 2 (P): the partials added in block order by one thread per entry
__global__ __launch_bounds__(64) void pg_mstep_finish_kernel(int nparts, int J, int P, const double* __restrict__ part, double* __restrict__ out) {
    const int i = threadIdx.x;
    __shared__ double tv[2 * kPgMaxHypers];
    if (i < 2 * kPgMaxHypers) {
        double v = 0.0;
        for (int b = 0; b < nparts; ++b) v += part[(int64_t)b * 2 * kPgMaxHypers + i];
        tv[i] = i >= kPgMaxHypers ? (J > 0 ? v / (double)J : 0.0) : v;
    }
    __syncthreads();
    if (i < P) {
        out[i] = tv[i];
        out[P + i] = tv[kPgMaxHypers + i];
        out[2 * P + i] = 0.5 * (tv[i] - tv[kPgMaxHypers + i]);
    }
}

static int pg_blocks(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + kPgThreads - 1) / kPgThreads, kPgMaxBlocks));
}

// The E-step pass of either likelihood: the update kernel, then (when a scalar is wanted) the fixed-order finish.
template <class L>
static int pg_estep_launch(const char* what, int device, int64_t npts, int nprobes, const double* s_rows, const double* probes,
                           uint64_t seed, L lik, const double* targets, double rho, double* delta, double* mean_out,
                           double* sigma_diag_out, double* residual_out, typename L::Out* metric_out, void* stream_) {
    using Acc = typename L::Acc;
    EFGP_REQUIRE(npts >= 1 && nprobes >= 0, "%s: bad sizes (npts %lld, nprobes %d)", what, (long long)npts, nprobes);
    EFGP_REQUIRE(s_rows && targets && delta && mean_out && sigma_diag_out, "%s: null argument", what);
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = pg_blocks(npts);
    char* buf = (char*)scratch(ctx, SLOT_MISC, (size_t)blocks * (sizeof(double) + sizeof(Acc)));
    if (!buf) return EFGP_ENOMEM;
    double* part_max = (double*)buf;
    Acc* part_metric = (Acc*)(buf + (size_t)blocks * sizeof(double));
    hipLaunchKernelGGL(pg_estep_update_kernel<L>, dim3(blocks), dim3(kPgThreads), 0, stream, npts, nprobes, s_rows, probes,
                       (unsigned long long)seed, lik, targets, rho, delta, mean_out, sigma_diag_out, part_max, part_metric);
    EFGP_HIP_CHECK(hipGetLastError());
    if (residual_out || metric_out) {
        hipLaunchKernelGGL(pg_estep_finish_kernel<L>, dim3(1), dim3(kPgThreads), 0, stream, blocks, (const double*)part_max,
                           (const Acc*)part_metric, residual_out, metric_out);
        EFGP_HIP_CHECK(hipGetLastError());
    }
    return EFGP_OK;
}

}  // namespace efgp

using namespace efgp;

extern "C" {

int efgp_pg_estep_update(int device, int64_t npts, int nprobes, const double* s_rows, const double* probes, uint64_t seed,
                         const double* pg_b, const double* targets, double rho, double* delta, double* mean_out, double* sigma_diag_out,
                         double* residual_out, int64_t* correct_out, void* stream_) {
    return pg_estep_launch("efgp_pg_estep_update", device, npts, nprobes, s_rows, probes, seed, PgBernoulli{pg_b}, targets, rho,
                           delta, mean_out, sigma_diag_out, residual_out, correct_out, stream_);
}

int efgp_pg_nb_estep_update(int device, int64_t npts, int nprobes, const double* s_rows, const double* probes, uint64_t seed,
                            const double* targets, double total_count, double rho, double* delta, double* mean_out,
                            double* sigma_diag_out, double* residual_out, double* abs_err_sum_out, void* stream_) {
    EFGP_REQUIRE(total_count > 0.0, "efgp_pg_nb_estep_update: total_count must be positive (got %g)", total_count);
    return pg_estep_launch("efgp_pg_nb_estep_update", device, npts, nprobes, s_rows, probes, seed, PgNegativeBinomial{total_count},
                           targets, rho, delta, mean_out, sigma_diag_out, residual_out, abs_err_sum_out, stream_);
}

int efgp_pg_nb_total_count_grad(int device, int64_t npts, const double* targets, const double* mean, const double* sigma_diag,
                                double total_count, int nnodes, const double* nodes, const double* weights, double* grad_out,
                                void* stream_) {
    EFGP_REQUIRE(npts >= 1 && nnodes >= 1 && nnodes <= kPgMaxNodes, "efgp_pg_nb_total_count_grad: bad sizes (npts %lld, nnodes %d, "
                 "at most %d nodes)", (long long)npts, nnodes, kPgMaxNodes);
    EFGP_REQUIRE(total_count > 0.0, "efgp_pg_nb_total_count_grad: total_count must be positive (got %g)", total_count);
    EFGP_REQUIRE(targets && mean && sigma_diag && nodes && weights && grad_out, "efgp_pg_nb_total_count_grad: null argument");
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = pg_blocks(npts);
    double* part = (double*)scratch(ctx, SLOT_MISC, (size_t)blocks * sizeof(double));
    if (!part) return EFGP_ENOMEM;
    hipLaunchKernelGGL(pg_nb_total_count_grad_kernel, dim3(blocks), dim3(kPgThreads), 0, stream, npts, targets, mean, sigma_diag,
                       total_count, nnodes, nodes, weights, part);
    EFGP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pg_sum_finish_kernel, dim3(1), dim3(kPgThreads), 0, stream, blocks, (const double*)part, grad_out);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

int efgp_pg_weight_rows(int device, int64_t npts, int nrows, const double* probes, uint64_t seed, const double* omega, double* out,
                        void* stream_) {
    EFGP_REQUIRE(npts >= 1 && nrows >= 1 && nrows <= 65535, "efgp_pg_weight_rows: bad sizes");
    EFGP_REQUIRE(omega && out, "efgp_pg_weight_rows: null argument");
    if (!device_ctx(device)) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((npts + kPgThreads - 1) / kPgThreads, 512));
    hipLaunchKernelGGL(pg_weight_rows_kernel, dim3(blocks, nrows), dim3(kPgThreads), 0, (hipStream_t)stream_, npts, probes,
                       (unsigned long long)seed, omega, out);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

int efgp_pg_mstep_terms(int device, int64_t nmodes, int nprobes, int nhypers, const void* beta_x, const void* beta_probes,
                        const void* r_probes, const void* dprime, int dprime_is_complex, double* out, void* stream_) {
    EFGP_REQUIRE(nmodes >= 1 && nprobes >= 0 && nhypers >= 1 && nhypers <= kPgMaxHypers, "efgp_pg_mstep_terms: bad sizes");
    EFGP_REQUIRE(beta_x && dprime && out && (nprobes == 0 || (beta_probes && r_probes)), "efgp_pg_mstep_terms: null argument");
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = pg_blocks(nmodes);
    double* part = (double*)scratch(ctx, SLOT_MISC, (size_t)blocks * 2 * kPgMaxHypers * sizeof(double));
    if (!part) return EFGP_ENOMEM;
    hipLaunchKernelGGL(pg_mstep_partial_kernel, dim3(blocks), dim3(kPgThreads), 0, stream, nmodes, nprobes, nhypers, (const double2*)beta_x,
                       (const double2*)beta_probes, (const double2*)r_probes, (const double*)dprime, dprime_is_complex ? 2 : 1, part);
    EFGP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pg_mstep_finish_kernel, dim3(1), dim3(64), 0, stream, blocks, nprobes, nhypers, (const double*)part, out);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

}  // extern "C"
