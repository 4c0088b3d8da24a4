// N-scale and M-scale passes of the Polya-Gamma (PG) GP classifier behind the C ABI
// (reference: polyagamma_classification/pg_classifier.py):
//   efgp_pg_estep_update  one pass over the N points after the E-step solves (:552-569, :252-257, :129-138)
//   efgp_pg_weight_rows   omega .* z for the M-step's R = F*(omega z) right-hand rows (:616)
//   efgp_pg_mstep_terms   term1 / term2 / gradient of the M-step in feature space (:616-623)
// Both reductions are two launches: per-workgroup partials over a grid whose size depends only on the problem size, then one
// workgroup that adds them in a fixed order -- a seeded fit is bit-reproducible run to run (no floating-point atomics).
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "nufft_dev.hpp"

namespace efgp {

constexpr int kPgThreads = 256;          // four wave64 per workgroup
constexpr int kPgMaxBlocks = 1024;
constexpr int kPgMaxHypers = 4;

__device__ __forceinline__ double pg_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ double pg_wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// One thread per point (grid-stride).  Explicit _rn operations keep the compiler from contracting the reference's separate
// multiplies and adds into FMAs, so the per-point values round as the reference's torch expressions do.
__global__ __launch_bounds__(kPgThreads) void pg_estep_update_kernel(int64_t N, int J, const double* __restrict__ S,
                                                                     const double* __restrict__ probes, unsigned long long seed,
                                                                     const double* __restrict__ pg_b, const double* __restrict__ y,
                                                                     double rho, double* __restrict__ delta, double* __restrict__ mean_out,
                                                                     double* __restrict__ sdiag_out, double* __restrict__ part_max,
                                                                     unsigned long long* __restrict__ part_cnt) {
    __shared__ double smax[kPgThreads / 64];
    __shared__ unsigned long long scnt[kPgThreads / 64];
    double lmax = 0.0;
    unsigned long long lcnt = 0;
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
        const double b = pg_b ? pg_b[n] : 1.0;
        // c2 = clamp_min(sigma_diag + mean^2, 1e-12); Lambda = E[omega] of PG(b, c)  (:557-559, :252-257)
        const double c2 = fmax(__dadd_rn(sd, __dmul_rn(m, m)), 1e-12);
        const double c = sqrt(c2);
        const double sc = fmax(c, 1e-12);
        const double lam = c > 1e-8 ? __ddiv_rn(__dmul_rn(__dmul_rn(0.5, b), tanh(__dmul_rn(0.5, sc))), sc) : __dmul_rn(0.25, b);
        // damped update and clamp (:561-563)
        const double dn = fmax(__dadd_rn(__dmul_rn(delta[n], one_m_rho), __dmul_rn(rho, lam)), 0.0);
        delta[n] = dn;
        mean_out[n] = m;
        sdiag_out[n] = sd;
        lmax = fmax(lmax, fabs(__dsub_rn(dn, lam)));
        // training accuracy of the logistic-Gaussian approximation (:129-138, :173-191)
        const double den = sqrt(__dadd_rn(1.0, __dmul_rn(M_PI / 8.0, fmax(sd, 0.0))));
        const double p = 1.0 / (1.0 + exp(-__ddiv_rn(m, den)));
        lcnt += ((p > 0.5) == (y[n] != 0.0)) ? 1ull : 0ull;
    }
    lmax = pg_wave_max(lmax);
    for (int off = 32; off > 0; off >>= 1) lcnt += __shfl_down(lcnt, off, 64);
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = lmax;
        scnt[threadIdx.x >> 6] = lcnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bm = smax[0];
        unsigned long long bc = scnt[0];
        for (int w = 1; w < kPgThreads / 64; ++w) {
            bm = fmax(bm, smax[w]);
            bc += scnt[w];
        }
        part_max[blockIdx.x] = bm;
        part_cnt[blockIdx.x] = bc;
    }
}

__global__ __launch_bounds__(kPgThreads) void pg_estep_finish_kernel(int nparts, const double* __restrict__ part_max,
                                                                     const unsigned long long* __restrict__ part_cnt,
                                                                     double* __restrict__ resid_out, int64_t* __restrict__ count_out) {
    __shared__ double smax[kPgThreads / 64];
    __shared__ unsigned long long scnt[kPgThreads / 64];
    double m = 0.0;
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
        m = fmax(m, part_max[i]);
        c += part_cnt[i];
    }
    m = pg_wave_max(m);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = m;
        scnt[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bm = smax[0];
        unsigned long long bc = scnt[0];
        for (int w = 1; w < kPgThreads / 64; ++w) {
            bm = fmax(bm, smax[w]);
            bc += scnt[w];
        }
        if (resid_out) resid_out[0] = bm;
        if (count_out) count_out[0] = (int64_t)bc;
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

}  // namespace efgp

using namespace efgp;

extern "C" {

int efgp_pg_estep_update(int device, int64_t npts, int nprobes, const double* s_rows, const double* probes, uint64_t seed,
                         const double* pg_b, const double* targets, double rho, double* delta, double* mean_out, double* sigma_diag_out,
                         double* residual_out, int64_t* correct_out, void* stream_) {
    EFGP_REQUIRE(npts >= 1 && nprobes >= 0, "efgp_pg_estep_update: bad sizes (npts %lld, nprobes %d)", (long long)npts, nprobes);
    EFGP_REQUIRE(s_rows && targets && delta && mean_out && sigma_diag_out, "efgp_pg_estep_update: null argument");
    DeviceCtx* ctx = device_ctx(device);
    if (!ctx) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = pg_blocks(npts);
    char* buf = (char*)scratch(ctx, SLOT_MISC, (size_t)blocks * (sizeof(double) + sizeof(unsigned long long)));
    if (!buf) return EFGP_ENOMEM;
    double* part_max = (double*)buf;
    unsigned long long* part_cnt = (unsigned long long*)(buf + (size_t)blocks * sizeof(double));
    hipLaunchKernelGGL(pg_estep_update_kernel, dim3(blocks), dim3(kPgThreads), 0, stream, npts, nprobes, s_rows, probes,
                       (unsigned long long)seed, pg_b, targets, rho, delta, mean_out, sigma_diag_out, part_max, part_cnt);
    EFGP_HIP_CHECK(hipGetLastError());
    if (residual_out || correct_out) {
        hipLaunchKernelGGL(pg_estep_finish_kernel, dim3(1), dim3(kPgThreads), 0, stream, blocks, (const double*)part_max,
                           (const unsigned long long*)part_cnt, residual_out, correct_out);
        EFGP_HIP_CHECK(hipGetLastError());
    }
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
