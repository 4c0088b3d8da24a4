// Direct DFTs for the tiny grids of the 2-D EFGP step (fine grid <= 128 x 128, <= 64 modes per dimension).
//
// At N = 1e6 the fit + mean step spends ~45 us in nine dependent small launches around the two N-scale kernels, each
// 4.4-5 us, i.e. launch latency, for ~1 MFLOP of work.  On the type-2 side (precorrect + two rocFFT kernels, 14 us) a
// separable dense DFT from the 23 x 23 modes to the real fine grid (the headline's: 64 x 64 cells at tolerance 1e-7) is
// ONE launch of about 6 us (and sums in a fixed order in double: at least as accurate as the FFT route).  The same idea on the type-1 side (int64 grid 96 x 96 x 2 ->
// two mode boxes, replacing reduce + two rocFFT kernels + deconvolve = 19 us) measured 16.7-21 us in one launch: every
// workgroup has to pull the 147-KB grid through L2 and walk 96-term sums serially -- not kept.
// Reference operation replaced: the mode placement / correction + FFT inside finufft type 2 (efgpnd.py:1533-1536).
#include "small_dft.hpp"

#include "nufft_plan_host.hpp"

#include <algorithm>
#include <cstdlib>

namespace efgp {

constexpr int kDftThreads = 256;

// ---- type 2 side -------------------------------------------------------------------------------------------------
struct M2GArgs {
    const double2* f;
    const double2* mul;
    int nm0, nm1, modeord, isign;
    const double *fac0, *fac1;
    int nf0, nf1;
    double2* fine;
    double* image;      // non-null: write the pair gather's LDS image (nufft.hip, interp_real2_pair_kernel) instead of `fine`
    int p0, p1;         // image rows and row pitch
};

// The multiply-add chains of the kernel, written once for both of its arms.  a b - c d is fma(a, b, -(c d)) and a b + c d is
// fma(c, d, a b): the forms the compiler chose for the first version of this kernel, pinned so that both arms give its bits.
__device__ __forceinline__ double m2g_re(double ax, double ay, double bx, double by) { return fma(ax, bx, -(ay * by)); }
__device__ __forceinline__ double m2g_im(double ax, double ay, double bx, double by) { return fma(ay, bx, ax * by); }
__device__ __forceinline__ double2 m2g_cmul(double2 v, double2 m) {
    return make_double2(m2g_re(v.x, v.y, m.x, m.y), m2g_im(v.x, v.y, m.x, m.y));
}
__device__ __forceinline__ double2 m2g_scale(double2 v, double f0, double f1) {
    const double fc = f0 * f1;
    return make_double2(v.x * fc, v.y * fc);
}
__device__ __forceinline__ void m2g_acc(double& re, double& im, double2 v, double2 w) {
    re += m2g_re(v.x, v.y, w.x, w.y);
    im += m2g_im(v.x, v.y, w.x, w.y);
}

constexpr int kDftGroup = 8;          // LDS operand pairs in flight per group of terms
constexpr int kDftLoadTrips = 4;      // mode loads (f, mul, fac0, fac1) in flight per thread
static_assert(2 * kDftMaxNf <= kDftThreads, "one twiddle per thread");

// One workgroup per fine-grid row x0.  The corrected modes c = fac f mul go to LDS first (coalesced, CMCL order);
// t[k1] = sum_k0 c[k0][k1] e(k0 x0) with all threads (k1 x a slice of k0, combined through LDS); then
// fine[x0][x1] = Re sum_k1 t[k1] e(k1 x1).  Phases advance by addition.
// Image mode: the same doubles go straight to every place they hold in the gather's two halo-padded parity copies
// (copy cp at [r][c] is Re fine[r mod nf0][(c + cp) mod nf1]), so the gather's workgroups fill their LDS with a flat copy
// instead of each redoing the wrap, the real/imaginary split and the parity shift.
// SERIAL = false (default) keeps every sum's partition and term order and takes the dependent round trips out: the mode loads
// of a thread are issued before the twiddles (one sincospi per thread, tw0 on threads [0, nf0), tw1 on the next nf1), the LDS
// operands of a chain are read kDftGroup terms ahead of their multiply-adds, and the image stores of a cell are spread over
// all four waves.  SERIAL = true (EFGP_SMALL_DFT_SERIAL) is the first version's statement order; same bits.
template <bool SERIAL>
__global__ __launch_bounds__(kDftThreads) void modes_to_grid_real_kernel(M2GArgs a) {
    __shared__ double2 tw0[kDftMaxNf], tw1[kDftMaxNf], t[64], part[4][64];
    __shared__ double res[kDftMaxNf];                                 // !SERIAL: Re fine[x0][.] on its way to the image
    extern __shared__ double2 cm[];                                   // [nm0][nm1] corrected modes, CMCL order
    const int nf0 = a.nf0, nf1 = a.nf1, nm0 = a.nm0, nm1 = a.nm1;
    const double sgn = a.isign < 0 ? -2.0 : 2.0;
    if constexpr (SERIAL) {
        for (int i = threadIdx.x; i < nf0; i += kDftThreads) {
            double s, c;
            sincospi(sgn * (double)i / (double)nf0, &s, &c);
            tw0[i] = make_double2(c, s);
        }
        for (int i = threadIdx.x; i < nf1; i += kDftThreads) {
            double s, c;
            sincospi(sgn * (double)i / (double)nf1, &s, &c);
            tw1[i] = make_double2(c, s);
        }
        for (int i = threadIdx.x; i < nm0 * nm1; i += kDftThreads) {
            const int s0 = i / nm1, s1 = i - s0 * nm1;
            const int k0 = s0 - nm0 / 2, k1 = s1 - nm1 / 2;
            const int slot0 = a.modeord == 0 ? s0 : (k0 >= 0 ? k0 : k0 + nm0);
            const int slot1 = a.modeord == 0 ? s1 : (k1 >= 0 ? k1 : k1 + nm1);
            const int64_t idx = (int64_t)slot0 * nm1 + slot1;
            double2 v = a.f[idx];
            if (a.mul) v = m2g_cmul(v, a.mul[idx]);
            cm[i] = m2g_scale(v, a.fac0[s0], a.fac1[s1]);
        }
    } else {
        const int nmodes = nm0 * nm1;
        const bool has_mul = a.mul != nullptr;
        bool tables = false;
        for (int base = threadIdx.x; base < nmodes || !tables; base += kDftLoadTrips * kDftThreads) {
            double2 v[kDftLoadTrips], m[kDftLoadTrips];
            double f0[kDftLoadTrips], f1[kDftLoadTrips];
#pragma unroll
            for (int j = 0; j < kDftLoadTrips; ++j) {                  // a trip past the end loads the last mode again
                const int i = min(base + j * kDftThreads, nmodes - 1);
                const int s0 = i / nm1, s1 = i - s0 * nm1;
                const int k0 = s0 - nm0 / 2, k1 = s1 - nm1 / 2;
                const int slot0 = a.modeord == 0 ? s0 : (k0 >= 0 ? k0 : k0 + nm0);
                const int slot1 = a.modeord == 0 ? s1 : (k1 >= 0 ? k1 : k1 + nm1);
                const int64_t idx = (int64_t)slot0 * nm1 + slot1;
                v[j] = a.f[idx];
                m[j] = has_mul ? a.mul[idx] : make_double2(0.0, 0.0);
                f0[j] = a.fac0[s0];
                f1[j] = a.fac1[s1];
            }
            if (!tables) {                                             // behind the loads of the first group, in their shadow
                const int i = threadIdx.x;
                const bool first = i < nf0;
                const int q = first ? i : i - nf0, n = first ? nf0 : nf1;
                if (q < n) {
                    double s, c;
                    sincospi(sgn * (double)q / (double)n, &s, &c);
                    (first ? tw0 : tw1)[q] = make_double2(c, s);
                }
                tables = true;
            }
#pragma unroll
            for (int j = 0; j < kDftLoadTrips; ++j) {
                const int i = base + j * kDftThreads;
                if (i < nmodes) cm[i] = m2g_scale(has_mul ? m2g_cmul(v[j], m[j]) : v[j], f0[j], f1[j]);
            }
        }
    }
    __syncthreads();
    const int x0 = blockIdx.x;
    {   // thread = (k1, quarter of the k0 range)
        const int s1 = threadIdx.x & 63, qtr = threadIdx.x >> 6;
        if (s1 < nm1) {
            const int lo = (nm0 * qtr) / 4, hi = (nm0 * (qtr + 1)) / 4;
            int ph = (int)(((int64_t)(lo - nm0 / 2) * x0) % nf0);
            ph = ph < 0 ? ph + nf0 : ph;
            double re = 0.0, im = 0.0;
            if constexpr (SERIAL) {
                for (int s0 = lo; s0 < hi; ++s0) {
                    const double2 v = cm[s0 * nm1 + s1], w = tw0[ph];
                    m2g_acc(re, im, v, w);
                    ph += x0;
                    ph = ph >= nf0 ? ph - nf0 : ph;
                }
            } else {
                for (int g0 = lo; g0 < hi; g0 += kDftGroup) {
                    const int n = min(kDftGroup, hi - g0);
                    double2 v[kDftGroup], w[kDftGroup];
#pragma unroll
                    for (int j = 0; j < kDftGroup; ++j) {              // reads past the group's end repeat its last term
                        v[j] = cm[(g0 + min(j, n - 1)) * nm1 + s1];
                        w[j] = tw0[ph];
                        ph += x0;
                        ph = ph >= nf0 ? ph - nf0 : ph;
                    }
                    __builtin_amdgcn_sched_barrier(0);                 // every read of the group in front of its multiply-adds
#pragma unroll
                    for (int j = 0; j < kDftGroup; ++j)
                        if (j == 0 || j < n) m2g_acc(re, im, v[j], w[j]);
                }
            }
            part[qtr][s1] = make_double2(re, im);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nm1) {
        const int s1 = threadIdx.x;
        t[s1] = make_double2(part[0][s1].x + part[1][s1].x + part[2][s1].x + part[3][s1].x,
                             part[0][s1].y + part[1][s1].y + part[2][s1].y + part[3][s1].y);
    }
    __syncthreads();
    if constexpr (SERIAL) {
        for (int x1 = threadIdx.x; x1 < nf1; x1 += kDftThreads) {
            int ph = (int)(((int64_t)(-(nm1 / 2)) * x1) % nf1);
            ph = ph < 0 ? ph + nf1 : ph;
            double re = 0.0;
            for (int s1 = 0; s1 < nm1; ++s1) {
                re += m2g_re(t[s1].x, t[s1].y, tw1[ph].x, tw1[ph].y);
                ph += x1;
                ph = ph >= nf1 ? ph - nf1 : ph;
            }
            if (a.image == nullptr) {
                a.fine[(int64_t)x0 * nf1 + x1] = make_double2(re, 0.0);
                continue;
            }
            const int p1 = a.p1, plane = a.p0 * p1;
            for (int r = x0; r < a.p0; r += nf0) {
                double* row = a.image + r * p1;
                for (int c = x1; c < p1; c += nf1) row[c] = re;
                for (int c = x1 == 0 ? nf1 - 1 : x1 - 1; c < p1; c += nf1) row[plane + c] = re;      // copy 1 holds column c + 1
            }
        }
    } else {
        const int x1 = threadIdx.x;                                    // nf1 <= kDftMaxNf < kDftThreads: one chain per thread
        if (x1 < nf1) {
            int ph = (int)(((int64_t)(-(nm1 / 2)) * x1) % nf1);
            ph = ph < 0 ? ph + nf1 : ph;
            double re = 0.0;
            for (int g0 = 0; g0 < nm1; g0 += kDftGroup) {
                const int n = min(kDftGroup, nm1 - g0);
                double2 v[kDftGroup], w[kDftGroup];
#pragma unroll
                for (int j = 0; j < kDftGroup; ++j) {
                    v[j] = t[g0 + min(j, n - 1)];
                    w[j] = tw1[ph];
                    ph += x1;
                    ph = ph >= nf1 ? ph - nf1 : ph;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < kDftGroup; ++j)
                    if (j == 0 || j < n) re += m2g_re(v[j].x, v[j].y, w[j].x, w[j].y);
            }
            if (a.image == nullptr) a.fine[(int64_t)x0 * nf1 + x1] = make_double2(re, 0.0);
            else res[x1] = re;
        }
        if (a.image == nullptr) return;
        __syncthreads();
        // the places of cell x1 in the image (rows r, two copies, columns c: eight at most for the gather's halos), dealt out
        // over the nsl threads that share x1
        const int nsl = kDftThreads / nf1, sl = (int)threadIdx.x / nf1, c0 = (int)threadIdx.x - sl * nf1;
        if (sl >= nsl) return;
        const double re = res[c0];
        const int p1 = a.p1, plane = a.p0 * p1;
        int turn = sl;
        for (int r = x0; r < a.p0; r += nf0) {
            double* row = a.image + r * p1;
            for (int c = c0; c < p1; c += nf1) {
                if (turn == 0) row[c] = re;
                turn = turn == 0 ? nsl - 1 : turn - 1;
            }
            for (int c = c0 == 0 ? nf1 - 1 : c0 - 1; c < p1; c += nf1) {                              // copy 1 holds column c + 1
                if (turn == 0) row[plane + c] = re;
                turn = turn == 0 ? nsl - 1 : turn - 1;
            }
        }
    }
}


int modes_to_grid_real_launch(DeviceCtx* ctx, const double2* f, const double2* mul, int nm0, int nm1, int modeord, int isign,
                              const double* fac0, const double* fac1, int nf0, int nf1, double2* fine, double* image, int p0, int p1,
                              hipStream_t stream) {
    (void)ctx;
    M2GArgs a{f, mul, nm0, nm1, modeord, isign, fac0, fac1, nf0, nf1, fine, image, p0, p1};
    const size_t lds = (size_t)nm0 * nm1 * sizeof(double2);
    const bool serial = std::getenv("EFGP_SMALL_DFT_SERIAL") != nullptr;      // comparison hook: the first version's statement order
    const void* fn = serial ? (const void*)modes_to_grid_real_kernel<true> : (const void*)modes_to_grid_real_kernel<false>;
    if (lds > 32 * 1024) EFGP_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (serial) hipLaunchKernelGGL(modes_to_grid_real_kernel<true>, dim3(nf0), dim3(kDftThreads), lds, stream, a);
    else hipLaunchKernelGGL(modes_to_grid_real_kernel<false>, dim3(nf0), dim3(kDftThreads), lds, stream, a);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}

}  // namespace efgp
