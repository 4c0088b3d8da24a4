// Device code shared by the Toeplitz translation units (toeplitz_cg.hip, cg_multi.hip, cg_coop2d.hip): the small helpers of their
// kernels and the in-LDS line transforms that both CG solvers call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cg_plan_host.hpp"
#include "toeplitz_cg.hpp"

namespace efgp {

constexpr int kVecThreads = 256;
constexpr int kCgThreads = 512;
constexpr double kDivEps = 1e-16;   // cg.py:57

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// index of block element `flat` (row-major over n) inside the padded FFT grid, shifted by `off` per dim
__device__ __forceinline__ int64_t pad_index(const ToepGeom& g, int64_t flat, int64_t off_mul) {
    int64_t idx = 0, stride = 1;
    for (int a = g.d - 1; a >= 0; --a) {
        int64_t ia = flat % g.n[a];
        flat /= g.n[a];
        idx += (ia + off_mul * (g.n[a] - 1)) * stride;
        stride *= g.F[a];
    }
    return idx;
}

// the same in 32-bit arithmetic (grids of the CG path have far fewer than 2^31 cells): a third of the ALU work
__device__ __forceinline__ int pad_index32(const ToepGeom& g, int flat, int off_mul) {
    int idx = 0, stride = 1;
    for (int a = g.d - 1; a >= 0; --a) {
        const int na = (int)g.n[a];
        const int q = flat / na;
        const int ia = flat - q * na;
        flat = q;
        idx += (ia + off_mul * (na - 1)) * stride;
        stride *= (int)g.F[a];
    }
    return idx;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    // wave reduce (64 lanes) then across waves through LDS
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double t = 0.0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) t += red[i];     // same order in every thread: deterministic
    return t;
}

// ---- line transforms in LDS (the multi-launch line kernels and the cooperative kernels) ---------------------------------------------
// kLineThreads, kCoopMaxG, kCoopLoads: cg_plan_host.hpp (the host's planners use them too)

__device__ __forceinline__ int ilog2(int v) { return 31 - __clz(v); }

// forward FFT of `nl` lines of length F (a power of two) held in A (line l at A + l*ld); result in the returned
// buffer (A or B).  `tw` = exp(-2 pi i q / F), q < F, in LDS.
__device__ __forceinline__ double2* line_fft(double2* A, double2* B, int F, int ld, int nl, const double2* tw) {
    double2* x = A;
    double2* y = B;
    int Ns = 1;
    while (Ns < F) {
        // radix 8 for the LATER stages where the remaining length allows it (a first radix-8 stage writes with a stride of 8
        // elements: 8-way bank conflicts): a stage is one LDS round trip and one barrier, and a radix-8 butterfly gives
        // its thread 8 independent loads (radix-4 stages are bound by the LDS latency of dependent work items)
        const int rem = F / Ns;
        const int R = (F >= 256 && (rem == 512 || rem == 64 || rem == 8)) ? 8 : ((rem & 3) == 0 ? 4 : 2);   // 256 = 4 8 8, 512 = 8 8 8
        // (measured, cooperative solve: 512^2 49.8 -> 40.4 us per iteration, 256^2 neutral, 128^2 = 4 4 8 slower than 4 4 4 2)
        const int per = F / R;                       // butterflies per line (a power of two)
        const int lper = ilog2(per);
        const int mult = F / (Ns * R);               // twiddle index step: angle = -2 pi r k / (Ns R)
        for (int w = threadIdx.x; w < (nl << lper); w += kLineThreads) {
            const int l = w >> lper, j = w & (per - 1);
            const int k = j & (Ns - 1);
            const double2* xl = x + l * ld;
            double2* yl = y + l * ld;
            const int j0 = (j - k) * R + k;
            if (R == 8) {
                double2 v[8];
#pragma unroll
                for (int m = 0; m < 8; ++m) v[m] = xl[j + m * per];
                if (Ns > 1) {
                    const int q = k * mult;          // 7 q < F: no wrap
#pragma unroll
                    for (int m = 1; m < 8; ++m) v[m] = cmul(v[m], tw[m * q]);
                }
                // DFT-8: two DFT-4 (even / odd inputs), odd outputs times w8^m, combine
                const double2 e0 = make_double2(v[0].x + v[4].x, v[0].y + v[4].y), e1 = make_double2(v[0].x - v[4].x, v[0].y - v[4].y);
                const double2 e2 = make_double2(v[2].x + v[6].x, v[2].y + v[6].y), e3 = make_double2(v[2].y - v[6].y, v[6].x - v[2].x);
                const double2 E0 = make_double2(e0.x + e2.x, e0.y + e2.y), E1 = make_double2(e1.x + e3.x, e1.y + e3.y);
                const double2 E2 = make_double2(e0.x - e2.x, e0.y - e2.y), E3 = make_double2(e1.x - e3.x, e1.y - e3.y);
                const double2 o0 = make_double2(v[1].x + v[5].x, v[1].y + v[5].y), o1 = make_double2(v[1].x - v[5].x, v[1].y - v[5].y);
                const double2 o2 = make_double2(v[3].x + v[7].x, v[3].y + v[7].y), o3 = make_double2(v[3].y - v[7].y, v[7].x - v[3].x);
                const double2 O0 = make_double2(o0.x + o2.x, o0.y + o2.y), O1r = make_double2(o1.x + o3.x, o1.y + o3.y);
                const double2 O2r = make_double2(o0.x - o2.x, o0.y - o2.y), O3r = make_double2(o1.x - o3.x, o1.y - o3.y);
                const double hh = 0.70710678118654752440;
                const double2 O1 = make_double2(hh * (O1r.x + O1r.y), hh * (O1r.y - O1r.x));
                const double2 O2 = make_double2(O2r.y, -O2r.x);
                const double2 O3 = make_double2(hh * (O3r.y - O3r.x), -hh * (O3r.x + O3r.y));
                yl[j0] = make_double2(E0.x + O0.x, E0.y + O0.y);
                yl[j0 + Ns] = make_double2(E1.x + O1.x, E1.y + O1.y);
                yl[j0 + 2 * Ns] = make_double2(E2.x + O2.x, E2.y + O2.y);
                yl[j0 + 3 * Ns] = make_double2(E3.x + O3.x, E3.y + O3.y);
                yl[j0 + 4 * Ns] = make_double2(E0.x - O0.x, E0.y - O0.y);
                yl[j0 + 5 * Ns] = make_double2(E1.x - O1.x, E1.y - O1.y);
                yl[j0 + 6 * Ns] = make_double2(E2.x - O2.x, E2.y - O2.y);
                yl[j0 + 7 * Ns] = make_double2(E3.x - O3.x, E3.y - O3.y);
            } else if (R == 4) {
                double2 v0 = xl[j], v1 = xl[j + per], v2 = xl[j + 2 * per], v3 = xl[j + 3 * per];
                if (Ns > 1) {
                    const int q = k * mult;          // 3 q < F: no wrap
                    v1 = cmul(v1, tw[q]);
                    v2 = cmul(v2, tw[2 * q]);
                    v3 = cmul(v3, tw[3 * q]);
                }
                const double2 t0 = make_double2(v0.x + v2.x, v0.y + v2.y), t1 = make_double2(v0.x - v2.x, v0.y - v2.y);
                const double2 t2 = make_double2(v1.x + v3.x, v1.y + v3.y);
                const double2 t3 = make_double2(v1.y - v3.y, v3.x - v1.x);          // -i (v1 - v3)
                yl[j0] = make_double2(t0.x + t2.x, t0.y + t2.y);
                yl[j0 + Ns] = make_double2(t1.x + t3.x, t1.y + t3.y);
                yl[j0 + 2 * Ns] = make_double2(t0.x - t2.x, t0.y - t2.y);
                yl[j0 + 3 * Ns] = make_double2(t1.x - t3.x, t1.y - t3.y);
            } else {
                double2 v0 = xl[j], v1 = xl[j + per];
                if (Ns > 1) v1 = cmul(v1, tw[k * mult]);
                yl[j0] = make_double2(v0.x + v1.x, v0.y + v1.y);
                yl[j0 + Ns] = make_double2(v0.x - v1.x, v0.y - v1.y);
            }
        }
        __syncthreads();
        double2* t = x;
        x = y;
        y = t;
        Ns *= R;
    }
    return x;
}

// ---- in-wave line transform (lengths 128, 256, 512) ---------------------------------------------------------------------
// A line of F = 64 R points (R = 2, 4, 8) is transformed by 8 R lanes of ONE wave, 8 points per lane, as R interleaved
// 64-point transforms (x[R m + r], r < R: radix 8 x 8 inside 8 adjacent lanes, as in cg_persistent.hip) followed by one
// radix-R combine over r:   X[k1 + 64 k2] = sum_r w_F^(r k1) w_R^(r k2) Y_r[k1].
// Three LDS exchanges, each written and read by the line's own lanes (wave fences, no workgroup barrier), all with
// conflict-free patterns: exchange 1 (inside the 64-point transforms) XOR-swizzled in the destination line, exchange 2
// in [r][k1] order in the source line (its contents are in registers by then), the result in natural order in the
// destination line.  ~230 fp64 instructions and 48 LDS accesses per lane for 8 points, no index arithmetic in loops.
// The generic Stockham stages above cost 1.5-2.5 k cycles per work item (measured in the cooperative solve).
__device__ __forceinline__ void dft8_inplace(double2 (&v)[8]) {
    const double2 e0 = make_double2(v[0].x + v[4].x, v[0].y + v[4].y), e1 = make_double2(v[0].x - v[4].x, v[0].y - v[4].y);
    const double2 e2 = make_double2(v[2].x + v[6].x, v[2].y + v[6].y), e3 = make_double2(v[2].y - v[6].y, v[6].x - v[2].x);
    const double2 E0 = make_double2(e0.x + e2.x, e0.y + e2.y), E1 = make_double2(e1.x + e3.x, e1.y + e3.y);
    const double2 E2 = make_double2(e0.x - e2.x, e0.y - e2.y), E3 = make_double2(e1.x - e3.x, e1.y - e3.y);
    const double2 o0 = make_double2(v[1].x + v[5].x, v[1].y + v[5].y), o1 = make_double2(v[1].x - v[5].x, v[1].y - v[5].y);
    const double2 o2 = make_double2(v[3].x + v[7].x, v[3].y + v[7].y), o3 = make_double2(v[3].y - v[7].y, v[7].x - v[3].x);
    const double2 O0 = make_double2(o0.x + o2.x, o0.y + o2.y), O1r = make_double2(o1.x + o3.x, o1.y + o3.y);
    const double2 O2r = make_double2(o0.x - o2.x, o0.y - o2.y), O3r = make_double2(o1.x - o3.x, o1.y - o3.y);
    const double hh = 0.70710678118654752440;
    const double2 O1 = make_double2(hh * (O1r.x + O1r.y), hh * (O1r.y - O1r.x));
    const double2 O2 = make_double2(O2r.y, -O2r.x);
    const double2 O3 = make_double2(hh * (O3r.y - O3r.x), -hh * (O3r.x + O3r.y));
    v[0] = make_double2(E0.x + O0.x, E0.y + O0.y);
    v[1] = make_double2(E1.x + O1.x, E1.y + O1.y);
    v[2] = make_double2(E2.x + O2.x, E2.y + O2.y);
    v[3] = make_double2(E3.x + O3.x, E3.y + O3.y);
    v[4] = make_double2(E0.x - O0.x, E0.y - O0.y);
    v[5] = make_double2(E1.x - O1.x, E1.y - O1.y);
    v[6] = make_double2(E2.x - O2.x, E2.y - O2.y);
    v[7] = make_double2(E3.x - O3.x, E3.y - O3.y);
}
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// forward transform of nl lines (line l at src + l * ld, natural order) into dst + l * ld (natural order); src is destroyed.
// tw = exp(-2 pi i q / F), q < F, in LDS.  Ends with a workgroup barrier.
// MUL = 1: the outputs are multiplied by mul[k * mul_stride + l] (entry k of line l) and conjugated on the way out -- the
// spectrum multiply and the conjugation in front of the inverse transform, done on the registers that hold the result;
// the return value is the thread's share of sum Re(mul) |X|^2 (with the centred spectrum: <w, T w> by Parseval).
// MUL = 2 (round 3, Hermitian cooperative solve): line l carries TWO real columns as real and imaginary part; they are
// multiplied by the REAL spectra Re mul[k * mul_stride + l] and Re mul[k * mul_stride + l + mul_pair], halved (the unpacking
// behind the inverse transform adds two terms) and conjugated; the return value is sum S_a re^2 + S_b im^2.
// MUL = 3: the same with `mul` pointing at an array of REAL spectrum values (3-D Hermitian iteration: half the bytes).
// MUL = 5: the thread's eight spectrum pairs are handed in (`mul` = its register array, filled by spectrum_prefetch<R> before the
// data of the lines was even loaded: 3-D mid0 kernel, one pass of <= 256 / (8 R) lines).
// MUL = 4: the same with the two real spectra of every line already in LDS as double2 pairs, `mul`[k * mul_stride + l] (the
// cooperative Hermitian solve keeps its workgroup's slice there: no global round trip inside the transform).
// B = 48 (round 4): lines of 48 R points (96, 192, 384 = 3 * 2^k) -- the smallest smooth circulant grids between the powers of two.
// The R interleaved sub-transforms are 48-point lines as 6 x 8 in eight lanes (cg_herm.hip, cg_herm48_kernel: radix 6 on
// eight lanes, writer-side twiddles, radix 8 on six lanes), the sub-blocks of the exchanges are 48 entries long, and the combine
// over r hands 48 / (8 R) = 3, 1.5, 0.75 butterflies to a lane (predicated beyond 48).
__device__ __forceinline__ void dft3_inplace(double2 b0, double2 b1, double2 b2, double2& x0, double2& x1, double2& x2) {
    const double s = 0.86602540378443864676;
    const double2 sm = make_double2(b1.x + b2.x, b1.y + b2.y), df = make_double2(b1.x - b2.x, b1.y - b2.y);
    x0 = make_double2(b0.x + sm.x, b0.y + sm.y);
    const double2 m = make_double2(fma(-0.5, sm.x, b0.x), fma(-0.5, sm.y, b0.y));
    x1 = make_double2(fma(s, df.y, m.x), fma(-s, df.x, m.y));
    x2 = make_double2(fma(-s, df.y, m.x), fma(s, df.x, m.y));
}
__device__ __forceinline__ void dft6_inplace(double2 (&v)[6]) {
    const double s = 0.86602540378443864676;
    double2 e0, e1, e2, o0, o1, o2;
    dft3_inplace(v[0], v[2], v[4], e0, e1, e2);
    dft3_inplace(v[1], v[3], v[5], o0, o1, o2);
    const double2 w1 = make_double2(fma(s, o1.y, 0.5 * o1.x), fma(-s, o1.x, 0.5 * o1.y));
    const double2 w2 = make_double2(fma(s, o2.y, -0.5 * o2.x), fma(-s, o2.x, -0.5 * o2.y));
    v[0] = make_double2(e0.x + o0.x, e0.y + o0.y);
    v[3] = make_double2(e0.x - o0.x, e0.y - o0.y);
    v[1] = make_double2(e1.x + w1.x, e1.y + w1.y);
    v[4] = make_double2(e1.x - w1.x, e1.y - w1.y);
    v[2] = make_double2(e2.x + w2.x, e2.y + w2.y);
    v[5] = make_double2(e2.x - w2.x, e2.y - w2.y);
}

template <int R, int MUL = 0, int B = 64>
__device__ __forceinline__ double line_fft_inwave(double2* src, double2* dst, int ld, int nl, const double2* tw,
                                                  const double2* __restrict__ mul = nullptr, int64_t mul_stride = 0,
                                                  int64_t mul_pair = 0) {
    static_assert(B == 64 || (B == 48 && R >= 2), "sub-transforms of 64 points, or of 48 points under a combine");
    constexpr int LPL = 8 * R, LINES = kLineThreads / LPL;
    constexpr int U = B == 64 ? (R > 1 ? 8 / R : 1) : (48 + LPL - 1) / LPL;       // k1 values per lane in the combine
    constexpr bool kPartial = B == 48 && U * LPL != 48;                          // the last k1 of a lane may lie beyond the block
    double psum = 0.0;          // MUL: this thread's share of sum_k Re(mul_k) |X_k|^2 over its lines (Parseval: <w, T w>)
    const int li = threadIdx.x & (LPL - 1), lsub = threadIdx.x / LPL;
    const int r = li >> 3, j = li & 7;
    for (int l0 = 0; l0 < nl; l0 += LINES) {
        const bool act = l0 + lsub < nl;
        double2* s = src + (act ? l0 + lsub : l0) * ld;
        double2* d = dst + (act ? l0 + lsub : l0) * ld;
        double2 v[8];
        if (B == 64) {
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = s[R * (j + 8 * t) + r];
            dft8_inplace(v);
            wave_sync_lds();
            if (act) {
#pragma unroll
                for (int m = 0; m < 8; ++m) d[r * 64 + 8 * j + (m ^ j)] = v[m];
            }
            wave_sync_lds();
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = d[r * 64 + 8 * t + (j ^ t)];
#pragma unroll
            for (int t = 1; t < 8; ++t) v[t] = cmul(v[t], tw[R * j * t]);            // w_64^(j t)
            dft8_inplace(v);                                                        // v[t] = Y_r[j + 8 t]
        } else {
            double2 u6[6];
#pragma unroll
            for (int t = 0; t < 6; ++t) u6[t] = s[R * (j + 8 * t) + r];
            dft6_inplace(u6);
#pragma unroll
            for (int k = 1; k < 6; ++k) u6[k] = cmul(u6[k], tw[R * j * k]);          // w_48^(j k), writer side (35 R < 48 R: no wrap)
            wave_sync_lds();
            if (act) {
#pragma unroll
                for (int k = 0; k < 6; ++k) d[r * 48 + 6 * j + k] = u6[k];
            }
            wave_sync_lds();
            const int jr = j < 6 ? j : 0;                                           // lanes 6, 7 of a sub-transform idle from here on
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = d[r * 48 + 6 * t + jr];
            dft8_inplace(v);                                                        // v[t] = Y_r[j + 6 t], j < 6
        }
        if (R == 1) {                                                           // a plain 64-point line: done
            if (MUL) {
                double2 mv[8];
                const int lq = act ? l0 + lsub : l0;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if (MUL == 5) {
                        mv[t] = mul[t];
                    } else if (MUL == 4) {
                        mv[t] = mul[(j + 8 * t) * (int)mul_stride + lq];
                    } else if (MUL == 3) {
                        const double* rs = reinterpret_cast<const double*>(mul);
                        mv[t] = make_double2(rs[(int64_t)(j + 8 * t) * mul_stride + lq], rs[(int64_t)(j + 8 * t) * mul_stride + lq + mul_pair]);
                    } else {
                        mv[t] = mul[(int64_t)(j + 8 * t) * mul_stride + lq];
                        if (MUL == 2) mv[t].y = mul[(int64_t)(j + 8 * t) * mul_stride + lq + mul_pair].x;
                    }
                }
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if (MUL >= 2) {
                        if (act) psum += mv[t].x * v[t].x * v[t].x + mv[t].y * v[t].y * v[t].y;
                        v[t] = make_double2(0.5 * mv[t].x * v[t].x, -0.5 * mv[t].y * v[t].y);
                    } else {
                        if (act) psum += mv[t].x * (v[t].x * v[t].x + v[t].y * v[t].y);
                        const double2 m = cmul(v[t], mv[t]);
                        v[t] = make_double2(m.x, -m.y);
                    }
                }
            }
            wave_sync_lds();
            if (act) {
#pragma unroll
                for (int t = 0; t < 8; ++t) d[j + 8 * t] = v[t];
            }
            continue;
        }
        constexpr int PS = B == 64 ? 8 : 6;                                     // stride of a lane's outputs inside its sub-transform
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = cmul(v[t], tw[r * ((B == 64 ? j : (j < 6 ? j : 0)) + PS * t)]);      // w_F^(r k1)
        wave_sync_lds();
        if (act && (B == 64 || j < 6)) {
#pragma unroll
            for (int t = 0; t < 8; ++t) s[r * B + j + PS * t] = v[t];
        }
        wave_sync_lds();
        // combine over r: lane li takes k1 = li + LPL u, u < U (B = 48: while k1 < 48)
        double2 mv[MUL ? 8 : 1];
        if (MUL) {                                                              // requested now, used after the butterflies
            const int lq = act ? l0 + lsub : l0;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const int k1 = (kPartial && li + LPL * u >= B) ? 0 : li + LPL * u;
                    if (MUL == 5) {
                        mv[u * R + q] = mul[u * R + q];
                    } else if (MUL == 4) {
                        mv[u * R + q] = mul[(k1 + B * q) * (int)mul_stride + lq];
                    } else if (MUL == 3) {
                        const double* rs = reinterpret_cast<const double*>(mul);
                        mv[u * R + q] = make_double2(rs[(int64_t)(k1 + B * q) * mul_stride + lq],
                                                     rs[(int64_t)(k1 + B * q) * mul_stride + lq + mul_pair]);
                    } else {
                        mv[u * R + q] = mul[(int64_t)(k1 + B * q) * mul_stride + lq];
                        if (MUL == 2) mv[u * R + q].y = mul[(int64_t)(k1 + B * q) * mul_stride + lq + mul_pair].x;
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < R; ++q) v[u * R + q] = s[q * B + ((kPartial && li + LPL * u >= B) ? 0 : li + LPL * u)];
        if (R == 8) {
            dft8_inplace(v);
        } else if (R == 4) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const double2 a0 = v[4 * u], a1 = v[4 * u + 1], a2 = v[4 * u + 2], a3 = v[4 * u + 3];
                const double2 t0 = make_double2(a0.x + a2.x, a0.y + a2.y), t1 = make_double2(a0.x - a2.x, a0.y - a2.y);
                const double2 t2 = make_double2(a1.x + a3.x, a1.y + a3.y), t3 = make_double2(a1.y - a3.y, a3.x - a1.x);
                v[4 * u] = make_double2(t0.x + t2.x, t0.y + t2.y);
                v[4 * u + 1] = make_double2(t1.x + t3.x, t1.y + t3.y);
                v[4 * u + 2] = make_double2(t0.x - t2.x, t0.y - t2.y);
                v[4 * u + 3] = make_double2(t1.x - t3.x, t1.y - t3.y);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double2 a0 = v[2 * u], a1 = v[2 * u + 1];
                v[2 * u] = make_double2(a0.x + a1.x, a0.y + a1.y);
                v[2 * u + 1] = make_double2(a0.x - a1.x, a0.y - a1.y);
            }
        }
        if (MUL) {
#pragma unroll
            for (int i = 0; i < U * R; ++i) {
                const bool live = act && !(kPartial && li + LPL * (i / R) >= B);
                if (MUL >= 2) {
                    if (live) psum += mv[i].x * v[i].x * v[i].x + mv[i].y * v[i].y * v[i].y;
                    v[i] = make_double2(0.5 * mv[i].x * v[i].x, -0.5 * mv[i].y * v[i].y);
                } else {
                    if (live) psum += mv[i].x * (v[i].x * v[i].x + v[i].y * v[i].y);
                    const double2 m = cmul(v[i], mv[i]);
                    v[i] = make_double2(m.x, -m.y);
                }
            }
        }
        wave_sync_lds();
        if (act) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int q = 0; q < R; ++q)
                    if (!(kPartial && li + LPL * u >= B)) d[li + LPL * u + B * q] = v[u * R + q];
        }
    }
    __syncthreads();
    return psum;
}

// One out-of-line copy per (R, MUL) shared by every call site of a kernel: inlined four times per operator application the
// unrolled transforms put the cooperative kernel's loop body beyond the instruction cache (its speed then moved by 10-40 %
// with every unrelated code change).  Operands are passed as offsets into the kernel's dynamic LDS so that the accesses
// stay LDS instructions.
extern __shared__ double2 efgp_line_lds[];
template <int R, int MUL, int B = 64>
__device__ __noinline__ double line_fft_inwave_call(int src_off, int dst_off, int ld, int nl, int tw_off, const double2* mul,
                                                    int64_t mul_stride, int64_t mul_pair = 0) {
    return line_fft_inwave<R, MUL, B>(efgp_line_lds + src_off, efgp_line_lds + dst_off, ld, nl, efgp_line_lds + tw_off, mul, mul_stride,
                                      mul_pair);
}
// lengths the in-wave transforms cover: 64 R and (round 4) 48 R
__device__ __host__ __forceinline__ bool line_fft_fast_len(int F) {
    return F == 64 || F == 128 || F == 256 || F == 512 || F == 96 || F == 192 || F == 384;
}
// one dispatch over the line length for every multiply mode (MUL as in line_fft_inwave)
template <int MUL>
__device__ __forceinline__ double line_fft_dispatch(int F, int so, int dn, int ld, int nl, int to, const double2* mul, int64_t mul_stride,
                                                    int64_t mul_pair) {
    switch (F) {
        case 128: return line_fft_inwave_call<2, MUL>(so, dn, ld, nl, to, mul, mul_stride, mul_pair);
        case 256: return line_fft_inwave_call<4, MUL>(so, dn, ld, nl, to, mul, mul_stride, mul_pair);
        case 512: return line_fft_inwave_call<8, MUL>(so, dn, ld, nl, to, mul, mul_stride, mul_pair);
        case 96: return line_fft_inwave_call<2, MUL, 48>(so, dn, ld, nl, to, mul, mul_stride, mul_pair);
        case 192: return line_fft_inwave_call<4, MUL, 48>(so, dn, ld, nl, to, mul, mul_stride, mul_pair);
        default: return line_fft_inwave_call<8, MUL, 48>(so, dn, ld, nl, to, mul, mul_stride, mul_pair);      // 384
    }
}
// result buffer is always `dst`
__device__ __forceinline__ double2* line_fft_fast(double2* src, double2* dst, int F, int ld, int nl, const double2* tw) {
    const int so = (int)(src - efgp_line_lds), dn = (int)(dst - efgp_line_lds), to = (int)(tw - efgp_line_lds);
    if (F == 64) line_fft_inwave_call<1, 0>(so, dn, ld, nl, to, nullptr, 0);
    else line_fft_dispatch<0>(F, so, dn, ld, nl, to, nullptr, 0, 0);
    return dst;
}
// forward transform, spectrum multiply (mul[k * mul_stride + l]) and conjugation in one pass (F = 96 .. 512)
__device__ __forceinline__ double2* line_fft_fast_mul(double2* src, double2* dst, int F, int ld, int nl, const double2* tw,
                                                      const double2* mul, int64_t mul_stride, double& psum) {
    const int so = (int)(src - efgp_line_lds), dn = (int)(dst - efgp_line_lds), to = (int)(tw - efgp_line_lds);
    psum += line_fft_dispatch<1>(F, so, dn, ld, nl, to, mul, mul_stride, 0);
    return dst;
}
// the same for lines that carry two real columns (MUL = 2)
__device__ __forceinline__ double2* line_fft_fast_mul2(double2* src, double2* dst, int F, int ld, int nl, const double2* tw,
                                                       const double2* mul, int64_t mul_stride, int64_t mul_pair, double& psum) {
    const int so = (int)(src - efgp_line_lds), dn = (int)(dst - efgp_line_lds), to = (int)(tw - efgp_line_lds);
    psum += line_fft_dispatch<2>(F, so, dn, ld, nl, to, mul, mul_stride, mul_pair);
    return dst;
}
// two real columns per line, spectra resident in LDS at offset spec_off (MUL = 4)
__device__ __forceinline__ double2* line_fft_fast_mul4(double2* src, double2* dst, int F, int ld, int nl, const double2* tw,
                                                       const double2* spec_lds, int stride, double& psum) {
    const int so = (int)(src - efgp_line_lds), dn = (int)(dst - efgp_line_lds), to = (int)(tw - efgp_line_lds);
    const double2* mul = efgp_line_lds + (int)(spec_lds - efgp_line_lds);
    psum += line_fft_dispatch<4>(F, so, dn, ld, nl, to, mul, stride, 0);
    return dst;
}
// two real columns per line, spectra given as a REAL array (MUL = 3)
__device__ __forceinline__ double2* line_fft_fast_mul3(double2* src, double2* dst, int F, int ld, int nl, const double2* tw,
                                                       const double* spec, int64_t stride, int64_t pair) {
    const int so = (int)(src - efgp_line_lds), dn = (int)(dst - efgp_line_lds), to = (int)(tw - efgp_line_lds);
    const double2* mul = reinterpret_cast<const double2*>(spec);
    if (F == 64) line_fft_inwave_call<1, 3>(so, dn, ld, nl, to, mul, stride, pair);
    else if (F == 128) line_fft_inwave_call<2, 3>(so, dn, ld, nl, to, mul, stride, pair);
    else if (F == 256) line_fft_inwave_call<4, 3>(so, dn, ld, nl, to, mul, stride, pair);
    else line_fft_inwave_call<8, 3>(so, dn, ld, nl, to, mul, stride, pair);
    return dst;
}
// the (S_a, S_b) pairs line_fft_inwave<R, 2..4> would read for this thread in its single pass over nl <= 256 / (8 R) lines
template <int R>
__device__ __forceinline__ void spectrum_prefetch(const double* __restrict__ spec, int64_t stride, int64_t pair, int nl, double2 (&pre)[8]) {
    constexpr int LPL = 8 * R, U = R > 1 ? 8 / R : 1;
    const int li = threadIdx.x & (LPL - 1), lsub = threadIdx.x / LPL;
    const int lq = lsub < nl ? lsub : 0;
    if (R == 1) {
        const int j = li & 7;
#pragma unroll
        for (int t = 0; t < 8; ++t) pre[t] = make_double2(spec[(int64_t)(j + 8 * t) * stride + lq], spec[(int64_t)(j + 8 * t) * stride + lq + pair]);
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < R; ++q)
                pre[u * R + q] = make_double2(spec[(int64_t)(li + LPL * u + 64 * q) * stride + lq], spec[(int64_t)(li + LPL * u + 64 * q) * stride + lq + pair]);
    }
}
// in-wave transform for the lengths it covers, the generic Stockham stages otherwise; the result buffer is returned
__device__ __forceinline__ double2* line_fft_any(double2* A, double2* B, int F, int ld, int nl, const double2* tw) {
    if (line_fft_fast_len(F)) return line_fft_fast(A, B, F, ld, nl, tw);
    return line_fft(A, B, F, ld, nl, tw);
}

// cooperative copy of a twiddle table into LDS (visible after the caller's next barrier)
__device__ __forceinline__ void load_twiddles(double2* dst, const double2* __restrict__ src, int F) {
    for (int i = threadIdx.x; i < F; i += kLineThreads) dst[i] = src[i];
}

}  // namespace efgp
