// Device code and launch types that more than one family of the single-launch CG kernels uses: the generic, 64 x 64 and 1-D kernels
// and the Toeplitz helper kernels of cg_persistent.hip, and the Hermitian solves of cg_herm.hip.  Everything here is inline or a
// type; the one host function declared is herm_launch (cg_herm.hip), through which persistent_cg_launch reaches the Hermitian
// kernels -- no __global__ template is declared across files.
#pragma once
#include <cmath>

#include "cg_plan_host.hpp"
#include "common.hpp"
#include "toeplitz_cg.hpp"

namespace efgp {

namespace pcg {

struct Pass {            // one 1-D FFT pass over dimension `dim`
    int dim;
    int n;               // FFT length
    int nstages;
    int radix[6];
    int w1_log2;         // lines are enumerated on a power-of-two padded box (no integer division):
    int lines_log2;      //   line = item & (2^lines_log2 - 1); c1 = line & (2^w1_log2 - 1); c0 = line >> w1_log2
    // line ranges of the two other dimensions [lo, hi)
    int other[2];
    int lo[2], hi[2];
    int in_limit;        // first stage: positions >= in_limit are zero (forward), n otherwise
    int out_lo, out_hi;  // last stage: only positions in [out_lo, out_hi) are stored
    int vs_pos, vs_c0, vs_c1;   // strides of (position, other[0], other[1]) in the UNPADDED spectrum array
    int pstride, s0, s1;        // strides of the same three coordinates in the padded LDS grid
    int tw_lds;                 // offset of this pass's twiddle table in LDS (double2 units) or -1 (use tw_glob)
    const double2* tw_glob;
};

struct Geom {
    int d;
    int n[3];            // block sizes
    int F[3];            // FFT sizes
    int ld[3];           // element strides of the padded grid per dimension
    int M;
    int padded;          // elements per buffer
    int npass;           // forward passes (== d), inverse passes are derived
    Pass fwd[3];
    Pass inv[3];
    const double2* tw[3];    // twiddle table per dimension: tw[a][q] = exp(-2 pi i q / F[a])  (global memory)
    int tw_lds_off[3];       // offset (in double2) of the LDS copy of tw[a] behind the two buffers, or -1
    int tw_lds_total;        // double2 elements of LDS used by twiddle copies
    int fuse_mid;            // 1: last forward stage, spectral multiply and first inverse stage run fused in registers
};

struct Args {
    Geom g;
    const double2* ws;
    const double* diag;      // Jacobi diagonal [M] or null
    const double* diag_scale;   // when diag is null and this is not: diagonal = (*diag_scale) * |ws|^2 + sigmasq (device scalar)
    int b_times_ws;          // right-hand side is ws .* b (the fit's D F*y, efgpnd.py:792)
    int zero_x0;             // x0 = 0: x is output only and the initial operator application is skipped (A 0 = 0)
    const double2* x0;       // start vectors (read once, before x is written; normally x itself: in place)
    const double2* vhat;     // [prod F] (unpadded row-major), already divided by prod F
    double sigmasq;
    int variant;
    double tol;
    int early_stop;
    int batched;
    int max_iter;
    const double2* b;
    double2* x;              // in: x0, out: solution
    int* iters;              // per row
    double* hist;            // diagnostic: row 0's |r_i| / |b| per iteration (efgp_cg_record_history) or null
    int hist_cap;
    // Lanczos mode (efgp_lanczos; reference: logdet_slq, efgpnd.py:1716-1738): lz_steps > 0 runs that many three-term
    // recurrence steps on A (variant as given) from q_0 = b / |b| instead of the CG loop; row r's alpha_k, beta_k go to
    // lz_alpha / lz_beta [r * lz_steps + k], |b|^2 to lz_norm2[r], the number of steps taken to iters[r]
    int lz_steps;
    double* lz_alpha;
    double* lz_beta;
    double* lz_norm2;
    // fused mean solve (cg_herm48_kernel<0, true>, efgp_cg_solve_mean_fused): ws evaluated in the kernel from the built-in kernel's
    // parameters (spectral_weights.hpp) and written to ws_out; the 48 x 48 spectrum made from the Toeplitz vector vsrc (L0 x L1)
    // in the prologue and written to vhat_out
    int wk_kind, wk_mtot;
    double wk_nu, wk_ell, wk_c0, wk_h;
    double2* ws_out;
    const double2* vsrc;
    int vL0, vL1;
    double2* vhat_out;
#ifdef EFGP_CG_STAMPS
    long long* stamps;       // diagnostic build only: cycles per phase class, accumulated by block 0
#endif
};

#ifdef EFGP_CG_STAMPS
#define EFGP_STAMP(slot)                                                     \
    do {                                                                     \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                           \
            const long long now__ = (long long)__builtin_readcyclecounter(); \
            a.stamps[slot] += now__ - stamp_prev;                            \
            stamp_prev = now__;                                              \
        }                                                                    \
    } while (0)
// the same from thread `who` of block 0, for a phase that thread 0's wave does not carry (cg_herm48_pairs_kernel), and a restart
// of the thread's clock behind a wait that another thread accounts for
#define EFGP_STAMP_BY(slot, who)                                             \
    do {                                                                     \
        if (blockIdx.x == 0 && threadIdx.x == (who)) {                       \
            const long long now__ = (long long)__builtin_readcyclecounter(); \
            a.stamps[slot] += now__ - stamp_prev;                            \
            stamp_prev = now__;                                              \
        }                                                                    \
    } while (0)
#define EFGP_STAMP_RESTART(who)                                                                                  \
    do {                                                                                                         \
        if (blockIdx.x == 0 && threadIdx.x == (who)) stamp_prev = (long long)__builtin_readcyclecounter();       \
    } while (0)
#else
#define EFGP_STAMP(slot) \
    do {                 \
    } while (0)
#define EFGP_STAMP_BY(slot, who) \
    do {                         \
    } while (0)
#define EFGP_STAMP_RESTART(who) \
    do {                        \
    } while (0)
#endif

__device__ __forceinline__ double2 cmulp(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// multiply by -i (forward) : (x, y) -> (y, -x)
__device__ __forceinline__ double2 mul_mi(double2 a) { return make_double2(a.y, -a.x); }

template <int R>
__device__ __forceinline__ void dft_fwd(double2 (&v)[R]);

template <>
__device__ __forceinline__ void dft_fwd<2>(double2 (&v)[2]) {
    double2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
}

template <>
__device__ __forceinline__ void dft_fwd<4>(double2 (&v)[4]) {
    double2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
    double2 t2 = cadd(v[1], v[3]), t3 = mul_mi(csub(v[1], v[3]));
    v[0] = cadd(t0, t2);
    v[1] = cadd(t1, t3);
    v[2] = csub(t0, t2);
    v[3] = csub(t1, t3);
}

template <>
__device__ __forceinline__ void dft_fwd<8>(double2 (&v)[8]) {
    // two interleaved DFT4 (even / odd), then combine with w8^m
    double2 e[4] = {v[0], v[2], v[4], v[6]};
    double2 o[4] = {v[1], v[3], v[5], v[7]};
    dft_fwd<4>(e);
    dft_fwd<4>(o);
    const double h = 0.70710678118654752440;
    // o[m] *= exp(-2 pi i m / 8)
    double2 o1 = make_double2(h * (o[1].x + o[1].y), h * (o[1].y - o[1].x));
    double2 o2 = mul_mi(o[2]);
    double2 o3 = make_double2(h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y));
    v[0] = cadd(e[0], o[0]);
    v[4] = csub(e[0], o[0]);
    v[1] = cadd(e[1], o1);
    v[5] = csub(e[1], o1);
    v[2] = cadd(e[2], o2);
    v[6] = csub(e[2], o2);
    v[3] = cadd(e[3], o3);
    v[7] = csub(e[3], o3);
}

// wave-level sum with DPP moves (VALU only; the LDS pipe stays free for the FFT stages).  gfx9 row_shr /
// row_bcast controls; the value ends up in lane 63 and is broadcast through an SGPR.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xF, true);
    return __hiloint2double(hi, lo);
}
#define EFGP_DPP_ADD(v, ctrl, rmask) v += dpp_move<ctrl, rmask>(v)
__device__ __forceinline__ double wave_sum(double v) {
    EFGP_DPP_ADD(v, 0x111, 0xF);   // row_shr:1
    EFGP_DPP_ADD(v, 0x112, 0xF);   // row_shr:2
    EFGP_DPP_ADD(v, 0x114, 0xF);   // row_shr:4
    EFGP_DPP_ADD(v, 0x118, 0xF);   // row_shr:8   -> lane 15 of every 16-lane row holds the row sum
    EFGP_DPP_ADD(v, 0x142, 0xA);   // row_bcast:15 into rows 1 and 3
    EFGP_DPP_ADD(v, 0x143, 0xC);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave sum
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// Jacobi diagonal entry t: explicit array, or scale * |ws_t|^2 + sigmasq with the two roundings of the
// reference's torch expression (efgpnd.py:795-799), or 1 (no preconditioner)
__device__ __forceinline__ double jacobi_entry(const Args& a, double2 w, int t) {
    if (a.diag) return a.diag[t];
    if (a.diag_scale) return __dadd_rn(__dmul_rn(*a.diag_scale, __dadd_rn(__dmul_rn(w.x, w.x), __dmul_rn(w.y, w.y))), a.sigmasq);
    return 1.0;
}

// load / store / twiddle of the eight values of a radix-8 butterfly (the 64 x 64 kernels' stages; the 48 x 48 lines' radix-8 halves)
namespace s64 {
constexpr int F = 64, LD = 65, BUF = F * LD;

__device__ __forceinline__ double2 conjd(double2 a) { return make_double2(a.x, -a.y); }

// v[t] = src[t * STRIDE] (t < 8), entries with t >= nvalid are zero
template <int STRIDE>
__device__ __forceinline__ void load8(const double2* __restrict__ src, int nvalid, double2 (&v)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = t < nvalid ? src[t * STRIDE] : make_double2(0.0, 0.0);
}
template <int STRIDE>
__device__ __forceinline__ void load8_all(const double2* __restrict__ src, double2 (&v)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = src[t * STRIDE];
}
template <int STRIDE>
__device__ __forceinline__ void store8_all(double2* __restrict__ dst, const double2 (&v)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) dst[t * STRIDE] = v[t];
}
__device__ __forceinline__ void twiddle8(double2 (&v)[8], const double2 (&w)[7]) {
#pragma unroll
    for (int t = 1; t < 8; ++t) v[t] = cmulp(v[t], w[t - 1]);
}
__device__ __forceinline__ void conj8(double2 (&v)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t].y = -v[t].y;
}
}  // namespace s64

// Line transforms of the 48 x 48 grid (layouts: cg_herm.hip, in front of namespace h48), for the spectrum kernel of cg_persistent.hip
// and the fused prologue of the 48 x 48 solves
namespace h48 {
constexpr int F = 48;                    // grid
constexpr int LX = 72;                   // row lanes' exchange scratch per line: [writer][value], writer pitch 9

// forward DFT-6 in natural order: even / odd split into two DFT-3
__device__ __forceinline__ void dft3(double2 b0, double2 b1, double2 b2, double2& x0, double2& x1, double2& x2) {
    const double s = 0.86602540378443864676;
    const double2 sm = cadd(b1, b2), df = csub(b1, b2);
    x0 = cadd(b0, sm);
    const double2 m = make_double2(fma(-0.5, sm.x, b0.x), fma(-0.5, sm.y, b0.y));
    x1 = make_double2(fma(s, df.y, m.x), fma(-s, df.x, m.y));      // m - i s (b1 - b2)
    x2 = make_double2(fma(-s, df.y, m.x), fma(s, df.x, m.y));
}
__device__ __forceinline__ void dft6(double2 (&v)[6]) {
    const double s = 0.86602540378443864676;
    double2 e0, e1, e2, o0, o1, o2;
    dft3(v[0], v[2], v[4], e0, e1, e2);
    dft3(v[1], v[3], v[5], o0, o1, o2);
    const double2 w1 = make_double2(fma(s, o1.y, 0.5 * o1.x), fma(-s, o1.x, 0.5 * o1.y));        // w6   o1, w6 = (1/2, -s)
    const double2 w2 = make_double2(fma(s, o2.y, -0.5 * o2.x), fma(-s, o2.x, -0.5 * o2.y));      // w6^2 o2
    v[0] = cadd(e0, o0);
    v[3] = csub(e0, o0);
    v[1] = cadd(e1, w1);
    v[4] = csub(e1, w1);
    v[2] = cadd(e2, w2);
    v[5] = csub(e2, w2);
}
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// vhat[f0][f1] = factor * sum_l v[l] w48^(f0 l0 + f1 l1), natural order: the spectrum of the Toeplitz vector on this grid.  Lines in
// the "8x6" layout (radix 6 on eight lanes, radix 8 on six), rows then columns, NT / 8 line slots, as many passes per dimension as
// 48 lines need (512 threads: one; 256: two -- the same arithmetic per line either way).  LDS: [48][49] grid + [NT / 8][72] scratch.
// KEEP: the result also stays in the grid, lds2[f0 * 49 + f1] (the fused mean solve loads its spectrum registers from there).
template <int NT, bool KEEP>
__device__ __forceinline__ void vhat48_lines(const double2* __restrict__ v, int L0, int L1, double factor, double2* __restrict__ vhat,
                                             double2* lds2) {
    constexpr int LD = 49, SLOTS = NT / 8, PASSES = (F + SLOTS - 1) / SLOTS, PER = (F * F + NT - 1) / NT;
    double2* const buf = lds2;                       // [48][LD]
    double2* const scr = lds2 + F * LD;              // [SLOTS lines][writer 9 j + value]
    const int tid = threadIdx.x;
    // every load of v in flight at once (one L2 round trip, not PER of them: 9 on 256 threads), the twiddles computed meanwhile
    double2 xs[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int t = tid + k * NT, i0 = t / F, i1 = t - i0 * F;
        xs[k] = (t < F * F && i0 < L0 && i1 < L1) ? v[i0 * L1 + i1] : make_double2(0.0, 0.0);
    }
    const int slot = tid >> 3, j = tid & 7;
    double2 tw[5];
#pragma unroll
    for (int t = 1; t < 6; ++t) {
        double sn, cs;
        sincospi(-(double)(j * t) / 24.0, &sn, &cs);      // exp(-2 pi i j t / 48)
        tw[t - 1] = make_double2(cs, sn);
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int t = tid + k * NT, i0 = t / F, i1 = t - i0 * F;
        double2 x = xs[k];
        if (i0 < L0 && i1 < L1) {
            x.x *= factor;
            x.y *= factor;
        }
        if (t < F * F) buf[i0 * LD + i1] = x;
    }
    double2* const wr = scr + slot * LX + 9 * j;
    const double2* const rd = scr + slot * LX + j;
    double2 u6[6], x8[8];
    __syncthreads();
    // dimension 1 (contiguous): line = row
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int line = slot + ps * SLOTS;
        const bool act = line < F;
#pragma unroll
        for (int t = 0; t < 6; ++t) u6[t] = act ? buf[line * LD + j + 8 * t] : make_double2(0.0, 0.0);
        dft6(u6);
#pragma unroll
        for (int t = 1; t < 6; ++t) u6[t] = cmulp(u6[t], tw[t - 1]);
        wave_sync();
#pragma unroll
        for (int t = 0; t < 6; ++t) wr[t] = u6[t];
        wave_sync();
        s64::load8_all<9>(rd, x8);
        dft_fwd<8>(x8);
        if (act && j < 6) {
#pragma unroll
            for (int t = 0; t < 8; ++t) buf[line * LD + j + 6 * t] = x8[t];
        }
    }
    __syncthreads();
    // dimension 0: line = column (a line reads and rewrites its own column only)
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int line = slot + ps * SLOTS;
        const bool act = line < F;
#pragma unroll
        for (int t = 0; t < 6; ++t) u6[t] = act ? buf[(j + 8 * t) * LD + line] : make_double2(0.0, 0.0);
        dft6(u6);
#pragma unroll
        for (int t = 1; t < 6; ++t) u6[t] = cmulp(u6[t], tw[t - 1]);
        wave_sync();
#pragma unroll
        for (int t = 0; t < 6; ++t) wr[t] = u6[t];
        wave_sync();
        s64::load8_all<9>(rd, x8);
        dft_fwd<8>(x8);
        if (act && j < 6) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                vhat[(j + 6 * t) * F + line] = x8[t];
                if (KEEP) buf[(j + 6 * t) * LD + line] = x8[t];
            }
        }
    }
}
}  // namespace h48

// kernel, workgroup size and dynamic LDS of a pick (one workgroup per system)
struct PickLaunch {
    void (*kernel)(Args);
    int threads;
    size_t lds;
    const char* what;
};
// the Hermitian picks (fused48, herm48, herm64), cg_herm.hip; for the 48 x 48 ones `a` gets the operator's second spectrum and
// twiddles, or what the fused mean solve makes itself
PickLaunch herm_launch(const PersistentChoice& c, int variant, const Herm48Operands* h48, const MeanFusedOperands* fuse, Args& a);

}  // namespace pcg

}  // namespace efgp
