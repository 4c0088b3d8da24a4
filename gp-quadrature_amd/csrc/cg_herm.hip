// The Hermitian single-launch CG solves: cg_herm64_kernel (64 x 64 grid), cg_herm48_kernel (48 x 48 grid, 256 threads) and
// cg_herm48_pairs_kernel (48 x 48, eight waves: the default of a single system).  persistent_cg_launch (cg_persistent.hip) reaches
// them through herm_launch at the end of this file.
#include <cstdlib>
#include <type_traits>

#include "cg_persistent_dev.hpp"
#include "spectral_weights.hpp"

namespace efgp {

namespace pcg {

// ------------------------------------------------------------------------------------------------
// Hermitian specialisation of the 64 x 64 solve (the fit's mean system, efgpnd.py:786-814).
//
// The right-hand side D F*y of a REAL y, the Toeplitz vector of real weights and the symmetric real ws make every CG
// vector the coefficient array of a real function: u[-k] = conj u[k] on the centred modes k in [-h, h]^2, h = (n-1)/2.
// The operator then is   coefficients -> real function on the 64 x 64 torus -> times a REAL spectrum -> coefficients,
// and real transforms cost half:
//   * only the rows k0 = 0..h of a vector are stored and transformed (A: h + 1 row lines instead of n),
//   * two real columns f1 = q, q + 32 ride through ONE complex column transform as real and imaginary part
//     (B/C: 32 column lines instead of 64; the spectrum multiply is two real multiplies),
//   * the rows of the result for k0 = 0..h come from the packed columns at +k0 and -k0 (D: h + 1 row lines).
// 88 line transforms per operator instead of 174.  Every line transform runs inside ONE wave (8 adjacent lanes x 8
// points, radix 8 x 8, one exchange through wave-private LDS), so an iteration has 4 workgroup barriers: A | B C | D |
// <p,Ap> | <r,r>,<r,z>.  The CG vectors live in the registers of the row lanes in exactly the positions the first
// radix-8 stage of A consumes and the last stage of D produces (position j + 8t of lane j, t in {0,1,6,7}: modes k1 and
// k1 - 64), so neither the load of ws.*p nor the crop touches LDS.  Dot products weigh the rows k0 > 0 twice.
// Same recurrences, stopping rule and preconditioner as the kernels above; the arithmetic differs from them (and from
// the reference's complex FFTs) by rounding only: the spectrum's rotated imaginary part (|.| ~ 1e-16 relative) and the
// anti-Hermitian rounding noise of the inputs are dropped.
// ------------------------------------------------------------------------------------------------
namespace h64 {
constexpr int kThreadsH = 256, kWavesH = kThreadsH / 64;
constexpr int LDR = 72;                  // pitch of the G rows and of the row lanes' exchange scratch (8 mod 16: conflict free)
constexpr int LT = 40;                   // pitch of the T rows (32 packed columns)
constexpr int LQ = 82;                   // column lanes' exchange scratch per line (2 mod 16)
constexpr int G_ELEMS = 16 * LDR, T_ELEMS = 32 * LT, Q_ELEMS = kWavesH * 8 * LQ;
constexpr int kLdsElems = G_ELEMS + T_ELEMS + Q_ELEMS;     // 80.9 KB

// DFT-8 of (a0, a1, 0, 0, 0, 0, a6, a7): the zero-padded first stage (modes 0..15 and -16..-1 of a 64-point line)
// its second half: from the first butterflies e = a0 + i^m a6, o = a1 + i^m a7 (m = 0..3) to the outputs
__device__ __forceinline__ void dft8_in4_tail(double2 e0, double2 e1, double2 e2, double2 e3, double2 o0, double2 o1r, double2 o2r,
                                              double2 o3r, double2 (&v)[8]) {
    const double hh = 0.70710678118654752440;
    const double2 o1 = make_double2(hh * (o1r.x + o1r.y), hh * (o1r.y - o1r.x));
    const double2 o2 = mul_mi(o2r);
    const double2 o3 = make_double2(hh * (o3r.y - o3r.x), -hh * (o3r.x + o3r.y));
    v[0] = cadd(e0, o0);
    v[4] = csub(e0, o0);
    v[1] = cadd(e1, o1);
    v[5] = csub(e1, o1);
    v[2] = cadd(e2, o2);
    v[6] = csub(e2, o2);
    v[3] = cadd(e3, o3);
    v[7] = csub(e3, o3);
}
__device__ __forceinline__ void dft8_in4(double2 a0, double2 a1, double2 a6, double2 a7, double2 (&v)[8]) {
    const double2 ia6 = make_double2(-a6.y, a6.x), ia7 = make_double2(-a7.y, a7.x);
    dft8_in4_tail(cadd(a0, a6), cadd(a0, ia6), csub(a0, a6), csub(a0, ia6), cadd(a1, a7), cadd(a1, ia7), csub(a1, a7), csub(a1, ia7), v);
}

// DFT-8 of which only the outputs 0, 1, 6, 7 are wanted (positions 0..15 and 48..63 of a cropped 64-point line)
__device__ __forceinline__ void dft8_out4(double2 (&v)[8]) {
    double2 e[4] = {v[0], v[2], v[4], v[6]};
    double2 o[4] = {v[1], v[3], v[5], v[7]};
    dft_fwd<4>(e);
    dft_fwd<4>(o);
    const double hh = 0.70710678118654752440;
    const double2 o1 = make_double2(hh * (o[1].x + o[1].y), hh * (o[1].y - o[1].x));
    const double2 o2 = mul_mi(o[2]);
    const double2 o3 = make_double2(hh * (o[3].y - o[3].x), -hh * (o[3].x + o[3].y));
    v[0] = cadd(e[0], o[0]);
    v[1] = cadd(e[1], o1);
    v[6] = csub(e[2], o2);
    v[7] = csub(e[3], o3);
}

// a / b from the correctly rounded reciprocal rb = 1 / b: one residual step (Markstein) -- the quotient the hardware division
// sequence returns for operands in the normal range, in 3 instructions instead of ~30
__device__ __forceinline__ double div_rcp(double a_, double b_, double rb) {
    const double q0 = a_ * rb;
    return fma(fma(-q0, b_, a_), rb, q0);
}

// second half of a 64-point line transform inside a wave: the 8 lanes of a line swap their first-stage outputs through
// `wr` (lane's own 8 slots, stride 1) / `rd` (stride 9), twiddle, second radix-8 stage.  v[t] = X[j + 8 t] on return.
template <bool OUT4 = false>
__device__ __forceinline__ void exchange_stage2(double2 (&v)[8], double2* __restrict__ wr, const double2* __restrict__ rd,
                                                const double2 (&tw)[7]) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    s64::store8_all<1>(wr, v);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    s64::load8_all<9>(rd, v);
    s64::twiddle8(v, tw);
    if (OUT4) dft8_out4(v);
    else dft_fwd<8>(v);
}

__device__ __forceinline__ double block_sum_h(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double* r1 = red + 2 * kWavesH;
    if (lane == 0) r1[wid] = v;
    __syncthreads();
    return (r1[0] + r1[1]) + (r1[2] + r1[3]);
}
__device__ __forceinline__ void block_sum_pair_h(double& u, double& v, double* red) {
    u = wave_sum(u);
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        red[wid] = u;
        red[kWavesH + wid] = v;
    }
    __syncthreads();
    u = (red[0] + red[1]) + (red[2] + red[3]);
    v = (red[kWavesH] + red[kWavesH + 1]) + (red[kWavesH + 2] + red[kWavesH + 3]);
}
}  // namespace h64

// ------------------------------------------------------------------------------------------------
// The row lanes' CG bookkeeping, ONE copy for cg_herm64_kernel and cg_herm48_pairs_kernel: what a lane that holds modes keeps and does outside the
// operator application -- slot set-up, right-hand side and first residual, refusal, the x / r / z update, beta and p, write-out --
// and the norm test of the wave that has the time for it.  The kernels keep what differs between them: apply_A, the reductions
// (block sums over four waves, or wave sums of the two row waves through red[]) and where alpha comes from (<p,Ap> summed over the
// modes, or formed inside D).  The members take and return the lane's SHARES of the inner products; the caller sums them.
// ------------------------------------------------------------------------------------------------
namespace hrow {
using h64::div_rcp;
constexpr int KS = 4;                    // vector slots of a row lane

// a Jacobi diagonal is given (as an array, or as the scalar it is made from).  ONE definition for RowLanes::setup and for the host's
// choice of cg_herm48_pairs_kernel's PRECOND instantiation (herm_launch): the two must not part
__host__ __device__ __forceinline__ bool has_precond(const Args& a) { return a.diag != nullptr || a.diag_scale != nullptr; }

// the sums over all modes that decide a refusal.  asym: |b[k] - conj b[-k]|^2, against <b,b> (rounding leaves ~1e-32 |b|^2);
// ws_bad > 0: ws is not real and even
__device__ __forceinline__ bool refused(double asym, double bb, double ws_bad) { return !(asym <= 1e-16 * bb) || ws_bad != 0.0; }

// Vector slots of a row lane: positions j + STRIDE t of its line, t in {0, 1, 6, 7} <-> k1 = j, j + STRIDE, j - 2 STRIDE, j - STRIDE
// (STRIDE 8: the 64-point lines, 6: the 48-point lines) of the row k0 >= 0; the modes -k are the conjugates and are not stored.
// What a row lane reads from memory before its first residual, issued at kernel entry (cg_herm48_pairs_kernel, round 10): the round
// trips run under the prologue instead of standing, one behind the other, between the prologue and the first iteration.  The slot
// arithmetic is RowLanes::setup's; a lane or slot without a mode loads nothing.
template <int STRIDE>
struct EarlyLoads {
    double2 bv[KS], bm[KS];              // b at the mode and at its mirror
    double2 x0[KS], w[KS], wm[KS];       // !FUSED: the start vector (warm start only), ws at the mode and at its mirror
    double dgv[KS], dscale;              // the Jacobi diagonal's entry, or the scalar it is made from

    template <bool FUSED>
    __device__ __forceinline__ void issue(const Args& a, bool role, int k0, int j) {
        const int n = a.g.n[0], h = (n - 1) / 2, M = a.g.M;
        const int64_t base = (int64_t)blockIdx.x * M;
        dscale = (role && !a.diag && a.diag_scale) ? *a.diag_scale : 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k1 = s == 0 ? j : (s == 1 ? j + STRIDE : (s == 2 ? j - 2 * STRIDE : j - STRIDE));
            const bool ok = role && k0 <= h && k1 <= h && -k1 <= h;
            const int idx = ok ? (k0 + h) * n + (k1 + h) : 0;
            const double2 zero = make_double2(0.0, 0.0);
            bv[s] = ok ? a.b[base + idx] : zero;
            bm[s] = ok ? a.b[base + (M - 1 - idx)] : zero;
            dgv[s] = (ok && a.diag) ? a.diag[idx] : 0.0;
            x0[s] = (ok && !FUSED && !a.zero_x0) ? a.x0[base + idx] : zero;
            w[s] = (ok && !FUSED) ? a.ws[idx] : zero;
            wm[s] = (ok && !FUSED) ? a.ws[M - 1 - idx] : zero;
        }
    }
    // jacobi_entry from what was loaded: the same two roundings
    __device__ __forceinline__ double jacobi(const Args& a, double2 wv, int s) const {
        if (a.diag) return dgv[s];
        if (a.diag_scale) return __dadd_rn(__dmul_rn(dscale, __dadd_rn(__dmul_rn(wv.x, wv.x), __dmul_rn(wv.y, wv.y))), a.sigmasq);
        return 1.0;
    }
};

template <int STRIDE>
struct RowLanes {
    double2 xv[KS], rv[KS], pv[KS];
    double wsr[KS], dg[KS], rdg[KS];     // ws is real here (checked in set-up): ws * u costs two multiplies
    bool ok[KS];                         // the slot holds a mode of the block
    int idx[KS];
    int64_t base;                        // of this workgroup's system in b, x0 and x
    int M, k0;
    bool precond;
    double wgt;                          // dot products weigh the rows k0 > 0 twice
    double ws_bad;                       // the lane's share; > 0: ws is not real and even

    // role: the lane may hold modes (a row lane; on the 48-point lines one with j < 6).  FUSED: the fit's cold-start mean solve, ws
    // evaluated here from the built-in kernel's parameters and written out for later users.
    // EARLY: x0, ws and the diagonal come from `e` (EarlyLoads::issue with the same role, k0_, j) instead of from memory.
    template <bool FUSED, bool EARLY = false>
    __device__ __forceinline__ void setup(const Args& a, bool role, int k0_, int j, const EarlyLoads<STRIDE>* e = nullptr) {
        const int n = a.g.n[0], h = (n - 1) / 2;
        M = a.g.M;
        k0 = k0_;
        base = (int64_t)blockIdx.x * M;
        precond = has_precond(a);
        wgt = k0 == 0 ? 1.0 : 2.0;
        ws_bad = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k1 = s == 0 ? j : (s == 1 ? j + STRIDE : (s == 2 ? j - 2 * STRIDE : j - STRIDE));
            ok[s] = role && k0 <= h && k1 <= h && -k1 <= h;
            idx[s] = ok[s] ? (k0 + h) * n + (k1 + h) : 0;
            double ws_im = 0.0;
            if (ok[s] && FUSED) {
                // ws = sqrt(S h^d) is real and even by construction: node idx and its mirror M - 1 - idx get the same value
                xv[s] = make_double2(0.0, 0.0);
                const double2 w = make_double2(spectral_weight_at(a.wk_kind, a.g.d, a.wk_nu, a.wk_ell, a.wk_c0, a.wk_h, a.wk_mtot, idx[s]), 0.0);
                a.ws_out[idx[s]] = w;
                a.ws_out[M - 1 - idx[s]] = w;
                wsr[s] = w.x;
                if constexpr (EARLY) dg[s] = e->jacobi(a, w, s);
                else dg[s] = jacobi_entry(a, w, idx[s]);
            } else if (ok[s]) {
                if constexpr (EARLY) xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : e->x0[s];
                else xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x0[base + idx[s]];
                double2 w, wm;
                if constexpr (EARLY) {
                    w = e->w[s];
                    wm = e->wm[s];
                } else {
                    w = a.ws[idx[s]];
                    wm = a.ws[M - 1 - idx[s]];
                }
                wsr[s] = w.x;
                ws_im = w.y * w.y + (w.x - wm.x) * (w.x - wm.x) + wm.y * wm.y;
                if constexpr (EARLY) dg[s] = e->jacobi(a, w, s);
                else dg[s] = jacobi_entry(a, w, idx[s]);
            } else {
                xv[s] = make_double2(0.0, 0.0);
                wsr[s] = 0.0;
                dg[s] = 1.0;
            }
            ws_bad += ws_im;
            rdg[s] = 1.0 / dg[s];
            rv[s] = pv[s] = make_double2(0.0, 0.0);
        }
    }

    // right-hand side, first residual r = b - A x0 (Ax: A x0, zeros for a cold start) and p = z; the lane's shares of <r,z>, <b,b>
    // (weighted) and of asym.  One uniform branch on the preconditioner around the whole block, here and in step(): with the choice
    // made per slot (precond ? r / diag : r) the compiler turns it into selects -- the quotients are then formed also when there is
    // no diagonal, and 16 v_cndmask sit on the row waves' chain (profiles/cg_herm_refactor_device_code.txt)
    // EARLY: b and its mirror come from `e`.
    template <bool EARLY = false>
    __device__ __forceinline__ void start(const Args& a, const double2 (&Ax)[KS], double& rz, double& bb, double& asym,
                                          const EarlyLoads<STRIDE>* e = nullptr) {
        if (precond) start_<true, EARLY>(a, Ax, rz, bb, asym, e);
        else start_<false, EARLY>(a, Ax, rz, bb, asym, e);
    }
    template <bool PRECOND, bool EARLY>
    __device__ __forceinline__ void start_(const Args& a, const double2 (&Ax)[KS], double& rz, double& bb, double& asym,
                                           const EarlyLoads<STRIDE>* e) {
        rz = bb = asym = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (ok[s]) {
                double2 bv, bm;
                if constexpr (EARLY) {
                    bv = e->bv[s];
                    bm = e->bm[s];
                } else {
                    bv = a.b[base + idx[s]];
                    bm = a.b[base + (M - 1 - idx[s])];                     // mode -k: must be the conjugate
                }
                if (a.b_times_ws) {
                    bv = make_double2(wsr[s] * bv.x, wsr[s] * bv.y);
                    bm = make_double2(wsr[s] * bm.x, wsr[s] * bm.y);
                }
                asym += (bv.x - bm.x) * (bv.x - bm.x) + (bv.y + bm.y) * (bv.y + bm.y);
                rv[s] = csub(bv, Ax[s]);
                pv[s] = PRECOND ? make_double2(div_rcp(rv[s].x, dg[s], rdg[s]), div_rcp(rv[s].y, dg[s], rdg[s])) : rv[s];
                rz += rv[s].x * pv[s].x + rv[s].y * pv[s].y;
                bb += bv.x * bv.x + bv.y * bv.y;
            }
        }
        rz *= wgt;
        bb *= wgt;
    }

    // not the coefficients of a real function, or a ws that is not real and even (refused() of the sums): refuse loudly instead of
    // solving another system -- a NaN solution and -2 iterations
    __device__ __forceinline__ void refuse(const Args& a) const {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (ok[s]) {
                a.x[base + idx[s]] = make_double2(__builtin_nan(""), __builtin_nan(""));
                a.x[base + (M - 1 - idx[s])] = make_double2(__builtin_nan(""), __builtin_nan(""));
            }
        }
        if (threadIdx.x == 0) a.iters[blockIdx.x] = -2;
    }

    // the lane's share of <p, A p>, summed over the modes
    __device__ __forceinline__ double dot_p(const double2 (&Ap)[KS]) const {
        double pAp = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) pAp += pv[s].x * Ap[s].x + pv[s].y * Ap[s].y;
        return pAp * wgt;
    }

    // x += alpha p, r -= alpha A p, z = r / diag (Jacobi) or r; the lane's shares of <r,r> and <r,z>
    // !X_UPDATE: x is left as it is; the caller owes it update_x(alpha, p) with this alpha and this p (nothing reads x before write-out)
    template <bool X_UPDATE = true>
    __device__ __forceinline__ void step(double alpha, const double2 (&Ap)[KS], double2 (&zv)[KS], double& rr, double& rzn) {
        if (precond) step_<true, X_UPDATE>(alpha, Ap, zv, rr, rzn);
        else step_<false, X_UPDATE>(alpha, Ap, zv, rr, rzn);
    }
    __device__ __forceinline__ void update_x(double alpha, const double2 (&p)[KS]) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xv[s].x += alpha * p[s].x;
            xv[s].y += alpha * p[s].y;
        }
    }
    template <bool PRECOND, bool X_UPDATE>
    __device__ __forceinline__ void step_(double alpha, const double2 (&Ap)[KS], double2 (&zv)[KS], double& rr, double& rzn) {
        rr = rzn = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if constexpr (X_UPDATE) {
                xv[s].x += alpha * pv[s].x;
                xv[s].y += alpha * pv[s].y;
            }
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = PRECOND ? make_double2(div_rcp(rv[s].x, dg[s], rdg[s]), div_rcp(rv[s].y, dg[s], rdg[s])) : rv[s];
            rr += rv[s].x * rv[s].x + rv[s].y * rv[s].y;
            rzn += rv[s].x * zv[s].x + rv[s].y * zv[s].y;
        }
        rr *= wgt;
        rzn *= wgt;
    }

    // beta = <r,z>_new / (<r,z> + 1e-16) from the reciprocal rcp_rz that the norm test's wave left, p = z + beta p.
    // cg.py:132 / 229: the test sits before (single) or after (batched) this update; p is not an output
    __device__ __forceinline__ void new_direction(const double2 (&zv)[KS], double rzn, double& rz, double rcp_rz) {
        const double beta = div_rcp(rzn, rz + 1e-16, rcp_rz);
#pragma unroll
        for (int s = 0; s < KS; ++s) pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
        rz = rzn;
    }
    // new_direction with the new p written to p_next while p_cur stays what it was: a caller that alternates two arrays (a loop body
    // of two iterations) keeps the last direction for a deferred x update without copying it.  The same operations.
    __device__ __forceinline__ void new_direction_to(const double2 (&zv)[KS], double rzn, double& rz, double rcp_rz,
                                                     const double2 (&p_cur)[KS], double2 (&p_next)[KS]) const {
        const double beta = div_rcp(rzn, rz + 1e-16, rcp_rz);
#pragma unroll
        for (int s = 0; s < KS; ++s) p_next[s] = make_double2(zv[s].x + beta * p_cur[s].x, zv[s].y + beta * p_cur[s].y);
        rz = rzn;
    }

    // the solution with its mirror, and the iteration count
    __device__ __forceinline__ void write_out(const Args& a, int it) const {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (ok[s]) {
                a.x[base + idx[s]] = xv[s];
                if (k0 > 0) a.x[base + (M - 1 - idx[s])] = s64::conjd(xv[s]);     // mode -k
            }
        }
        if (threadIdx.x == 0) a.iters[blockIdx.x] = it;
    }
};

// The norm test of a completed iteration and the reciprocal for the next beta: neither is on the row waves' dependent chain, so a wave
// that is idle during A takes them (a sqrt and two divisions).  Its decision is read behind the first barrier of the next operator
// application.
struct NormTest {
    double den_eps, rcp_den;             // |b| + 1e-16 (b = 0: 1 + 1e-16) and its reciprocal
    __device__ __forceinline__ explicit NormTest(double bb) {
        const double bn = sqrt(bb);
        const double den = bn > 0.0 ? bn : 1.0;
        den_eps = den + 1e-16;
        rcp_den = 1.0 / den_eps;
    }
    // every lane of the wave calls; lane 0 publishes.  rr, rzn: <r,r> and <r,z> of iteration `it`, summed over the modes
    __device__ __forceinline__ void publish(const Args& a, double rr, double rzn, int it, int lane, double* s_rcp, int* s_stop) const {
        const double ratio = div_rcp(sqrt(rr), den_eps, rcp_den);
        const bool conv = a.early_stop && ((ratio < a.tol) || (a.batched && sqrt(rr) < 1e-12));
        if (lane == 0) {
            if (a.hist && blockIdx.x == 0 && it <= a.hist_cap) a.hist[it - 1] = ratio;
            *s_stop = conv ? 1 : 0;
            *s_rcp = 1.0 / (rzn + 1e-16);
        }
    }
};
}  // namespace hrow

template <int VARIANT>
__global__ __launch_bounds__(h64::kThreadsH) void cg_herm64_kernel(Args a) {
    using namespace h64;
    constexpr int F = 64;
    using hrow::KS;
    extern __shared__ double2 lds2[];
    __shared__ double red[4 * kWavesH];
    __shared__ double s_rcp;             // 1 / (<r,z> + 1e-16) for the next beta, computed by an idle wave during A
    __shared__ int s_stop;               // convergence decision of the last completed iteration, taken by an idle wave during A
    double2* const Gb = lds2;                    // G[k0][f1], k0 = 0..15 (rows beyond h are zero)
    double2* const Tb = lds2 + G_ELEMS;          // conj T[row(p)][q]: rows p = 0..15 and 48..63 (stored at p - 32)
    double2* const Qb = Tb + T_ELEMS;            // exchange scratch: column lines (B/C), aliased by the row lines (A, D)
    const int n = a.g.n[0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // row role (waves 0, 1): lane = k0 * 8 + j; column role (all waves): lane = jc * 8 + ql, packed column q = 8 wave + ql
    const int k0 = tid >> 3, j = tid & 7;
    const bool row_role = tid < 128;
    const int jc = lane >> 3, ql = lane & 7, q = wave * 8 + ql;
    double2* const xw = Qb + (k0 & 15) * LDR + 9 * j;
    const double2* const xr = Qb + (k0 & 15) * LDR + j;
    double2* const qw = Qb + (wave * 8 + ql) * LQ + 9 * jc;
    const double2* const qr = Qb + (wave * 8 + ql) * LQ + jc;

    double2 twr[7], twc[7];
#pragma unroll
    for (int t = 1; t < 8; ++t) {
        twr[t - 1] = a.g.tw[0][j * t];
        twc[t - 1] = a.g.tw[0][jc * t];
    }
    // real spectrum of the centred lags, halved (the unpacking of D averages two terms): vhat = w^((n-1)(f0+f1)) S
    double sa[8], sb[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int f0 = jc + 8 * t;
        const double2 va = a.vhat[f0 * F + q], vb = a.vhat[f0 * F + q + 32];
        const double2 wa = a.g.tw[0][((n - 1) * (f0 + q)) & 63], wb = a.g.tw[0][((n - 1) * (f0 + q + 32)) & 63];
        sa[t] = 0.5 * (va.x * wa.x + va.y * wa.y);
        sb[t] = -0.5 * (vb.x * wb.x + vb.y * wb.y);      // sign: conjugation in front of the inverse transform
    }
    const bool z6_ok = jc > 0;                            // row 16 - jc exists

    hrow::RowLanes<8> L;                 // slots k1 = j, j + 8, j - 16, j - 8
    L.setup<false>(a, row_role, k0, j);
    const double (&wsr)[KS] = L.wsr;

#ifdef EFGP_CG_STAMPS
    long long stamp_prev = (long long)__builtin_readcyclecounter();
#endif
    int stop = 0;
    double rcp_rz = 0.0;
    auto apply_A = [&](const double2 (&u)[KS], double2 (&Au)[KS]) __attribute__((always_inline)) {
        double2 v[8];
        EFGP_STAMP(7);
        // A: rows k0 >= 0, modes k1 wrapped to positions k1 mod 64 -> G[k0][f1]
        if (row_role) {
            dft8_in4(make_double2(wsr[0] * u[0].x, wsr[0] * u[0].y), make_double2(wsr[1] * u[1].x, wsr[1] * u[1].y),
                     make_double2(wsr[2] * u[2].x, wsr[2] * u[2].y), make_double2(wsr[3] * u[3].x, wsr[3] * u[3].y), v);
            exchange_stage2(v, xw, xr, twr);
            s64::store8_all<8>(Gb + k0 * LDR + j, v);
        }
        __syncthreads();
        stop = s_stop;
        rcp_rz = s_rcp;
        if (stop) return;                                 // uniform: the iteration that just started is abandoned
        EFGP_STAMP(0);
        // B: packed columns z[k0] = G[k0][q] + i G[k0][q + 32] (k0 >= 0), conj G[-k0][q] + i conj G[-k0][q + 32] (k0 < 0)
        {
            const double2* g0 = Gb + q;
            const double2 a0 = g0[jc * LDR], b0 = g0[jc * LDR + 32];
            const double2 a1 = g0[(jc + 8) * LDR], b1 = g0[(jc + 8) * LDR + 32];
            const double2 a6 = g0[((16 - jc) & 15) * LDR], b6 = g0[((16 - jc) & 15) * LDR + 32];
            const double2 a7 = g0[(8 - jc) * LDR], b7 = g0[(8 - jc) * LDR + 32];
            // jc = 0 reads row k0 = 0, whose modes +k1 and -k1 are BOTH stored: its line G[0][.] is real only up to the rounding
            // noise the iterates have collected in that row's anti-Hermitian part, and the packing would hand that noise to the
            // other column of the pair as if it were signal -- a non-symmetric perturbation of the operator that held the TRUE
            // residual of a cg_tol = 1e-12 solve at 2e-6 (round 3, c2 golden: beta 1.3e-6 off; the reference reaches 7e-10).
            // Dropping the imaginary parts is the orthogonal projection onto coefficient arrays of real functions.
            const double2 z0 = jc == 0 ? make_double2(a0.x, b0.x) : make_double2(a0.x - b0.y, a0.y + b0.x);
            const double2 z1 = make_double2(a1.x - b1.y, a1.y + b1.x);
            double2 z6 = make_double2(a6.x + b6.y, b6.x - a6.y);
            const double2 z7 = make_double2(a7.x + b7.y, b7.x - a7.y);
            if (!z6_ok) z6 = make_double2(0.0, 0.0);
            dft8_in4(z0, z1, z6, z7, v);
            exchange_stage2(v, qw, qr, twc);              // v[t] = R_q[f0] + i R_{q+32}[f0], f0 = jc + 8 t
            // C: times the real spectrum, conjugate, forward transform = conj of the inverse transform
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = make_double2(v[t].x * sa[t], v[t].y * sb[t]);
            dft_fwd<8>(v);
            exchange_stage2<true>(v, qw, qr, twc);        // v[t] = conj T[jc + 8 t], t in {0, 1, 6, 7}
            double2* t0 = Tb + jc * LT + q;
            t0[0] = v[0];
            t0[8 * LT] = v[1];
            t0[16 * LT] = v[6];
            t0[24 * LT] = v[7];
        }
        __syncthreads();
        EFGP_STAMP(1);
        // D: row k0 >= 0 of the result from the packed columns at +k0 and -k0; conjugated inputs, forward transform
        if (row_role) {
            const double2* tp = Tb + (k0 & 15) * LT + j;
            const double2* tm = Tb + ((k0 & 15) == 0 ? 0 : 32 - (k0 & 15)) * LT + j;
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) {
                const double2 P = tp[8 * u4], Mv = tm[8 * u4];
                v[u4] = make_double2(P.x + Mv.x, P.y - Mv.y);
                v[u4 + 4] = make_double2(-P.y - Mv.y, P.x - Mv.x);
            }
            dft_fwd<8>(v);
            exchange_stage2<true>(v, xw, xr, twr);        // v[t] = conj Y[k0][j + 8 t], t in {0, 1, 6, 7}
            const double2 y[KS] = {s64::conjd(v[0]), s64::conjd(v[1]), s64::conjd(v[6]), s64::conjd(v[7])};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const double2 gg = make_double2(wsr[s] * y[s].x, wsr[s] * y[s].y);
                if (VARIANT == 0) Au[s] = make_double2(gg.x + a.sigmasq * u[s].x, gg.y + a.sigmasq * u[s].y);
                else Au[s] = make_double2(gg.x / a.sigmasq + u[s].x, gg.y / a.sigmasq + u[s].y);
            }
        } else {
#pragma unroll
            for (int s = 0; s < KS; ++s) Au[s] = make_double2(0.0, 0.0);
        }
        EFGP_STAMP(2);
    };

    if (tid == 0) {
        s_stop = 0;
        s_rcp = 0.0;
    }
    double2 Ap[KS];
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Ap[s] = make_double2(0.0, 0.0);
    } else {
        apply_A(L.xv, Ap);
    }
    double rz, bb, asym;
    L.start(a, Ap, rz, bb, asym);
    block_sum_pair_h(rz, bb, red);
    asym = block_sum_h(asym, red);
    const double ws_bad = block_sum_h(L.ws_bad, red + kWavesH);      // (disjoint scratch: no barrier between the two sums' reads and writes)
    if (hrow::refused(asym, bb, ws_bad)) {
        L.refuse(a);
        return;
    }
    const hrow::NormTest norm(bb);
    // Per iteration the row waves (0, 1) carry the dependent chain  A -> B/C -> D -> <p,Ap> -> alpha -> r -> <r,r>,<r,z> ->
    // beta -> p -> A;  everything that is not on it is done by wave 3, idle during A: the norm test of iteration i (sqrt and a
    // division) and the reciprocal for the next beta.  Its decision is read behind the first barrier of the next operator
    // application, whose A phase has then run speculatively (LDS only; x is final, p is not an output).
    if (wave == 3 && lane == 0) s_rcp = 1.0 / (rz + 1e-16);
    int it = 0;
    for (; it < a.max_iter;) {
        apply_A(L.pv, Ap);
        if (stop) break;
        const double pAp = block_sum_h(L.dot_p(Ap), red) + 1e-16;
        EFGP_STAMP(3);
        const double alpha = rz / pAp;
        double rr, rzn;
        double2 zv[KS];
        L.step(alpha, Ap, zv, rr, rzn);
        EFGP_STAMP(4);
        block_sum_pair_h(rr, rzn, red);
        EFGP_STAMP(5);
        ++it;
        if (wave == 3) norm.publish(a, rr, rzn, it, lane, &s_rcp, &s_stop);
        L.new_direction(zv, rzn, rz, rcp_rz);
    }
    L.write_out(a, it);
}

// ------------------------------------------------------------------------------------------------
// Hermitian solve on the SMALLEST circulant grid (round 4): 48 x 48 for blocks of up to 23 x 23 modes.
// The Toeplitz product is exact on any circulant grid F >= 2 n - 1 (wrap-around lands outside the crop window,
// efgpnd.py:1266-1271: the reference's own `_next_fast_fft_size` branch); next_pow2 is a choice.  The headline block
// (mtot 23, 2 n - 1 = 45) fits 48 = 3 * 16: 0.56 x the grid of cg_herm64_kernel -- 24 packed column lines instead of 32, 48-point
// lines instead of 64-point ones.  Same structure as cg_herm64_kernel (rows k0 >= 0 only, two real columns per complex column
// transform, CG vectors in the row lanes' registers, the norm test on an idle wave, refusal of non-conforming input), same
// recurrences and stopping rules (cg.py:86-153 / 155-244); results differ from the 64 x 64 embedding by rounding only.
// fft_shape / efgp_toeplitz_apply keep the reference's grid.
//
// Round 6: a single system applies the operator with ONE transformed dimension -- row transforms A, per-frequency 23 x 23
// Hermitian Toeplitz products over k0 on 192 lanes with their coefficients in registers (dense48_coeffs), row transforms D --
// two line-transform phases per application instead of four.  The packed column transforms B / C below remain for batches (the
// resident coefficients cost the second workgroup per CU: 256 + 16 registers) and behind EFGP_CG48_FFT2D=1.
// Round 9: that single system runs on eight waves, the Toeplitz products on waves of their own from sums and differences of lags at
// half the multiply-adds (cg_herm48_pairs_kernel below; EFGP_CG48_LAG_COEFFS=1 keeps the 256-thread kernel).
//
// A 48-point line lives in 8 adjacent lanes as 48 = 6 x 8, in two mirrored factorizations so that every pruned stage is a
// radix-8 butterfly with four live legs (dft8_in4 / dft8_out4 of the 64-point kernel) on SIX lanes holding positions j + 6 t,
// and every full stage a radix-6 butterfly on EIGHT lanes holding positions j + 8 t:
//   "6x8" (phases A, B: zero-padded input):  lanes j < 6: DFT-8 over t of x[j + 6 t] (t in {0, 1, 6, 7} live) -> exchange ->
//                                            lanes k < 8: twiddle w48^(k t), DFT-6 over t -> X[k + 8 k2], k2 < 6
//   "8x6" (phases C, D: cropped output):     lanes j < 8: DFT-6 over t of x[j + 8 t], twiddle w48^(j k) -> exchange ->
//                                            lanes k < 6: DFT-8 over the 8 writers -> X[k + 6 k2], k2 in {0, 1, 6, 7} kept
// The output layout of one is the input layout of the other: the CG vectors stay in the registers of the lanes j < 6 of a row
// (slots k1 = j, j + 6, j - 12, j - 6) between D and the next A, and the spectrum multiply between B and C works on registers.
// ------------------------------------------------------------------------------------------------
namespace h48 {
constexpr int kThreadsH = 256, kWavesH = kThreadsH / 64;
constexpr int HF = 24, NR = 12;          // packed column pairs, stored rows k0 = 0..11 (the grid F = 48 and LX: cg_persistent_dev.hpp)
constexpr int LDR = 56;                  // pitch of the G rows (8 mod 16)
constexpr int LT = 28;                   // pitch of the T rows (24 packed columns)
constexpr int LQ = 82;                   // column lanes' exchange scratch per line (2 mod 16)
constexpr int G_ELEMS = NR * LDR, T_ELEMS = 2 * NR * LT, Q_ELEMS = HF * LQ;
static_assert(NR * LX <= Q_ELEMS, "the row lines' scratch aliases the column lines' scratch");
constexpr int kLdsElems = G_ELEMS + T_ELEMS + Q_ELEMS;     // 53 KB
// per-frequency Toeplitz products (round 6, dense48_coeffs below): lane = (f1, three rows k0 = a0 .. a0 + 2), a0 = 0, 3, 6, 9
constexpr int ND = 4 * F;                // dense lanes (waves 0..2)
constexpr int NC = 25;                   // lags a0 - 11 .. a0 + 13 of a dense lane
constexpr int kReread = 8;               // row of the multiply-adds in front of which a dense lane re-reads G of its own three rows
constexpr int LDV = 49;                  // pitch of the prologue's 48 x 48 grid (vhat48_lines)
constexpr int kLdsElemsDense = F * LDV + (kThreadsH / 8) * LX;      // the prologue's grid + 32 line slots: 73 KB
static_assert(2 * G_ELEMS + NR * LX <= kLdsElemsDense, "the iteration's G, Yh and row scratch alias the prologue's grid");
// eight waves with paired lags (round 9, cg_herm48_pairs_kernel): waves 0-1 the row role, waves 2..7 the dense role, lane =
// (f1, group g): groups 0..3 (waves 2-4) own the rows 2 g and 2 g + 1, groups 4..7 (waves 5-7) the row 8 + (g - 4)
constexpr int kThreadsP = 512, kRowWavesP = 2, kPairWavesP = 3;
constexpr int NDP = kThreadsP - 64 * kRowWavesP;       // dense lanes: 48 frequencies x 8 groups
static_assert(NDP == 8 * F && 64 * kPairWavesP == 4 * F, "no wave mixes two-row and one-row groups");
// the one-row dense wave that sums <u, A u> and forms the step length between barriers 2 and 2b (round 12): the duty wave.  Waves
// 5, 6 and 7 measure alike (profiles/r12_cg48_alpha_wave.txt); the duty wave reads <r,z> behind barrier 3 anyway
constexpr int kAlphaWaveP = 7;
static_assert(kAlphaWaveP >= kRowWavesP + kPairWavesP && kAlphaWaveP < kThreadsP / 64, "a wave of the one-row dense role");
constexpr int kLdsElemsPairs = F * LDV + (kThreadsP / 8) * LX;      // the prologue's grid + 64 line slots: 111 KB

// "6x8", second half: the lanes j < 6 of a line hand their eight first-stage outputs over (scratch [writer][value], pitch 9);
// every lane k < 8 takes value k of the six writers, twiddles with tw[t - 1] = w48^(k t) and runs the radix-6 stage:
// u[k2] = X[k + 8 k2].
__device__ __forceinline__ void exchange_8to6(const double2 (&v)[8], double2 (&u)[6], bool writer, double2* __restrict__ wr,
                                              const double2* __restrict__ rd, const double2 (&tw)[5]) {
    wave_sync();
    if (writer) s64::store8_all<1>(wr, v);
    wave_sync();
#pragma unroll
    for (int t = 0; t < 6; ++t) u[t] = rd[9 * t];
#pragma unroll
    for (int t = 1; t < 6; ++t) u[t] = cmulp(u[t], tw[t - 1]);
    dft6(u);
}
// a row lane's share of <x, x>: scale * sum |x[s]|^2 over its four slots.  The statements of exchange_8to6_norm below, for a caller
// that forms the share outside the exchange (cg_herm48_pairs_kernel with ALPHA_WAVE).  A copy, not a call from there: calling it
// from exchange_8to6_norm reorders the assembly of every kernel that uses the exchange (profiles/r12_cg48_alpha_wave.txt)
__device__ __forceinline__ double norm_share(const double2 (&x)[4], double scale) {
    const double x01 = fma(x[0].x, x[0].x, x[0].y * x[0].y) + fma(x[1].x, x[1].x, x[1].y * x[1].y);
    const double x23 = fma(x[2].x, x[2].x, x[2].y * x[2].y) + fma(x[3].x, x[3].x, x[3].y * x[3].y);
    return scale * (x01 + x23);
}
// exchange_8to6 for an iteration that forms <p, A p> ahead of D (cg_herm48_kernel, FREQ_DOT): the lane's share of <x, x>,
// scale * sum |x[s]|^2, is issued behind the six reads, while they are under way.
__device__ __forceinline__ double exchange_8to6_norm(const double2 (&v)[8], double2 (&u)[6], bool writer, double2* __restrict__ wr,
                                                     const double2* __restrict__ rd, const double2 (&tw)[5], const double2 (&x)[4],
                                                     double scale) {
    wave_sync();
    if (writer) s64::store8_all<1>(wr, v);
    wave_sync();
#pragma unroll
    for (int t = 0; t < 6; ++t) u[t] = rd[9 * t];
    __builtin_amdgcn_sched_barrier(0);
    const double x01 = fma(x[0].x, x[0].x, x[0].y * x[0].y) + fma(x[1].x, x[1].x, x[1].y * x[1].y);
    const double x23 = fma(x[2].x, x[2].x, x[2].y * x[2].y) + fma(x[3].x, x[3].x, x[3].y * x[3].y);
    const double xx = scale * (x01 + x23);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 1; t < 6; ++t) u[t] = cmulp(u[t], tw[t - 1]);
    dft6(u);
    return xx;
}
// "8x6", second half: every lane j < 8 has run the radix-6 stage on u and twiddles its outputs with tw[k - 1] = w48^(j k); the
// lanes k < 6 take value k of the eight writers and run the radix-8 stage of which the outputs 0, 1, 6, 7 are wanted:
// v[k2] = X[k + 6 k2].
__device__ __forceinline__ void exchange_6to8(double2 (&u)[6], double2 (&v)[8], double2* __restrict__ wr, const double2* __restrict__ rd,
                                              const double2 (&tw)[5]) {
#pragma unroll
    for (int t = 1; t < 6; ++t) u[t] = cmulp(u[t], tw[t - 1]);
    wave_sync();
#pragma unroll
    for (int t = 0; t < 6; ++t) wr[t] = u[t];
    wave_sync();
    s64::load8_all<9>(rd, v);
    h64::dft8_out4(v);
}

// sum over the lanes 0..31 of a wave, returned to every lane; also right where the lanes 32..63 sit out (they are not read)
__device__ __forceinline__ double half_wave_sum(double v) {
    EFGP_DPP_ADD(v, 0x111, 0xF);   // row_shr:1
    EFGP_DPP_ADD(v, 0x112, 0xF);   // row_shr:2
    EFGP_DPP_ADD(v, 0x114, 0xF);   // row_shr:4
    EFGP_DPP_ADD(v, 0x118, 0xF);   // row_shr:8   -> lane 15 of every 16-lane row holds the row sum
    EFGP_DPP_ADD(v, 0x142, 0xA);   // row_bcast:15 into row 1 -> lane 31 holds the sum of the lanes 0..31
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 31);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 31);
    return __hiloint2double(hi, lo);
}
// num / (sum of `part` over the lanes 0..31 + 1e-16): the step length of an iteration that forms <p, A p> ahead of D
__device__ __forceinline__ double quot_half_wave(double part, double num) { return num / (half_wave_sum(part) + 1e-16); }

// h64::dft8_in4 of (w[0] u[0], w[1] u[1], 0, 0, 0, 0, w[2] u[2], w[3] u[3]) with the roundings written out.  Each first butterfly
// adds two products, and which of the two the compiler rounds and which it fuses into the sum is its choice: it fell the other way
// when u became one of two alternating arrays (cg_herm48_pairs_kernel, round 11).  This is the form the kernels had before: the
// products of the slots 0 and 1 are rounded and those of the slots 2 and 3 fused in the loop's applications (LOW_ROUNDED), the
// reverse in the application in front of the loop (A x0 of a warm start).
// The odd outputs of the tail, e + hh t and e - hh t, are one fused multiply-add each where the whole tail stands in the writers'
// block; when the compiler leaves half of it in front of that block (cg_herm48_pairs_kernel with ALPHA_WAVE, round 12) the product
// hh t is rounded for the outputs behind the branch.  h64::dft8_in4_tail with those eight roundings written out as every kernel
// had them.
__device__ __forceinline__ void dft8_in4_tail_fused(double2 e0, double2 e1, double2 e2, double2 e3, double2 o0, double2 o1r, double2 o2r,
                                                    double2 o3r, double2 (&v)[8]) {
    const double hh = 0.70710678118654752440;
    const double s1 = o1r.x + o1r.y, d1 = o1r.y - o1r.x, s3 = o3r.x + o3r.y, d3 = o3r.y - o3r.x;
    const double2 o2 = mul_mi(o2r);
    v[0] = cadd(e0, o0);
    v[4] = csub(e0, o0);
    v[1] = make_double2(fma(hh, s1, e1.x), fma(hh, d1, e1.y));
    v[5] = make_double2(fma(-hh, s1, e1.x), fma(-hh, d1, e1.y));
    v[2] = cadd(e2, o2);
    v[6] = csub(e2, o2);
    v[3] = make_double2(fma(hh, d3, e3.x), fma(-hh, s3, e3.y));
    v[7] = make_double2(fma(-hh, d3, e3.x), fma(hh, s3, e3.y));
}

// FUSED_TAIL: the tail's roundings written out as well (dft8_in4_tail_fused).
template <bool LOW_ROUNDED, bool FUSED_TAIL = false>
__device__ __forceinline__ void dft8_in4_ws(const double (&w)[4], const double2 (&u)[4], double2 (&v)[8]) {
    // r0, r1: the slots whose products are rounded (ra, rb); f0, f1: those whose products are fused (wa ua, wb ub)
    constexpr int r0 = LOW_ROUNDED ? 0 : 2, r1 = LOW_ROUNDED ? 1 : 3, f0 = LOW_ROUNDED ? 2 : 0, f1 = LOW_ROUNDED ? 3 : 1;
    double2 e0, e1, e2, e3, o0, o1r, o2r, o3r;
    const double2 ra = make_double2(__dmul_rn(w[r0], u[r0].x), __dmul_rn(w[r0], u[r0].y));
    const double2 rb = make_double2(__dmul_rn(w[r1], u[r1].x), __dmul_rn(w[r1], u[r1].y));
    const double wa = w[f0], wb = w[f1];
    const double2 ua = u[f0], ub = u[f1];
    if constexpr (LOW_ROUNDED) {
        // a0 = ra, a6 = wa ua: a0 + a6, a0 + i a6, a0 - a6, a0 - i a6; the same of a1 = rb, a7 = wb ub
        e0 = make_double2(fma(wa, ua.x, ra.x), fma(wa, ua.y, ra.y));
        e1 = make_double2(fma(-wa, ua.y, ra.x), fma(wa, ua.x, ra.y));
        e2 = make_double2(fma(-wa, ua.x, ra.x), fma(-wa, ua.y, ra.y));
        e3 = make_double2(fma(wa, ua.y, ra.x), fma(-wa, ua.x, ra.y));
        o0 = make_double2(fma(wb, ub.x, rb.x), fma(wb, ub.y, rb.y));
        o1r = make_double2(fma(-wb, ub.y, rb.x), fma(wb, ub.x, rb.y));
        o2r = make_double2(fma(-wb, ub.x, rb.x), fma(-wb, ub.y, rb.y));
        o3r = make_double2(fma(wb, ub.y, rb.x), fma(-wb, ub.x, rb.y));
    } else {
        // a0 = wa ua, a6 = ra
        e0 = make_double2(fma(wa, ua.x, ra.x), fma(wa, ua.y, ra.y));
        e1 = make_double2(fma(wa, ua.x, -ra.y), fma(wa, ua.y, ra.x));
        e2 = make_double2(fma(wa, ua.x, -ra.x), fma(wa, ua.y, -ra.y));
        e3 = make_double2(fma(wa, ua.x, ra.y), fma(wa, ua.y, -ra.x));
        o0 = make_double2(fma(wb, ub.x, rb.x), fma(wb, ub.y, rb.y));
        o1r = make_double2(fma(wb, ub.x, -rb.y), fma(wb, ub.y, rb.x));
        o2r = make_double2(fma(wb, ub.x, -rb.x), fma(wb, ub.y, -rb.y));
        o3r = make_double2(fma(wb, ub.x, rb.y), fma(wb, ub.y, -rb.x));
    }
    if constexpr (FUSED_TAIL) dft8_in4_tail_fused(e0, e1, e2, e3, o0, o1r, o2r, o3r, v);
    else h64::dft8_in4_tail(e0, e1, e2, e3, o0, o1r, o2r, o3r, v);
}

// wave_sum of two values at once: the stages of the two chains alternate, so that the moves of one stand where the other waits for
// its sum.  Each value goes through wave_sum's tree, stage by stage: the same bits.
__device__ __forceinline__ void wave_sum_pair(double& u, double& v) {
    EFGP_DPP_ADD(u, 0x111, 0xF);
    EFGP_DPP_ADD(v, 0x111, 0xF);
    EFGP_DPP_ADD(u, 0x112, 0xF);
    EFGP_DPP_ADD(v, 0x112, 0xF);
    EFGP_DPP_ADD(u, 0x114, 0xF);
    EFGP_DPP_ADD(v, 0x114, 0xF);
    EFGP_DPP_ADD(u, 0x118, 0xF);
    EFGP_DPP_ADD(v, 0x118, 0xF);
    EFGP_DPP_ADD(u, 0x142, 0xA);
    EFGP_DPP_ADD(v, 0x142, 0xA);
    EFGP_DPP_ADD(u, 0x143, 0xC);
    EFGP_DPP_ADD(v, 0x143, 0xC);
    const int ulo = __builtin_amdgcn_readlane(__double2loint(u), 63), uhi = __builtin_amdgcn_readlane(__double2hiint(u), 63);
    const int vlo = __builtin_amdgcn_readlane(__double2loint(v), 63), vhi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    u = __hiloint2double(uhi, ulo);
    v = __hiloint2double(vhi, vlo);
}

// exchange_6to8 for an iteration that forms <p, A p> ahead of D (cg_herm48_kernel, FREQ_DOT): the sum of `part` over the lanes 0..31
// and the quotient num / (sum + 1e-16) are issued behind the eight reads, while the LDS trip (the six writes, then the reads) is
// under way.  A wave runs one instruction at a time, so the wait for LDS is where they cost least.
__device__ __forceinline__ double exchange_6to8_quot(double2 (&u)[6], double2 (&v)[8], double2* __restrict__ wr,
                                                     const double2* __restrict__ rd, const double2 (&tw)[5], double part, double num) {
#pragma unroll
    for (int t = 1; t < 6; ++t) u[t] = cmulp(u[t], tw[t - 1]);
    wave_sync();
#pragma unroll
    for (int t = 0; t < 6; ++t) wr[t] = u[t];
    wave_sync();
    s64::load8_all<9>(rd, v);
    __builtin_amdgcn_sched_barrier(0);
    const double quot = quot_half_wave(part, num);
    __builtin_amdgcn_sched_barrier(0);
    h64::dft8_out4(v);
    return quot;
}

// <u, A u> of the eight-wave kernel from the 480 summands in s_part (cg_herm48_pairs_kernel): fifteen per lane, lane l of a wave
// takes the entries l mod 32 + 32 t -- twelve Toeplitz terms of the dense lanes and three of the row lanes' shares of sigma^2 <u,u>
// -- then quot_half_wave over the lanes 0..31.  ONE definition of the reads and of the tree for the row lanes (the ALPHA_WAVE false
// arms) and for the dense wave that sums beside D (ALPHA_WAVE): the arms are compared bit for bit.
__device__ __forceinline__ void uAu_summands(const double* s_part, int lane, double (&pt)[15]) {
    const double* sp = s_part + (lane & 31);
#pragma unroll
    for (int t = 0; t < 15; ++t) pt[t] = sp[32 * t];
}
template <int VARIANT>
__device__ __forceinline__ double uAu_of_lane(const double (&pt)[15], double sigmasq) {
    double tsum = (((pt[0] + pt[1]) + (pt[2] + pt[3])) + ((pt[4] + pt[5]) + (pt[6] + pt[7]))) + ((pt[8] + pt[9]) + (pt[10] + pt[11]));
    if (VARIANT == 1) tsum /= sigmasq;
    return tsum + ((pt[12] + pt[13]) + pt[14]);
}

// Coefficients of the per-frequency Toeplitz products (round 6).  After the row transforms of phase A the remaining convolution
// over k0 is, for every f1, a 23 x 23 Hermitian Toeplitz product
//     Yh[k0][f1] = sum_{k0' = -11..11} c(k0 - k0', f1) G[k0'][f1],      G[-k0'][f1] = conj G[k0'][f1],
//     c(l0, f1) = (1 / 48) sum_l1 v(l0, l1) w48^(f1 l1),                c(-l0, f1) = conj c(l0, f1)
// (the 1 / 48 is the inverse row transform's, the lags are centred).  buf = lds2[f0 * LDV + f1] holds the 48 x 48 spectrum
// (vhat48_lines: factor 1 / 2304, lag l stored at l + n - 1); one inverse pass along f0 in place (the "8x6" lines of
// vhat48_lines on conjugated data) leaves w48^((n - 1) f1) c(i0 - (n - 1), f1) at [i0][f1].  The dense lane (f1, a0) then takes its
// 25 lags a0 - 11 .. a0 + 13 into registers for the whole solve: cf[i] = c(a0 - 11 + i, f1), negative lags as conjugates of the
// positive ones, lag 0 real, lags beyond the Toeplitz vector zero.  NT = 256 threads, tw[t - 1] = w48^((tid & 7) t).
template <int NT>
__device__ __forceinline__ void dense48_coeffs(double2* lds2, const double2 (&tw)[5], const double2* __restrict__ twg, int n,
                                               double2 (&cf)[NC]) {
    constexpr int SLOTS = NT / 8, PASSES = (F + SLOTS - 1) / SLOTS;
    double2* const buf = lds2;                       // [48][LDV]
    double2* const scr = lds2 + F * LDV;             // [SLOTS lines][writer 9 j + value]
    const int tid = threadIdx.x, slot = tid >> 3, j = tid & 7;
    double2* const wr = scr + slot * LX + 9 * j;
    const double2* const rd = scr + slot * LX + j;
    double2 u6[6], x8[8];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int line = slot + ps * SLOTS;
        const bool act = line < F;
#pragma unroll
        for (int t = 0; t < 6; ++t) u6[t] = act ? s64::conjd(buf[(j + 8 * t) * LDV + line]) : make_double2(0.0, 0.0);
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
            for (int t = 0; t < 8; ++t) buf[(j + 6 * t) * LDV + line] = s64::conjd(x8[t]);
        }
    }
    __syncthreads();
    const int f1 = tid % F, a0 = 3 * (tid / F);
    const bool dense = tid < ND;
    const double2 wc = twg[((n - 1) * f1) % F];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int l = a0 - 11 + i, al = l < 0 ? -l : l;
        double2 c = make_double2(0.0, 0.0);
        if (dense && al <= n - 1) {
            const double2 r = buf[(al + n - 1) * LDV + f1];
            c = make_double2(fma(r.y, wc.y, r.x * wc.x), fma(-r.x, wc.y, r.y * wc.x));       // r conj(wc)
            if (l < 0) c.y = -c.y;
            if (l == 0) c.y = 0.0;
        }
        cf[i] = c;
    }
}

// The inverse pass of dense48_coeffs and the fetch of one lag for the eight-wave kernel (cg_herm48_pairs_kernel, round 9), which runs
// the pass on 512 threads (64 line slots, one pass) and makes sums and differences of lags out of the same c(l0, f1): the same
// statements per line and per lag.  They stand beside dense48_coeffs, not inside it: called from there, the 256-thread kernels no
// longer compiled to the instructions they had (the schedule moved in five instantiations, profiles/r9_cg48_lag_pairs_ab.txt).
template <int NT>
__device__ __forceinline__ void dense48_inverse_pass(double2* lds2, const double2 (&tw)[5]) {
    constexpr int SLOTS = NT / 8, PASSES = (F + SLOTS - 1) / SLOTS;
    double2* const buf = lds2;                       // [48][LDV]
    double2* const scr = lds2 + F * LDV;             // [SLOTS lines][writer 9 j + value]
    const int tid = threadIdx.x, slot = tid >> 3, j = tid & 7;
    double2* const wr = scr + slot * LX + 9 * j;
    const double2* const rd = scr + slot * LX + j;
    double2 u6[6], x8[8];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int line = slot + ps * SLOTS;
        const bool act = line < F;
#pragma unroll
        for (int t = 0; t < 6; ++t) u6[t] = act ? s64::conjd(buf[(j + 8 * t) * LDV + line]) : make_double2(0.0, 0.0);
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
            for (int t = 0; t < 8; ++t) buf[(j + 6 * t) * LDV + line] = s64::conjd(x8[t]);
        }
    }
}
// c(l, f1) out of the grid the inverse pass leaves, wc = w48^((n - 1) f1): negative lags as conjugates of the positive ones, lag 0
// real, lags beyond the Toeplitz vector zero
__device__ __forceinline__ double2 lag_coeff(const double2* buf, double2 wc, int n, int f1, int l) {
    const int al = l < 0 ? -l : l;
    double2 c = make_double2(0.0, 0.0);
    if (al <= n - 1) {
        const double2 r = buf[(al + n - 1) * LDV + f1];
        c = make_double2(fma(r.y, wc.y, r.x * wc.x), fma(-r.x, wc.y, r.y * wc.x));       // r conj(wc)
        if (l < 0) c.y = -c.y;
        if (l == 0) c.y = 0.0;
    }
    return c;
}

// Paired lags (round 9).  With G[m] = a + i b the two terms of an input row m >= 1,
//     c(k0 - m) G[m] + c(k0 + m) conj G[m] = S a + i Q b,      S(k0, m) = c(k0 - m) + c(k0 + m),  Q(k0, m) = c(k0 - m) - c(k0 + m),
// cost four multiply-adds instead of eight: Re += S.x a - Q.y b, Im += S.y a + Q.x b.  S and Q belong to one output row (they are
// not Toeplitz-shared between the rows of a lane): c(k0), eleven S and eleven Q are 46 doubles per output, rounded once here.
constexpr int NM = NR - 1;               // input rows m = 1..11
struct PairCoeffs {
    double2 c0;                          // c(k0): the m = 0 term, c(k0) Re G[0]
    double2 S[NM], Q[NM];
};
__device__ __forceinline__ void pair_coeffs(const double2* buf, double2 wc, int n, int f1, int k0, PairCoeffs& pc) {
    pc.c0 = lag_coeff(buf, wc, n, f1, k0);
#pragma unroll
    for (int m = 1; m < NR; ++m) {
        const double2 cm = lag_coeff(buf, wc, n, f1, k0 - m), cp = lag_coeff(buf, wc, n, f1, k0 + m);
        pc.S[m - 1] = cadd(cm, cp);
        pc.Q[m - 1] = csub(cm, cp);
    }
}
// Yh[k0] of one frequency from the twelve rows gm[m] = G[m]: two statements for m = 0 (the imaginary part of G[0] is dropped, as in
// cg_herm48_kernel), four multiply-adds per m >= 1
__device__ __forceinline__ double2 pair_product(const PairCoeffs& pc, const double2 (&gm)[NR]) {
    double2 acc = make_double2(pc.c0.x * gm[0].x, pc.c0.y * gm[0].x);
#pragma unroll
    for (int m = 1; m < NR; ++m) {
        acc.x = fma(pc.S[m - 1].x, gm[m].x, acc.x);
        acc.y = fma(pc.S[m - 1].y, gm[m].x, acc.y);
        acc.x = fma(-pc.Q[m - 1].y, gm[m].y, acc.x);
        acc.y = fma(pc.Q[m - 1].x, gm[m].y, acc.y);
    }
    return acc;
}
}  // namespace h48

// FUSED (the fit's cold-start mean solve, efgp_cg_solve_mean_fused): the 48 x 48 spectrum is made in the prologue from the Toeplitz
// vector (vhat48_lines on the 256 threads, in LDS the iteration reuses afterwards) and ws is evaluated from the built-in kernel's
// parameters (spectral_weights.hpp) by the row lanes that hold the modes; both are written out for later users.  The iteration is
// the same code.
// DENSE (round 6): the operator application keeps the row transforms A and D and replaces the packed column transforms B / C by
// per-frequency Hermitian Toeplitz products over k0 with coefficients resident in registers (h48::dense48_coeffs); !DENSE is the
// round 4 application (EFGP_CG48_FFT2D=1).
// FREQ_DOT (round 7, DENSE only): <p, A p> is formed in the row-frequency domain, one phase early, and the iteration runs on three
// workgroup barriers instead of four.  ws is real and A transforms ws * p, so <p, A p> = sigma^2 <p, p> + <ws p, T (ws p)>, and by
// Parseval along k1 (a 48-point transform of a row supported on the 23 modes; the 1 / 48 of the inverse sits in cf)
//     <ws p, T ws p> = sum_f1 [ Re G[0][f1] Yh[0][f1] + 2 sum_{k0 = 1..11} Re(conj G[k0][f1] Yh[k0][f1]) ]
// with exactly the G the dense lanes read and the Yh they produce (row 0: both after the projection, so the identity also holds
// for an iterate with a conjugate-odd part).  The same recurrence with one inner product evaluated in another basis; no vector is
// formed by recurrence.  !FREQ_DOT (EFGP_CG48_MODE_DOT=1) is the round 6 iteration: <p, A p> summed over the modes behind D.
// This kernel keeps its own text of the row lanes' bookkeeping (hrow::RowLanes serves the other two): with the shared members, or
// with only set-up, first residual, refusal and write-out shared, its arms ran 0.5 to 2 % slower per iteration (profiles/cg_herm_refactor_ab.txt;
// 256 VGPRs plus AGPRs: the allocation moved).  A change to the stopping rule, the preconditioner or the refusal is made in hrow AND here.
template <int VARIANT, bool FUSED = false, bool DENSE = true, bool FREQ_DOT = false>
__global__ __launch_bounds__(h48::kThreadsH) void cg_herm48_kernel(Args a) {
    using namespace h48;
    using h64::block_sum_h;
    using h64::block_sum_pair_h;
    using h64::dft8_in4;
    using h64::div_rcp;
    constexpr int KS = 4;
    static_assert(h64::kWavesH == kWavesH, "the block reductions are shared with the 64 x 64 kernel");
    static_assert(DENSE || !FREQ_DOT, "the row-frequency <p,Ap> reads what the per-frequency Toeplitz products hold");
    extern __shared__ double2 lds2[];
    __shared__ double red[4 * kWavesH];
    __shared__ double s_rcp;             // 1 / (<r,z> + 1e-16) for the next beta, computed by an idle wave during A
    __shared__ int s_stop;               // convergence decision of the last completed iteration, taken by an idle wave during A
    // FREQ_DOT: the lanes' summands of <u, A u>.  [0, ND): the Toeplitz terms of the dense lanes, written between barriers 1 and 2;
    // [ND, ND + 96): wgt * sigma^2 sum |u|^2 over the four slots of every row lane (0 where a lane holds no mode), written in A, in
    // front of barrier 1.  Both are read behind barrier 2, by the row lanes in D; the next writes (the next A, the next dense
    // phase) have barrier 3 behind that read.  A warm start's first application leaves nothing to clear: every slot is rewritten.
    __shared__ double s_part[FREQ_DOT ? ND + 8 * NR : 1];
    double2* const Gb = lds2;                    // G[k0][f1], k0 = 0..11 (rows beyond h are zero), f1 = 0..47
    double2* const Tb = lds2 + G_ELEMS;          // conj T[row(p)][q]: rows p = 0..11 and 36..47 (stored at p - 24); DENSE: conj Yh[k0][f1], pitch LDR
    double2* const Qb = Tb + (DENSE ? G_ELEMS : T_ELEMS);       // exchange scratch: column lines (B/C), aliased by the row lines (A, D)
    const int n = a.g.n[0], h = (n - 1) / 2, M = a.g.M;
    const int row = blockIdx.x;
    const int64_t base = (int64_t)row * M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // row role (12 lines x 8 lanes: wave 0 and half of wave 1): lane = k0 * 8 + j, the vector lives in the lanes j < 6;
    // column role (waves 0..2): lane = jc * 8 + ql, packed column q = 8 wave + ql < 24
    const int k0 = tid >> 3, j = tid & 7;
    const bool row_role = tid < 8 * NR, vec_role = row_role && j < 6;
    const int jc = lane >> 3, ql = lane & 7, q = wave * 8 + ql;
    const bool col_role = wave < 3, col6 = jc < 6;
    const int k0s = row_role ? k0 : 0;
    double2* const xw = Qb + k0s * LX + 9 * j;
    const double2* const xr = Qb + k0s * LX + j;
    const int qs = col_role ? q : 0;
    double2* const qw = Qb + qs * LQ + 9 * jc;
    const double2* const qr = Qb + qs * LQ + jc;
    // dense role (DENSE, waves 0..2): lane = (f1d, rows k0 = kd, kd + 1, kd + 2)
    const bool dense_role = tid < ND;
    const int f1d = tid % F, kd = 3 * (tid / F);

    double2 twr[5], twc[5];              // w48^(lane-in-line * t), t = 1..5 (35 at most: no wrap)
#pragma unroll
    for (int t = 1; t < 6; ++t) {
        twr[t - 1] = a.g.tw[0][j * t];
        twc[t - 1] = a.g.tw[0][jc * t];
    }
    if (FUSED) {
        vhat48_lines<kThreadsH, true>(a.vsrc, a.vL0, a.vL1, 1.0 / 2304.0, a.vhat_out, lds2);
        __syncthreads();
    }
    double sa[6], sb[6];
    double2 cf[DENSE ? NC : 1];
    if constexpr (DENSE) {
        // the operator's spectrum, from memory or from the prologue's grid (the same numbers), through one inverse pass along f0:
        // the same statements with and without FUSED
        if (!FUSED) {
#pragma unroll
            for (int k = 0; k < F * F / kThreadsH; ++k) {
                const int t = tid + k * kThreadsH, i0 = t / F, i1 = t - i0 * F;
                lds2[i0 * LDV + i1] = a.vhat[t];
            }
            __syncthreads();
        }
        dense48_coeffs<kThreadsH>(lds2, twr, a.g.tw[0], n, cf);
        __syncthreads();                                  // the iteration's G / Yh / scratch alias the prologue's grid
    } else {
        // real spectrum of the centred lags, halved (the unpacking of D averages two terms): vhat = w^((n-1)(f0+f1)) S
        const double2* const vh = FUSED ? lds2 : a.vhat;
        constexpr int LV = FUSED ? LDV : F;               // pitch of vh: the prologue's grid, or the operator's spectrum
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int f0 = jc + 8 * t;
            const double2 va = vh[f0 * LV + qs], vb = vh[f0 * LV + qs + HF];
            const double2 wa = a.g.tw[0][((n - 1) * (f0 + qs)) % F], wb = a.g.tw[0][((n - 1) * (f0 + qs + HF)) % F];
            sa[t] = 0.5 * (va.x * wa.x + va.y * wa.y);
            sb[t] = -0.5 * (vb.x * wb.x + vb.y * wb.y);      // sign: conjugation in front of the inverse transform
        }
        if (FUSED) __syncthreads();                           // the iteration's G / T / scratch alias the prologue's grid
    }
    const bool z6_ok = jc > 0;                            // row 12 - jc exists
    const int jr = col6 ? jc : 0;                         // rows this lane packs in B (the lanes jc >= 6 only take part in the radix-6 stages)

    // vector slots of a row lane j < 6: positions j + 6 t, t in {0, 1, 6, 7} <-> k1 = j, j + 6, j - 12, j - 6
    double2 xv[KS], rv[KS], pv[KS];
    double wsr[KS], dg[KS], rdg[KS];     // ws is real here (checked below): ws * u costs two multiplies
    bool ok[KS];
    int idx[KS];
    const bool precond = a.diag != nullptr || a.diag_scale != nullptr;
    const double wgt = k0 == 0 ? 1.0 : 2.0;
    double ws_bad = 0.0;                 // > 0: ws is not real and even
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k1 = s == 0 ? j : (s == 1 ? j + 6 : (s == 2 ? j - 12 : j - 6));
        ok[s] = vec_role && k0 <= h && k1 <= h && -k1 <= h;
        idx[s] = ok[s] ? (k0 + h) * n + (k1 + h) : 0;
        double ws_im = 0.0;
        if (ok[s] && FUSED) {
            // ws = sqrt(S h^d) is real and even by construction: node idx and its mirror M - 1 - idx get the same value
            xv[s] = make_double2(0.0, 0.0);
            const double2 w = make_double2(spectral_weight_at(a.wk_kind, a.g.d, a.wk_nu, a.wk_ell, a.wk_c0, a.wk_h, a.wk_mtot, idx[s]), 0.0);
            a.ws_out[idx[s]] = w;
            a.ws_out[M - 1 - idx[s]] = w;
            wsr[s] = w.x;
            dg[s] = jacobi_entry(a, w, idx[s]);
        } else if (ok[s]) {
            xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x0[base + idx[s]];
            const double2 w = a.ws[idx[s]], wm = a.ws[M - 1 - idx[s]];
            wsr[s] = w.x;
            ws_im = w.y * w.y + (w.x - wm.x) * (w.x - wm.x) + wm.y * wm.y;
            dg[s] = jacobi_entry(a, w, idx[s]);
        } else {
            xv[s] = make_double2(0.0, 0.0);
            wsr[s] = 0.0;
            dg[s] = 1.0;
        }
        ws_bad += ws_im;
        rdg[s] = 1.0 / dg[s];
        rv[s] = pv[s] = make_double2(0.0, 0.0);
    }

#ifdef EFGP_CG_STAMPS
    long long stamp_prev = (long long)__builtin_readcyclecounter();
#endif
    int stop = 0;
    double rcp_rz = 0.0;
    double rz = 0.0;
    double alpha_fd = 0.0;               // FREQ_DOT: rz / (<u, A u> + 1e-16) of the last operator application, formed inside D
    auto apply_A = [&](const double2 (&u)[KS], double2 (&Au)[KS]) __attribute__((always_inline)) {
        double2 v[8], u6[6];
        EFGP_STAMP(7);
        // A ("6x8"): rows k0 >= 0, modes k1 wrapped to positions k1 mod 48 -> G[k0][f1]
        if (row_role) {
            double uu = 0.0;
            dft8_in4(make_double2(wsr[0] * u[0].x, wsr[0] * u[0].y), make_double2(wsr[1] * u[1].x, wsr[1] * u[1].y),
                     make_double2(wsr[2] * u[2].x, wsr[2] * u[2].y), make_double2(wsr[3] * u[3].x, wsr[3] * u[3].y), v);
            // u6[k2] = G[k0][j + 8 k2].  FREQ_DOT: and the lane's share of the sigma^2 <u,u> of <u, A u> (the slots without a mode
            // hold zeros)
            if constexpr (FREQ_DOT) uu = exchange_8to6_norm(v, u6, j < 6, xw, xr, twr, u, VARIANT == 0 ? wgt * a.sigmasq : wgt);
            else exchange_8to6(v, u6, j < 6, xw, xr, twr);
            double2* g0 = Gb + k0 * LDR + j;
#pragma unroll
            for (int t = 0; t < 6; ++t) g0[8 * t] = u6[t];
            if constexpr (FREQ_DOT) s_part[ND + tid] = uu;
        }
        __syncthreads();
        stop = s_stop;
        rcp_rz = s_rcp;
        if (stop) return;                                 // uniform: the iteration that just started is abandoned
        EFGP_STAMP(0);
        if constexpr (DENSE) {
            // per-frequency Hermitian Toeplitz product over k0: Yh[k0] = c(k0) Re G[0] + sum_m c(k0 - m) G[m] + c(k0 + m) conj G[m],
            // m = 1..11.  Row 0 holds the modes +k1 and -k1 BOTH: the imaginary parts of G[0] and Yh[0] are dropped (the projection
            // onto coefficient arrays of real functions that the packed columns make; see cg_herm64_kernel).  All twelve reads of
            // G are in flight before the first multiply; the accumulators are six independent chains.
            if (dense_role) {
                const double2* g0 = Gb + f1d;
                double2 gm[NR];
#pragma unroll
                for (int m = 0; m < NR; ++m) gm[m] = g0[m * LDR];
                double2 acc[3];
#pragma unroll
                for (int o = 0; o < 3; ++o) acc[o] = make_double2(cf[11 + o].x * gm[0].x, cf[11 + o].y * gm[0].x);
                double2 gk[3];
#pragma unroll
                for (int m = 1; m < NR; ++m) {
                    if constexpr (FREQ_DOT) {
                        // G of the lane's own rows once more (kd differs between the lanes of a wave: gm[kd + o] is no register).
                        // Issued late in the multiply-adds, into registers that rows of gm have left: next to the twelve reads the
                        // three would push coefficients out to AGPRs, behind the loop their latency would stand exposed.
                        if (m == kReread) {
#pragma unroll
                            for (int o = 0; o < 3; ++o) gk[o] = g0[(kd + o) * LDR];
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
#pragma unroll
                    for (int o = 0; o < 3; ++o) {
                        const double2 cm = cf[11 + o - m], cp = cf[11 + o + m];
                        acc[o].x = fma(cm.x, gm[m].x, acc[o].x);
                        acc[o].y = fma(cm.x, gm[m].y, acc[o].y);
                        acc[o].x = fma(-cm.y, gm[m].y, acc[o].x);
                        acc[o].y = fma(cm.y, gm[m].x, acc[o].y);
                        acc[o].x = fma(cp.x, gm[m].x, acc[o].x);
                        acc[o].y = fma(-cp.x, gm[m].y, acc[o].y);
                        acc[o].x = fma(cp.y, gm[m].y, acc[o].x);
                        acc[o].y = fma(cp.y, gm[m].x, acc[o].y);
                    }
                }
                double2* t0 = Tb + kd * LDR + f1d;
                t0[0] = make_double2(acc[0].x, kd == 0 ? 0.0 : -acc[0].y);       // conj Yh: D transforms conjugated inputs
                t0[LDR] = make_double2(acc[1].x, -acc[1].y);
                t0[2 * LDR] = make_double2(acc[2].x, -acc[2].y);
                if constexpr (FREQ_DOT) {
                    EFGP_STAMP(1);
                    // Re(conj G Yh) of the three rows: row 0 once and from the real parts only, the others twice (rows beyond h
                    // have G = 0)
                    const double t0r = kd == 0 ? gk[0].x * acc[0].x : 2.0 * fma(gk[0].y, acc[0].y, gk[0].x * acc[0].x);
                    const double t12 = fma(gk[1].y, acc[1].y, gk[1].x * acc[1].x) + fma(gk[2].y, acc[2].y, gk[2].x * acc[2].x);
                    // no wave sum here, where it would stand on the chain of the phase: the row lanes add the lanes' terms up in D
                    s_part[tid] = fma(2.0, t12, t0r);
                }
            }
        } else if (col_role) {
            // B ("6x8"): packed columns z[k0] = G[k0][q] + i G[k0][q + 24] (k0 >= 0), conj G[-k0][q] + i conj G[-k0][q + 24] (k0 < 0),
            // rows of lane jc < 6: k0 = jc, jc + 6, jc - 12, jc - 6
            const double2* g0 = Gb + q;
            const double2 a0 = g0[jr * LDR], b0 = g0[jr * LDR + HF];
            const double2 a1 = g0[(jr + 6) * LDR], b1 = g0[(jr + 6) * LDR + HF];
            const double2 a6 = g0[((12 - jr) % 12) * LDR], b6 = g0[((12 - jr) % 12) * LDR + HF];
            const double2 a7 = g0[(6 - jr) * LDR], b7 = g0[(6 - jr) * LDR + HF];
            // jc = 0 reads row k0 = 0, whose modes +k1 and -k1 are BOTH stored: drop the imaginary parts (the projection onto
            // coefficient arrays of real functions; see cg_herm64_kernel)
            const double2 z0 = jc == 0 ? make_double2(a0.x, b0.x) : make_double2(a0.x - b0.y, a0.y + b0.x);
            const double2 z1 = make_double2(a1.x - b1.y, a1.y + b1.x);
            double2 z6 = make_double2(a6.x + b6.y, b6.x - a6.y);
            const double2 z7 = make_double2(a7.x + b7.y, b7.x - a7.y);
            if (!z6_ok) z6 = make_double2(0.0, 0.0);
            dft8_in4(z0, z1, z6, z7, v);
            exchange_8to6(v, u6, col6, qw, qr, twc);      // u6[t] = R_q[f0] + i R_{q+24}[f0], f0 = jc + 8 t
            // C ("8x6"): times the real spectrum, conjugate, forward transform = conj of the inverse transform
#pragma unroll
            for (int t = 0; t < 6; ++t) u6[t] = make_double2(u6[t].x * sa[t], u6[t].y * sb[t]);
            dft6(u6);
            exchange_6to8(u6, v, qw, qr, twc);            // lanes jc < 6: v[k2] = conj T[jc + 6 k2], k2 in {0, 1, 6, 7}
            if (col6) {
                double2* t0 = Tb + jc * LT + q;
                t0[0] = v[0];
                t0[6 * LT] = v[1];
                t0[12 * LT] = v[6];                       // p = jc + 36, stored at p - 24
                t0[18 * LT] = v[7];
            }
        }
        __syncthreads();
        EFGP_STAMP(FREQ_DOT ? 6 : 1);
        // D ("8x6"): row k0 >= 0 of the result, from Yh[k0] (DENSE) or from the packed columns at +k0 and -k0; conjugated inputs,
        // forward transform
        if (row_role) {
            double uAu = 0.0;
            if constexpr (DENSE) {
                // FREQ_DOT: <u, A u> and the step length in the block of D.  The 288 summands: nine per lane here, then over the 32
                // lanes (both row waves have their lanes 0..31 in this block) and the division inside the exchange.  All fifteen
                // reads go out together, the summands first.
                double pt[9];
                if constexpr (FREQ_DOT) {
                    const double* sp = s_part + (lane & 31);
#pragma unroll
                    for (int t = 0; t < 9; ++t) pt[t] = sp[32 * t];
                }
                const double2* tp = Tb + k0 * LDR + j;
#pragma unroll
                for (int t = 0; t < 6; ++t) u6[t] = tp[8 * t];
                if constexpr (FREQ_DOT) {
                    __builtin_amdgcn_sched_barrier(0);
                    double tsum = ((pt[0] + pt[1]) + (pt[2] + pt[3])) + (pt[4] + pt[5]);
                    if (VARIANT == 1) tsum /= a.sigmasq;
                    uAu = tsum + ((pt[6] + pt[7]) + pt[8]);
                }
            } else {
                const double2* tp = Tb + k0 * LT + j;
                const double2* tm = Tb + (k0 == 0 ? 0 : 2 * NR - k0) * LT + j;
#pragma unroll
                for (int u3 = 0; u3 < 3; ++u3) {
                    const double2 P = tp[8 * u3], Mv = tm[8 * u3];
                    u6[u3] = make_double2(P.x + Mv.x, P.y - Mv.y);
                    u6[u3 + 3] = make_double2(-P.y - Mv.y, P.x - Mv.x);
                }
            }
            dft6(u6);
            // lanes j < 6: v[k2] = conj Y[k0][j + 6 k2], k2 in {0, 1, 6, 7}.  FREQ_DOT: and rz / (<u, A u> + 1e-16); a warm start's
            // first application has rz = 0 and drops the value
            if constexpr (FREQ_DOT) alpha_fd = exchange_6to8_quot(u6, v, xw, xr, twr, uAu, rz);
            else exchange_6to8(u6, v, xw, xr, twr);
            const double2 y[KS] = {s64::conjd(v[0]), s64::conjd(v[1]), s64::conjd(v[6]), s64::conjd(v[7])};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const double2 gg = make_double2(wsr[s] * y[s].x, wsr[s] * y[s].y);
                double2 val;
                if (VARIANT == 0) val = make_double2(gg.x + a.sigmasq * u[s].x, gg.y + a.sigmasq * u[s].y);
                else val = make_double2(gg.x / a.sigmasq + u[s].x, gg.y / a.sigmasq + u[s].y);
                // the lanes j >= 6 of a line only lend their radix-6 stages: what they read in the radix-8 stage is stale scratch
                Au[s] = ok[s] ? val : make_double2(0.0, 0.0);
            }
        } else {
            if constexpr (FREQ_DOT) alpha_fd = 0.0;      // these lanes hold no modes: their vectors are zero and stay zero
#pragma unroll
            for (int s = 0; s < KS; ++s) Au[s] = make_double2(0.0, 0.0);
        }
        EFGP_STAMP(2);
    };

    if (tid == 0) {
        s_stop = 0;
        s_rcp = 0.0;
    }
    double2 Ap[KS];
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Ap[s] = make_double2(0.0, 0.0);
    } else {
        apply_A(xv, Ap);
    }
    double bb = 0.0, asym = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (ok[s]) {
            double2 bv = a.b[base + idx[s]];
            double2 bm = a.b[base + (M - 1 - idx[s])];                 // mode -k: must be the conjugate
            if (a.b_times_ws) {
                bv = make_double2(wsr[s] * bv.x, wsr[s] * bv.y);
                bm = make_double2(wsr[s] * bm.x, wsr[s] * bm.y);
            }
            asym += (bv.x - bm.x) * (bv.x - bm.x) + (bv.y + bm.y) * (bv.y + bm.y);
            rv[s] = csub(bv, Ap[s]);
            pv[s] = precond ? make_double2(div_rcp(rv[s].x, dg[s], rdg[s]), div_rcp(rv[s].y, dg[s], rdg[s])) : rv[s];
            rz += rv[s].x * pv[s].x + rv[s].y * pv[s].y;
            bb += bv.x * bv.x + bv.y * bv.y;
        }
    }
    rz *= wgt;
    bb *= wgt;
    block_sum_pair_h(rz, bb, red);
    asym = block_sum_h(asym, red);
    ws_bad = block_sum_h(ws_bad, red + kWavesH);      // (disjoint scratch: no barrier between the two sums' reads and writes)
    if (!(asym <= 1e-16 * bb) || ws_bad != 0.0) {
        // not the coefficients of a real function (rounding leaves ~1e-32 |b|^2): refuse loudly instead of solving another system
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (ok[s]) {
                a.x[base + idx[s]] = make_double2(__builtin_nan(""), __builtin_nan(""));
                a.x[base + (M - 1 - idx[s])] = make_double2(__builtin_nan(""), __builtin_nan(""));
            }
        }
        if (tid == 0) a.iters[row] = -2;
        return;
    }
    const double bn = sqrt(bb);
    const double den = bn > 0.0 ? bn : 1.0;
    const double den_eps = den + 1e-16, rcp_den = 1.0 / den_eps;
    // as in cg_herm64_kernel: the row waves carry the dependent chain, wave 3 (idle during A) takes the norm test of iteration i
    // and the reciprocal for the next beta; its decision is read behind the first barrier of the next operator application
    if (wave == 3 && lane == 0) s_rcp = 1.0 / (rz + 1e-16);
    int it = 0;
    for (; it < a.max_iter;) {
        apply_A(pv, Ap);
        if (stop) break;
        double alpha;
        if constexpr (FREQ_DOT) {
            alpha = alpha_fd;                             // from D straight into the updates
        } else {
            double pAp = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) pAp += pv[s].x * Ap[s].x + pv[s].y * Ap[s].y;
            pAp = block_sum_h(pAp * wgt, red) + 1e-16;
            EFGP_STAMP(3);
            alpha = rz / pAp;
        }
        double rr = 0.0, rzn = 0.0;
        double2 zv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xv[s].x += alpha * pv[s].x;
            xv[s].y += alpha * pv[s].y;
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = precond ? make_double2(div_rcp(rv[s].x, dg[s], rdg[s]), div_rcp(rv[s].y, dg[s], rdg[s])) : rv[s];
            rr += rv[s].x * rv[s].x + rv[s].y * rv[s].y;
            rzn += rv[s].x * zv[s].x + rv[s].y * zv[s].y;
        }
        rr *= wgt;
        rzn *= wgt;
        EFGP_STAMP(4);
        block_sum_pair_h(rr, rzn, red);
        EFGP_STAMP(5);
        ++it;
        if (wave == 3) {
            const double ratio = div_rcp(sqrt(rr), den_eps, rcp_den);
            const bool conv = a.early_stop && ((ratio < a.tol) || (a.batched && sqrt(rr) < 1e-12));
            if (lane == 0) {
                if (a.hist && row == 0 && it <= a.hist_cap) a.hist[it - 1] = ratio;
                s_stop = conv ? 1 : 0;
                s_rcp = 1.0 / (rzn + 1e-16);
            }
        }
        // cg.py:132 / 229: the test sits before (single) or after (batched) this update; p is not an output
        const double beta = div_rcp(rzn, rz + 1e-16, rcp_rz);
#pragma unroll
        for (int s = 0; s < KS; ++s) pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
        rz = rzn;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (ok[s]) {
            a.x[base + idx[s]] = xv[s];
            if (k0 > 0) a.x[base + (M - 1 - idx[s])] = s64::conjd(xv[s]);     // mode -k
        }
    }
    if (tid == 0) a.iters[row] = it;
}

// ------------------------------------------------------------------------------------------------
// Round 9: the single-system dense solve on EIGHT waves with paired lags (the default; EFGP_CG48_LAG_COEFFS=1 selects
// cg_herm48_kernel<.., true, true> above).  The iteration is that kernel's FREQ_DOT iteration -- A, barrier, per-frequency Toeplitz
// products, barrier, D and the updates, barrier -- with the products on waves of their own: 384 lanes (waves 2..7) instead of 192,
// four multiply-adds per (output row, input row) instead of eight (h48::pair_product).  Each role runs its own loop, selected per
// wave, so that a wave keeps only its role's state in registers: the row waves the CG vectors, the dense waves 46 doubles of
// coefficients per output row.  Every role executes the same workgroup barriers in the same order -- one behind the coefficients, two
// per operator application, one behind the sums in front of the loop, three per iteration (with ALPHA_WAVE, round 12 below: three
// per operator application, four per iteration) -- and reads s_stop behind the same one.
//
// Dense role, NOUT output rows per lane (2: waves 2-4, rows kd = 2 g, 2 g + 1; 1: waves 5-7, row kd = g + 4).  The last wave is the
// one with the least to do: it also takes the norm test and the reciprocal for the next beta (the duties of cg_herm48_kernel's idle
// wave 3).
//
// Round 10 (CHAIN_V1 false, the default; EFGP_CG48_CHAIN_V1=1 keeps the statements of round 9), the row role only: two things leave
// the dependent chain, neither changes an operation or its order.  The row lanes run x += alpha_k p_k between barriers 1 and 2 of
// application k + 1, where they wait for the dense waves, from a copy of p_k taken in the same place one application earlier; every
// way out of the loop pays what is owed.  And what the row lanes read from memory before the first residual is loaded at kernel
// entry (hrow::EarlyLoads).  The dense role is untouched: reading the stop flag together with G and branching behind the products
// was measured and dropped (profiles/r10_cg48_chain_ab.txt: no time gained).
//
// Round 12 (ALPHA_WAVE, the default; EFGP_CG48_ALPHA_ROWS=1 keeps the row lanes' statements of round 11): the sum of <u, A u> and the
// step length leave the row waves' stream.  Between barriers 2 and 3 the dense waves had nothing to do; now the one-row wave
// h48::kAlphaWaveP runs, behind barrier 2, the statements the row lanes ran inside D (h48::uAu_summands, uAu_of_lane,
// quot_half_wave: the same reads, tree and quotient, so the same bits), stores the quotient to *s_alpha, and every wave of the
// workgroup meets at one more barrier, "2b": the dense waves right behind barrier 2 (the summing wave behind its store), the row
// waves behind D's transforms, where they read the quotient.  rz: the <r,z> the row lanes hold in this application (0 in front of
// the loop).
template <int NOUT, int VARIANT, bool ALPHA_WAVE>
__device__ __forceinline__ void pairs_dense_role(const Args& a, double2* lds2, double* red, double* s_part, double* s_rcp, int* s_stop,
                                                 double* s_alpha) {
    using namespace h48;
    const double2* const Gb = lds2;
    double2* const Tb = lds2 + G_ELEMS;
    const int n = a.g.n[0];
    const int tid = threadIdx.x, lane = tid & 63, d = tid - 64 * kRowWavesP;
    const int f1d = d % F, grp = d / F, kd = NOUT == 2 ? 2 * grp : grp + 4;
    const bool duty = tid >= kThreadsP - 64;
    [[maybe_unused]] const bool sums = NOUT == 1 && tid >> 6 == kAlphaWaveP;
    PairCoeffs pc[NOUT];
    {
        const double2 wc = a.g.tw[0][((n - 1) * f1d) % F];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) pair_coeffs(lds2, wc, n, f1d, kd + o, pc[o]);
    }
    __syncthreads();                                      // the iteration's G / Yh / scratch alias the prologue's grid
#ifdef EFGP_CG_STAMPS
    long long stamp_prev = 0;
#endif
    const double2* const g0 = Gb + f1d;
    double2* const t0 = Tb + kd * LDR + f1d;
    // one operator application, as the dense lanes see it; false: the stopping decision of the last iteration was "stop"
    auto products = [&]([[maybe_unused]] double rz) __attribute__((always_inline)) -> bool {
        __syncthreads();                                  // barrier 1: G and the row lanes' shares of <u,u> are written
#ifdef EFGP_CG_STAMPS
        // slot 8: from barrier 1 until the flag and the first row of G are in the first dense lane's registers
        EFGP_STAMP_RESTART(64 * kRowWavesP);
        const int flag = *s_stop;
        if (flag) return false;
#else
        if (*s_stop) return false;
#endif
        double2 gm[NR], acc[NOUT], gk[NOUT];
#pragma unroll
        for (int m = 0; m < NR; ++m) gm[m] = g0[m * LDR];
#ifdef EFGP_CG_STAMPS
        asm volatile("" ::"v"(gm[0].x), "v"(gm[0].y), "v"(flag));
        EFGP_STAMP_BY(8, 64 * kRowWavesP);
#endif
#pragma unroll
        for (int o = 0; o < NOUT; ++o) acc[o] = pair_product(pc[o], gm);
        // G of the lane's own rows once more (kd differs between the lanes of a wave: gm[kd + o] is no register)
#pragma unroll
        for (int o = 0; o < NOUT; ++o) gk[o] = g0[(kd + o) * LDR];
        t0[0] = make_double2(acc[0].x, kd == 0 ? 0.0 : -acc[0].y);       // conj Yh: D transforms conjugated inputs
        if constexpr (NOUT == 2) t0[LDR] = make_double2(acc[1].x, -acc[1].y);
        EFGP_STAMP_BY(1, 64 * kRowWavesP);
        // Re(conj G Yh): row 0 once and from the real parts only, the others twice (rows beyond h have G = 0)
        const double t0r = kd == 0 ? gk[0].x * acc[0].x : 2.0 * fma(gk[0].y, acc[0].y, gk[0].x * acc[0].x);
        if constexpr (NOUT == 2) s_part[d] = fma(2.0, fma(gk[1].y, acc[1].y, gk[1].x * acc[1].x), t0r);
        else s_part[d] = t0r;
        __syncthreads();                                  // barrier 2: Yh and the summands of <u, A u> are written
        EFGP_STAMP_BY(6, 64 * kRowWavesP);
        if constexpr (ALPHA_WAVE) {
            if (sums) {
                double pt[15];
                uAu_summands(s_part, lane, pt);
                const double alpha = quot_half_wave(uAu_of_lane<VARIANT>(pt, a.sigmasq), rz);
                if (lane == 0) *s_alpha = alpha;
            }
            __syncthreads();                              // barrier 2b: the step length is written
        }
        return true;
    };
    if (!a.zero_x0) products(0.0);
    __syncthreads();                                      // the row waves' sums in front of the loop
    double rz = red[0] + red[4];
    const double bb = red[1] + red[5], asym = red[2] + red[6], ws_bad = red[3] + red[7];
    if (hrow::refused(asym, bb, ws_bad)) return;          // (the row lanes write the NaNs and the -2)
    const hrow::NormTest norm(bb);
    if (duty && lane == 0) *s_rcp = 1.0 / (rz + 1e-16);
    for (int it = 0; it < a.max_iter;) {
        if (!products(rz)) break;
        __syncthreads();                                  // barrier 3: the row waves' sums of <r,r> and <r,z>
        ++it;
        if (duty) norm.publish(a, red[0] + red[1], red[2] + red[3], it, lane, s_rcp, s_stop);
        if constexpr (ALPHA_WAVE) {
            if (sums) rz = red[2] + red[3];               // as the row lanes have it (RowLanes::new_direction_to)
        }
    }
}

// Register budget: 512 threads are two waves per SIMD, which an allocation of up to 256 VGPR + AGPR still admits on gfx950
// (__launch_bounds__(512) is that limit).  The two-row dense lanes are the tight role: 184 registers of coefficients, 48 of G, 8 of
// accumulators; no role may spill (scratch 0 -- profiles/r9_cg48_lag_pairs_ab.txt records the compiler's figures).
//
// Round 11 (ROW_V1 false, the default; EFGP_CG48_ROW_V1=1 keeps the row role of round 10): the row waves' instruction stream, 607
// instructions per iteration, loses the 58 that served no operation (profiles/r11_cg48_row_stream.txt).  No floating-point
// operation and no order changes:
//   * PRECOND is a template parameter (the host reads it off the arguments as RowLanes::setup does): the uniform branch around
//     the updates left phi copies of r, z and the partial sums on both of its paths;
//   * the loop's body is two iterations and p alternates between two arrays: the deferred x update reads the array the iteration
//     before ran along, so neither the copy of p nor the eight moves at the back edge are needed;
//   * the sixteen selects that zeroed A u in the slots without a mode are gone: such a slot has ws = 0 and u = 0, and what it
//     multiplies by that zero is finite once the four scratch entries per line that no stage writes are zeroed (in front of the
//     loop).  If a solve overflows, a dead slot now carries a NaN into <r,r> where the select carried a zero into a sum that was
//     not finite either;
//   * the two wave sums of <r,r> and <r,z> run with their stages interleaved (wave_sum_pair).
// Where the compiler had a choice between two contractions (the first butterflies of A, ws y + sigma^2 u in D) it chose differently
// once u was one of two arrays; those roundings are written out in the form round 10 had (dft8_in4_ws, D).
template <int VARIANT, bool FUSED = false, bool CHAIN_V1 = false, bool ROW_V1 = CHAIN_V1, bool PRECOND = true, bool ALPHA_WAVE = !ROW_V1>
__global__ __launch_bounds__(h48::kThreadsP) void cg_herm48_pairs_kernel(Args a) {
    static_assert(ROW_V1 || !CHAIN_V1, "the statements of round 9 come with round 10's loop");
    static_assert(!ALPHA_WAVE || !ROW_V1, "the step length on a dense wave comes with round 11's row role");
    using namespace h48;
    using h64::dft8_in4;
    using hrow::KS;
    extern __shared__ double2 lds2[];
    // the row waves' wave sums: [4 wave + i] in front of the loop (<r,z>, <b,b>, the two refusal sums), [wave] and [2 + wave] in the
    // iteration (<r,r>, <r,z>).  The other waves hold no modes; adding their zeros would keep the bits, so they are not added.
    __shared__ double red[4 * kRowWavesP];
    __shared__ double s_rcp;             // 1 / (<r,z> + 1e-16) for the next beta, computed by the last wave during A
    __shared__ int s_stop;               // convergence decision of the last completed iteration, taken by the last wave during A
    // the lanes' summands of <u, A u>.  [0, NDP): the Toeplitz terms of the dense lanes, written between barriers 1 and 2;
    // [NDP, NDP + 96): wgt * sigma^2 sum |u|^2 of every row lane, written in A (ALPHA_WAVE: between barriers 1 and 2).  Read behind barrier 2: by the row lanes in D, or by the summing
    // dense wave (ALPHA_WAVE).
    __shared__ double s_part[NDP + 8 * NR];
    // ALPHA_WAVE: rz / (<u, A u> + 1e-16) of the application under way, written by the dense wave h48::kAlphaWaveP between barriers
    // 2 and 2b, read by the row lanes behind barrier 2b
    __shared__ double s_alpha;
    double2* const Gb = lds2;                    // G[k0][f1], k0 = 0..11 (rows beyond h are zero), f1 = 0..47
    double2* const Tb = lds2 + G_ELEMS;          // conj Yh[k0][f1], pitch LDR
    double2* const Qb = Tb + G_ELEMS;            // the row lines' exchange scratch
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k0 = tid >> 3, j = tid & 7;

    double2 twr[5];                      // w48^(lane-in-line * t), t = 1..5 (35 at most: no wrap)
#pragma unroll
    for (int t = 1; t < 6; ++t) twr[t - 1] = a.g.tw[0][j * t];
    if (tid == 0) {
        s_stop = 0;
        s_rcp = 0.0;
    }
    // the row lanes' loads of b, the diagonal and, without FUSED, x0 and ws go out here and are used behind the prologue
    constexpr bool EARLY = !CHAIN_V1, DEFER_X = !CHAIN_V1;
    // the row lanes' shares of sigma^2 <u,u> are formed between barriers 1 and 2, where the row waves wait for the dense waves,
    // instead of in A, where they stood behind the exchange's LDS wait (profiles/r12_cg48_alpha_wave.txt)
    constexpr bool UU_GAP = ALPHA_WAVE;
    // the lanes of wave 1 without modes keep the zeros that A u and the step length have there from the start, instead of writing
    // them in every application: behind barrier 2b those nine moves stand on wave 1's chain (the arms of round 11 have them in the
    // wait between barriers 1 and 2)
    constexpr bool ZEROS_ONCE = ALPHA_WAVE;
    [[maybe_unused]] hrow::EarlyLoads<6> early;
    if constexpr (EARLY) early.template issue<FUSED>(a, tid < 8 * NR && j < 6, k0, j);
    // the operator's spectrum, made here (one pass per dimension on 64 line slots) or from memory -- the same numbers -- and one
    // inverse pass along f0: the same statements with and without FUSED
    if (FUSED) {
        vhat48_lines<kThreadsP, true>(a.vsrc, a.vL0, a.vL1, 1.0 / 2304.0, a.vhat_out, lds2);
    } else {
#pragma unroll
        for (int k = 0; k < (F * F + kThreadsP - 1) / kThreadsP; ++k) {
            const int t = tid + k * kThreadsP, i0 = t / F, i1 = t - i0 * F;
            if (t < F * F) lds2[i0 * LDV + i1] = a.vhat[t];
        }
    }
    __syncthreads();
    dense48_inverse_pass<kThreadsP>(lds2, twr);
    __syncthreads();
    if (wave >= kRowWavesP + kPairWavesP) {
        pairs_dense_role<1, VARIANT, ALPHA_WAVE>(a, lds2, red, s_part, &s_rcp, &s_stop, &s_alpha);
        return;
    }
    if (wave >= kRowWavesP) {
        pairs_dense_role<2, VARIANT, ALPHA_WAVE>(a, lds2, red, s_part, &s_rcp, &s_stop, &s_alpha);
        return;
    }

    // row role (12 lines x 8 lanes: wave 0 and half of wave 1): lane = k0 * 8 + j, the vector lives in the lanes j < 6.  From here
    // to the end the statements on these lanes are cg_herm48_kernel's, but for the summands of <u, A u> (more of them) and the
    // wave sums (two waves)
    const bool row_role = tid < 8 * NR, vec_role = row_role && j < 6;
    const int k0s = row_role ? k0 : 0;
    double2* const xw = Qb + k0s * LX + 9 * j;
    const double2* const xr = Qb + k0s * LX + j;
    hrow::RowLanes<6> L;                 // slots k1 = j, j + 6, j - 12, j - 6 of the lanes j < 6
    if constexpr (EARLY) L.template setup<FUSED, true>(a, vec_role, k0, j, &early);
    else L.template setup<FUSED>(a, vec_role, k0, j);
    const double (&wsr)[KS] = L.wsr;
    const bool (&ok)[KS] = L.ok;
    const double wgt = L.wgt;
    __syncthreads();                                      // the dense lanes have their coefficients: G / Yh / scratch may be written
    if constexpr (!ROW_V1) {
        // values 6 and 7 of the writers 6 and 7 of a line's scratch: no stage writes them, and the lanes j >= 6 read them in D
        if (row_role && j >= 6) xw[6] = xw[7] = make_double2(0.0, 0.0);
    }

#ifdef EFGP_CG_STAMPS
    long long stamp_prev = (long long)__builtin_readcyclecounter();
#endif
    int stop = 0;
    double rcp_rz = 0.0;
    double rz = 0.0;
    double alpha_fd = 0.0;               // rz / (<u, A u> + 1e-16) of the last operator application, formed inside D
    // DEFER_X: x is one update behind.  owed: x += alpha_fd * p_prev is outstanding, with alpha_fd still that of the last completed
    // application (D of the next one has not run) and p_prev the vector that application transformed
    [[maybe_unused]] bool owed = false;
    [[maybe_unused]] double2 p_prev[KS];
    // prev: the vector of the last completed application, for the x update that is owed (DEFER_X)
    // first: the application in front of the loop
    auto apply_A = [&](const double2 (&u)[KS], double2 (&Au)[KS], const double2 (&prev)[KS], auto first) __attribute__((always_inline)) {
        double2 v[8], u6[6];
        EFGP_STAMP(7);
        // A ("6x8"): rows k0 >= 0, modes k1 wrapped to positions k1 mod 48 -> G[k0][f1]
        if (row_role) {
            if constexpr (ROW_V1)
                dft8_in4(make_double2(wsr[0] * u[0].x, wsr[0] * u[0].y), make_double2(wsr[1] * u[1].x, wsr[1] * u[1].y),
                         make_double2(wsr[2] * u[2].x, wsr[2] * u[2].y), make_double2(wsr[3] * u[3].x, wsr[3] * u[3].y), v);
            else
                dft8_in4_ws<!decltype(first)::value, ALPHA_WAVE>(wsr, u, v);          // the same roundings, written out
            // u6[k2] = G[k0][j + 8 k2], and the lane's share of the sigma^2 <u,u> of <u, A u> (the slots without a mode hold zeros)
            double uu = 0.0;
            if constexpr (UU_GAP) exchange_8to6(v, u6, j < 6, xw, xr, twr);
            else uu = exchange_8to6_norm(v, u6, j < 6, xw, xr, twr, u, VARIANT == 0 ? wgt * a.sigmasq : wgt);
            double2* g0 = Gb + k0 * LDR + j;
#pragma unroll
            for (int t = 0; t < 6; ++t) g0[8 * t] = u6[t];
            if constexpr (!UU_GAP) s_part[NDP + tid] = uu;
        }
        __syncthreads();                                  // barrier 1
        stop = s_stop;
        rcp_rz = s_rcp;
        if (stop) return;                                 // uniform: the iteration that just started is abandoned
        EFGP_STAMP(0);
        if constexpr (DEFER_X) {
            // the row waves wait here for the dense waves: the x update of the last iteration, and the copy of u for the next one
            if (owed) L.update_x(alpha_fd, prev);
            owed = false;
            // (moves written out: a plain assignment is a renaming to the compiler, and the moves it then needs at the loop's back
            // edge stand behind D, on the chain)
            if constexpr (ROW_V1) {
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    asm volatile("v_mov_b64 %0, %1" : "=v"(p_prev[s].x) : "v"(u[s].x));
                    asm volatile("v_mov_b64 %0, %1" : "=v"(p_prev[s].y) : "v"(u[s].y));
                }
            }
        }
        if constexpr (UU_GAP) {
            // the share of sigma^2 <u,u> stood behind the exchange's LDS wait in A; the summing wave reads it behind barrier 2
            if (row_role) s_part[NDP + tid] = norm_share(u, VARIANT == 0 ? wgt * a.sigmasq : wgt);
        }
        __syncthreads();                                  // barrier 2: the dense waves' products (pairs_dense_role stamps them)
        EFGP_STAMP_RESTART(0);
        // D ("8x6"): row k0 >= 0 of the result from Yh[k0]; conjugated inputs, forward transform
        // A u of the lanes j < 6 from v[k2] = conj Y[k0][j + 6 k2], k2 in {0, 1, 6, 7}
        auto form_Au = [&]() __attribute__((always_inline)) {
            const double2 y[KS] = {s64::conjd(v[0]), s64::conjd(v[1]), s64::conjd(v[6]), s64::conjd(v[7])};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const double2 gg = make_double2(wsr[s] * y[s].x, wsr[s] * y[s].y);
                double2 val;
                if (VARIANT == 0) val = make_double2(gg.x + a.sigmasq * u[s].x, gg.y + a.sigmasq * u[s].y);
                else val = make_double2(gg.x / a.sigmasq + u[s].x, gg.y / a.sigmasq + u[s].y);
                // the lanes j >= 6 of a line only lend their radix-6 stages: what they read in the radix-8 stage is stale scratch
                // Without the select the compiler is free to contract the other product of VARIANT 0's sum (ws y rounded and
                // sigma^2 u fused, or the reverse); the roundings are written out as the select's form has them
                if constexpr (!ROW_V1 && VARIANT == 0)
                    Au[s] = make_double2(fma(a.sigmasq, u[s].x, __dmul_rn(wsr[s], y[s].x)), fma(a.sigmasq, u[s].y, __dmul_rn(wsr[s], y[s].y)));
                else if constexpr (!ROW_V1) Au[s] = val;
                else Au[s] = ok[s] ? val : make_double2(0.0, 0.0);
            }
        };
        if constexpr (ALPHA_WAVE) {
            // <u, A u> and the step length are the dense wave h48::kAlphaWaveP's (pairs_dense_role): the row lanes run the transforms
            // alone and meet it at barrier 2b, outside the row lanes' branch (every wave of the workgroup arrives)
            if (row_role) {
                const double2* tp = Tb + k0 * LDR + j;
#pragma unroll
                for (int t = 0; t < 6; ++t) u6[t] = tp[8 * t];
                dft6(u6);
                exchange_6to8(u6, v, xw, xr, twr);
            }
            __syncthreads();                              // barrier 2b: the step length is written
        }
        if (row_role) {
            if constexpr (ALPHA_WAVE) {
                // rz / (<u, A u> + 1e-16): the read goes out first and A u is formed under it; a warm start's first application
                // has rz = 0 and drops the value
                alpha_fd = s_alpha;
            } else {
                // <u, A u> and the step length in the block of D.  The 480 summands: fifteen per lane here, then over the 32 lanes
                // (both row waves have their lanes 0..31 in this block) and the division inside the exchange.  All twenty-one reads
                // go out together, the summands first.
                double pt[15];
                uAu_summands(s_part, lane, pt);
                const double2* tp = Tb + k0 * LDR + j;
#pragma unroll
                for (int t = 0; t < 6; ++t) u6[t] = tp[8 * t];
                __builtin_amdgcn_sched_barrier(0);
                const double uAu = uAu_of_lane<VARIANT>(pt, a.sigmasq);
                dft6(u6);
                // lanes j < 6: v[k2] = conj Y[k0][j + 6 k2], k2 in {0, 1, 6, 7}, and rz / (<u, A u> + 1e-16); a warm start's
                // first application has rz = 0 and drops the value
                alpha_fd = exchange_6to8_quot(u6, v, xw, xr, twr, uAu, rz);
            }
            form_Au();
        } else if constexpr (!ZEROS_ONCE) {
            alpha_fd = 0.0;                               // these lanes hold no modes: their vectors are zero and stay zero
#pragma unroll
            for (int s = 0; s < KS; ++s) Au[s] = make_double2(0.0, 0.0);
        }
        EFGP_STAMP(2);
    };

    double2 Ap[KS];
    if (a.zero_x0 || ZEROS_ONCE) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Ap[s] = make_double2(0.0, 0.0);
    }
    if (!a.zero_x0) apply_A(L.xv, Ap, p_prev, std::true_type{});
    double bb, asym;
    if constexpr (EARLY) L.template start<true>(a, Ap, rz, bb, asym, &early);
    else L.start(a, Ap, rz, bb, asym);
    rz = wave_sum(rz);
    bb = wave_sum(bb);
    asym = wave_sum(asym);
    double ws_bad = wave_sum(L.ws_bad);
    if (lane == 0) {
        red[4 * wave] = rz;
        red[4 * wave + 1] = bb;
        red[4 * wave + 2] = asym;
        red[4 * wave + 3] = ws_bad;
    }
    __syncthreads();                                      // the sums in front of the loop
    rz = red[0] + red[4];
    bb = red[1] + red[5];
    asym = red[2] + red[6];
    ws_bad = red[3] + red[7];
    if (hrow::refused(asym, bb, ws_bad)) {
        L.refuse(a);
        return;
    }
    int it = 0;
    if constexpr (!ROW_V1) {
        double2 p_alt[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) p_alt[s] = make_double2(0.0, 0.0);
        // one iteration along pc; the next direction goes to pn, which held the direction before pc.  false: "stop"
        auto half = [&](const double2 (&pc)[KS], double2 (&pn)[KS]) __attribute__((always_inline)) -> bool {
            apply_A(pc, Ap, pn, std::false_type{});
            if (stop) return false;
            double rr, rzn;
            double2 zv[KS];
            L.template step_<PRECOND, false>(alpha_fd, Ap, zv, rr, rzn);
            owed = true;
            EFGP_STAMP(4);
            wave_sum_pair(rr, rzn);
            if (lane == 0) {
                red[wave] = rr;
                red[2 + wave] = rzn;
            }
            __syncthreads();                              // barrier 3
            rzn = red[2] + red[3];
            EFGP_STAMP(5);
            ++it;
            L.new_direction_to(zv, rzn, rz, rcp_rz, pc, pn);
            return true;
        };
        bool owed_alt = false;
        // the loop's body is two iterations, so that the two arrays swap their names instead of their contents.  owed_alt: the last
        // completed iteration ran along p_alt
        for (;;) {
            owed_alt = true;
            if (it >= a.max_iter || !half(L.pv, p_alt)) break;
            owed_alt = false;
            if (it >= a.max_iter || !half(p_alt, L.pv)) break;
        }
        // the update of the last completed iteration: the loop ended at max_iter, or on "stop" behind barrier 1, in front of D
        if (owed) L.update_x(alpha_fd, owed_alt ? p_alt : L.pv);
        L.write_out(a, it);
        return;
    }
    for (; it < a.max_iter;) {
        apply_A(L.pv, Ap, p_prev, std::false_type{});
        if (stop) break;
        double rr, rzn;
        double2 zv[KS];
        if constexpr (DEFER_X) {
            L.template step<false>(alpha_fd, Ap, zv, rr, rzn);
            owed = true;
        } else {
            L.step(alpha_fd, Ap, zv, rr, rzn);            // alpha from D straight into the updates
        }
        EFGP_STAMP(4);
        rr = wave_sum(rr);
        rzn = wave_sum(rzn);
        if (lane == 0) {
            red[wave] = rr;
            red[2 + wave] = rzn;
        }
        __syncthreads();                                  // barrier 3
        rzn = red[2] + red[3];
        EFGP_STAMP(5);
        ++it;
        L.new_direction(zv, rzn, rz, rcp_rz);
    }
    if constexpr (DEFER_X) {
        // the update of the last completed iteration: the loop ended at max_iter, or on "stop" behind barrier 1, in front of D
        if (owed) L.update_x(alpha_fd, p_prev);
    }
    L.write_out(a, it);
}

// the 48 x 48 kernels: the operator's second spectrum and twiddles; the fused mean solve makes ws and that spectrum itself
static void operands48(const Herm48Operands& h48, const MeanFusedOperands* fuse, Args& a) {
    a.vhat = fuse ? nullptr : h48.vhat;
    a.g.F[0] = a.g.F[1] = 48;
    a.g.tw[0] = a.g.tw[1] = h48.tw;
    if (!fuse) return;
    a.ws = nullptr;
    a.wk_kind = fuse->kind;
    a.wk_mtot = fuse->mtot;
    a.wk_nu = fuse->nu;
    a.wk_ell = fuse->ell;
    a.wk_c0 = fuse->c0;
    a.wk_h = fuse->h;
    a.ws_out = fuse->ws_out;
    a.vsrc = fuse->v;
    a.vL0 = fuse->L0;
    a.vL1 = fuse->L1;
    a.vhat_out = fuse->vhat48_out;
}

PickLaunch herm_launch(const PersistentChoice& c, int variant, const Herm48Operands* h48, const MeanFusedOperands* fuse, Args& a) {
    if (c.pick == PersistentPick::fused48 || c.pick == PersistentPick::herm48) operands48(*h48, fuse, a);
    // 48 x 48: the coefficient prologue works on the 48 x 48 grid, 73 KB (two workgroups per CU still fit); the fused prologue's
    // grid + 32 line slots of scratch outgrow the iteration's 53 KB too -- one workgroup, so the extra LDS costs nothing
    constexpr size_t lds48d = (size_t)h48::kLdsElemsDense * sizeof(double2);
    static_assert(h48::kLdsElemsDense >= h48::kLdsElems, "the fused prologue's LDS covers the iteration's");
    // EFGP_CG48_MODE_DOT=1 (read per call): the dense 48 x 48 kernels sum <p,Ap> over the modes behind D (the round 6 iteration, four
    // barriers) instead of forming it in the row-frequency domain (round 7, three)
    const bool freq_dot = std::getenv("EFGP_CG48_MODE_DOT") == nullptr;
    // EFGP_CG48_LAG_COEFFS=1 (read per call): a single dense system runs on the 256-thread kernels with 25 resident lags (rounds 6 / 7)
    // instead of the eight waves with paired lags (round 9).  EFGP_CG48_MODE_DOT=1 is an iteration of the 256-thread kernels only.
    const bool pairs = c.dense48 && freq_dot && std::getenv("EFGP_CG48_LAG_COEFFS") == nullptr;
    constexpr size_t lds48p = (size_t)h48::kLdsElemsPairs * sizeof(double2);
    // EFGP_CG48_CHAIN_V1=1 (read per call): the eight-wave kernel with the x update inside the iteration's chain and the row lanes'
    // loads behind the prologue (round 9) instead of off the chain (round 10); equal bits
    const bool chain_v1 = std::getenv("EFGP_CG48_CHAIN_V1") != nullptr;
    // EFGP_CG48_ROW_V1=1 (read per call): the row role's loop of round 10 (one iteration per pass, a copy of p, the preconditioner's
    // branch and the selects inside it) instead of round 11's; equal bits.  EFGP_CG48_CHAIN_V1=1 implies it.
    // The default arm has the preconditioner's choice as a template parameter (RowLanes::setup's `precond`).
    // EFGP_CG48_ALPHA_ROWS=1 (read per call): the default row role sums <u, A u> and forms the step length itself, inside D (round 11),
    // instead of reading it from a dense wave behind barrier 2b (round 12); equal bits.  The other two switches' arms never had the
    // dense wave's sum and do not see this one.
    const bool alpha_rows = std::getenv("EFGP_CG48_ALPHA_ROWS") != nullptr;
    const int arm =
        chain_v1 ? 3 : (std::getenv("EFGP_CG48_ROW_V1") != nullptr ? 2 : (hrow::has_precond(a) ? 0 : 1) + (alpha_rows ? 4 : 0));
    // the launch's label names the arm (efgp_cg_last_launch reports it: the tests of the switches read it)
    static const char* const fused8[6] = {"fused mean solve (48x48, eight waves)",
                                          "fused mean solve (48x48, eight waves, no diagonal)",
                                          "fused mean solve (48x48, eight waves, row role of round 10)",
                                          "fused mean solve (48x48, eight waves, round 9)",
                                          "fused mean solve (48x48, eight waves, step length on the row waves)",
                                          "fused mean solve (48x48, eight waves, no diagonal, step length on the row waves)"};
    static const char* const herm8[6] = {"persistent CG (48x48, Hermitian, eight waves)",
                                         "persistent CG (48x48, Hermitian, eight waves, no diagonal)",
                                         "persistent CG (48x48, Hermitian, eight waves, row role of round 10)",
                                         "persistent CG (48x48, Hermitian, eight waves, round 9)",
                                         "persistent CG (48x48, Hermitian, eight waves, step length on the row waves)",
                                         "persistent CG (48x48, Hermitian, eight waves, no diagonal, step length on the row waves)"};
    switch (c.pick) {
        case PersistentPick::fused48: {
            if (pairs) {
                void (*const eight[6])(Args) = {cg_herm48_pairs_kernel<0, true>,
                                                cg_herm48_pairs_kernel<0, true, false, false, false>,
                                                cg_herm48_pairs_kernel<0, true, false, true>,
                                                cg_herm48_pairs_kernel<0, true, true>,
                                                cg_herm48_pairs_kernel<0, true, false, false, true, false>,
                                                cg_herm48_pairs_kernel<0, true, false, false, false, false>};
                return {eight[arm], h48::kThreadsP, lds48p, fused8[arm]};
            }
            void (*const dense[2])(Args) = {cg_herm48_kernel<0, true, true, false>, cg_herm48_kernel<0, true, true, true>};
            return {c.dense48 ? dense[freq_dot] : cg_herm48_kernel<0, true, false>, h48::kThreadsH, lds48d, "fused mean solve (48x48)"};
        }
        case PersistentPick::herm48: {
            if (pairs) {
                void (*const eight[6][2])(Args) = {
                    {cg_herm48_pairs_kernel<0>, cg_herm48_pairs_kernel<1>},
                    {cg_herm48_pairs_kernel<0, false, false, false, false>, cg_herm48_pairs_kernel<1, false, false, false, false>},
                    {cg_herm48_pairs_kernel<0, false, false, true>, cg_herm48_pairs_kernel<1, false, false, true>},
                    {cg_herm48_pairs_kernel<0, false, true>, cg_herm48_pairs_kernel<1, false, true>},
                    {cg_herm48_pairs_kernel<0, false, false, false, true, false>, cg_herm48_pairs_kernel<1, false, false, false, true, false>},
                    {cg_herm48_pairs_kernel<0, false, false, false, false, false>, cg_herm48_pairs_kernel<1, false, false, false, false, false>}};
                return {eight[arm][variant != 0], h48::kThreadsP, lds48p, herm8[arm]};
            }
            void (*const dense[2][2])(Args) = {{cg_herm48_kernel<0, false, true, false>, cg_herm48_kernel<1, false, true, false>},
                                               {cg_herm48_kernel<0, false, true, true>, cg_herm48_kernel<1, false, true, true>}};
            void (*const fft2d[2])(Args) = {cg_herm48_kernel<0, false, false>, cg_herm48_kernel<1, false, false>};
            return {(c.dense48 ? dense[freq_dot] : fft2d)[variant != 0], h48::kThreadsH,
                    c.dense48 ? lds48d : (size_t)h48::kLdsElems * sizeof(double2), "persistent CG (48x48, Hermitian)"};
        }
        default:
            break;
    }
    // PersistentPick::herm64
    return {variant == 0 ? cg_herm64_kernel<0> : cg_herm64_kernel<1>, h64::kThreadsH, (size_t)h64::kLdsElems * sizeof(double2),
            "persistent CG (64x64, Hermitian)"};
}

}  // namespace pcg

}  // namespace efgp
