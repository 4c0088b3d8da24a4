// Persistent fused CG: one workgroup solves one system completely inside ONE kernel launch.
//
// For the headline configuration (d=2, mtot=23 -> Toeplitz FFT 64x64) the whole circulant grid is
// 64 KB, so the entire CG iteration (cg.py:116-150 / :193-241) -- diagonal scaling, zero padding,
// forward FFT, spectral multiply, inverse FFT, crop, <p,Ap>, x/r updates, norms, preconditioner,
// p update, convergence test -- runs out of LDS and registers with no launch, no HBM round trip and
// no host involvement per iteration.  Batched solves map one system per workgroup (grid = rows).
//
// LDS layout: two ping-pong buffers of the padded grid (Stockham autosort FFT, radix 8/4/2 stages);
// the fastest dimension is padded by one complex element so that lines of the other dimensions are
// conflict-free across lanes.  FFT passes are pruned: only lines that can be non-zero are
// transformed forward (the operand occupies the leading n-box), and the inverse passes only produce
// the [n-1, 2n-1) window that the Toeplitz product keeps (efgpnd.py:1289-1290).
//
// Eligibility (checked on the host): every FFT length a power of two, padded grid <= kMaxGrid
// complex elements, M <= kSlots * kThreads.
#include <cmath>
#include <cstdlib>

#include "cg_persistent_dev.hpp"

namespace efgp {

namespace pcg {

// kThreads, kSlots, kMaxGrid and l1d::KS: cg_plan_host.hpp (the host's planners use them too)
constexpr int kRedWaves = kThreads / 64;

// Pass, Geom, Args, the stamps, the complex helpers, dft_fwd, wave_sum and jacobi_entry: cg_persistent_dev.hpp

// eight named registers with a compile-time accessor (a plain array here ends up in scratch memory)
struct V8 {
    double2 a0, a1, a2, a3, a4, a5, a6, a7;
};
template <int T>
__device__ __forceinline__ double2& v8(V8& v) {
    if constexpr (T == 0) return v.a0;
    else if constexpr (T == 1) return v.a1;
    else if constexpr (T == 2) return v.a2;
    else if constexpr (T == 3) return v.a3;
    else if constexpr (T == 4) return v.a4;
    else if constexpr (T == 5) return v.a5;
    else if constexpr (T == 6) return v.a6;
    else return v.a7;
}
template <int T, int R>
__device__ __forceinline__ void spectral_mul_regs(double2 (&v)[R], V8& sp) {
    if constexpr (T < R) {
        double2 val = cmulp(v[T], v8<T>(sp));
        val.y = -val.y;
        v[T] = val;
        spectral_mul_regs<T + 1, R>(v, sp);
    }
}
template <int T, int R>
__device__ __forceinline__ void spectral_load_regs(V8& sp, const double2* __restrict__ vhat, int idx0, int step) {
    if constexpr (T < R) {
        v8<T>(sp) = vhat[idx0 + T * step];
        spectral_load_regs<T + 1, R>(sp, vhat, idx0, step);
    }
}

// One Stockham stage of radix R over all lines of a pass.  INV: inverse transform (conjugate trick).
// `first`/`last` select the pruning predicates.  MID (forward only): this is the last stage of the last
// forward pass; its outputs are multiplied by the spectrum `vreg` (held in registers, one butterfly per
// thread) and immediately pushed through the FIRST inverse stage of the same dimension (same radix,
// Ns = 1, no twiddles: the outputs k + t*n/R of the forward stage are exactly the inputs of that
// inverse stage), saving one LDS round trip per iteration.
template <int R, bool INV, bool MID>
__device__ __forceinline__ void stage(const Geom& g, const Pass& p, int Ns, int ns_log2, bool first, bool last,
                                      const double2* __restrict__ src, double2* __restrict__ dst,
                                      const double2* __restrict__ tw, const double2* __restrict__ vhat, V8& sp,
                                      bool use_sp) {
    const int n = p.n;
    const int nb = n / R;                                  // butterflies per line
    const int w0 = p.hi[0] - p.lo[0], w1 = p.hi[1] - p.lo[1];
    const int pstride = p.pstride;
    const int s0 = p.s0, s1 = p.s1;
    const int tw_step = n / (Ns * R);
    const int items = nb << p.lines_log2;
    const int lmask = (1 << p.lines_log2) - 1, w1mask = (1 << p.w1_log2) - 1;
    for (int item = threadIdx.x; item < items; item += kThreads) {
        const int line = item & lmask;                     // lines vary fastest across lanes
        const int j = item >> p.lines_log2;
        const int c1r = line & w1mask, c0r = line >> p.w1_log2;
        if (c1r >= w1 || c0r >= w0) continue;
        const int c1 = p.lo[1] + c1r, c0 = p.lo[0] + c0r;
        const int base = c0 * s0 + c1 * s1;
        const int k = j & (Ns - 1);
        double2 v[R];
        const int a_in = base + j * pstride, in_step = nb * pstride, tw_k = k * tw_step;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            double2 val = make_double2(0.0, 0.0);
            if (!first || j + t * nb < p.in_limit) val = src[a_in + t * in_step];
            if (INV) val.y = -val.y;
            if (t > 0 && Ns > 1) val = cmulp(val, tw[t * tw_k]);
            v[t] = val;
        }
        dft_fwd<R>(v);
        if (MID) {
            // spectral multiply, then the first inverse stage (Ns = 1) on the same R values
            if (use_sp) {
                spectral_mul_regs<0, R>(v, sp);
            } else {
                const int i0 = ((j - k) * R + k) * p.vs_pos + c0 * p.vs_c0 + c1 * p.vs_c1, istep = Ns * p.vs_pos;
#pragma unroll
                for (int t = 0; t < R; ++t) {
                    double2 val = cmulp(v[t], vhat[i0 + t * istep]);
                    val.y = -val.y;                        // conj in
                    v[t] = val;
                }
            }
            dft_fwd<R>(v);
            // inverse stage 0 writes position j*R + t; if it is also the last inverse stage of the pass
            // (single-stage FFT) the crop window applies
            const bool only = p.nstages == 1;
            const int a_out = base + j * R * pstride;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const int pos = j * R + t;
                if (only && (pos < p.in_limit - 1 || pos >= 2 * p.in_limit - 1)) continue;   // in_limit == n[dim] (forward pass)
                double2 val = v[t];
                val.y = -val.y;                            // conj out
                dst[a_out + t * pstride] = val;
            }
            continue;
        }
        const int ob = (j - k) * R + k;
        const int a_out = base + ob * pstride, out_step = Ns * pstride;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int pos = ob + t * Ns;
            if (last && (pos < p.out_lo || pos >= p.out_hi)) continue;
            double2 val = v[t];
            if (INV) val.y = -val.y;
            if (vhat) val = cmulp(val, vhat[pos * p.vs_pos + c0 * p.vs_c0 + c1 * p.vs_c1]);
            dst[a_out + t * out_step] = val;
        }
    }
}

// runs the stages [s_begin, s_end) of a pass
template <bool INV>
__device__ __forceinline__ void run_pass(const Geom& g, const Pass& p, int s_begin, int s_end, double2*& cur,
                                         double2*& alt, const double2* tw, const double2* vhat_last, bool mid_last,
                                         V8& sp, bool use_sp) {
    int Ns = 1, lg = 0;
    for (int s = 0; s < s_begin; ++s) {
        Ns *= p.radix[s];
        lg += p.radix[s] == 8 ? 3 : (p.radix[s] == 4 ? 2 : 1);
    }
    for (int s = s_begin; s < s_end; ++s) {
        const bool first = s == 0, last = s == p.nstages - 1;
        const double2* vh = (last && !mid_last ? vhat_last : nullptr);
        const bool mid = last && mid_last && !INV;
        if (mid) {
            switch (p.radix[s]) {
                case 8: stage<8, false, true>(g, p, Ns, lg, first, last, cur, alt, tw, vhat_last, sp, use_sp); break;
                case 4: stage<4, false, true>(g, p, Ns, lg, first, last, cur, alt, tw, vhat_last, sp, use_sp); break;
                default: stage<2, false, true>(g, p, Ns, lg, first, last, cur, alt, tw, vhat_last, sp, use_sp); break;
            }
        } else {
            switch (p.radix[s]) {
                case 8: stage<8, INV, false>(g, p, Ns, lg, first, last, cur, alt, tw, vh, sp, false); break;
                case 4: stage<4, INV, false>(g, p, Ns, lg, first, last, cur, alt, tw, vh, sp, false); break;
                default: stage<2, INV, false>(g, p, Ns, lg, first, last, cur, alt, tw, vh, sp, false); break;
            }
        }
        Ns *= p.radix[s];
        lg += p.radix[s] == 8 ? 3 : (p.radix[s] == 4 ? 2 : 1);
        __syncthreads();
        double2* t = cur;
        cur = alt;
        alt = t;
    }
}

// Block reductions.  The single sum and the pair use DISJOINT scratch (red[2*kRedWaves ..] vs red[0 ..]), and a
// scratch region is rewritten only after other barriers have passed since its last read (the other reduction
// and the FFT phases sit in between), so no barrier is needed in front of the writes.
__device__ __forceinline__ double block_sum2(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double* r1 = red + 2 * kRedWaves;
    if (lane == 0) r1[wid] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < kRedWaves; ++i) t += r1[i];
    return t;
}

// two sums with one barrier
__device__ __forceinline__ void block_sum_pair(double& u, double& v, double* red) {
    u = wave_sum(u);
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        red[wid] = u;
        red[kRedWaves + wid] = v;
    }
    __syncthreads();
    double t = 0.0, w = 0.0;
#pragma unroll
    for (int i = 0; i < kRedWaves; ++i) {
        t += red[i];
        w += red[kRedWaves + i];
    }
    u = t;
    v = w;
}

// flat block index -> offset in the padded grid, optionally shifted by (n-1) per dimension
__device__ __forceinline__ int grid_offset(const Geom& g, int flat, int shift) {
    int off = 0;
    for (int a = g.d - 1; a >= 0; --a) {
        const int ia = flat % g.n[a];
        flat /= g.n[a];
        off += (ia + shift * (g.n[a] - 1)) * g.ld[a];
    }
    return off;
}

// Lanczos three-term recurrence inside the persistent kernels (shared by both): no launch and no host round trip per step
// (the host loop it replaces made two device->host reads per step: 100 probes x 25 steps x 2 at the defaults).
#define EFGP_LANCZOS_BRANCH(NS_, TID_)                                                                          \
    if (a.lz_steps > 0) {                                                                                       \
        double2 q[NS_], qp[NS_], vv[NS_];                                                                       \
        double nb = 0.0;                                                                                        \
        _Pragma("unroll") for (int s = 0; s < NS_; ++s) {                                                       \
            const int t = TID_ + s * kThreads;                                                                  \
            q[s] = t < M ? a.b[base + t] : make_double2(0.0, 0.0);                                              \
            qp[s] = make_double2(0.0, 0.0);                                                                     \
            nb += q[s].x * q[s].x + q[s].y * q[s].y;                                                            \
        }                                                                                                       \
        nb = block_sum2(nb, red);                                                                               \
        const double inv_nb = nb > 0.0 ? 1.0 / sqrt(nb) : 0.0;                                                  \
        _Pragma("unroll") for (int s = 0; s < NS_; ++s) q[s] = make_double2(q[s].x * inv_nb, q[s].y * inv_nb);  \
        double beta_prev = 0.0;                                                                                 \
        int k = 0;                                                                                              \
        while (k < a.lz_steps) {                                                                                \
            apply_A(q, vv);                                                                                     \
            double al = 0.0;                                                                                    \
            _Pragma("unroll") for (int s = 0; s < NS_; ++s) {                                                   \
                vv[s].x -= beta_prev * qp[s].x;                                                                 \
                vv[s].y -= beta_prev * qp[s].y;                                                                 \
                al += q[s].x * vv[s].x + q[s].y * vv[s].y;                                                      \
            }                                                                                                   \
            al = block_sum2(al, red);                                                                           \
            double bt = 0.0, unused = 0.0;                                                                      \
            _Pragma("unroll") for (int s = 0; s < NS_; ++s) {                                                   \
                vv[s].x -= al * q[s].x;                                                                         \
                vv[s].y -= al * q[s].y;                                                                         \
                bt += vv[s].x * vv[s].x + vv[s].y * vv[s].y;                                                    \
            }                                                                                                   \
            block_sum_pair(bt, unused, red);                                                                    \
            bt = sqrt(bt);                                                                                      \
            if (TID_ == 0) {                                                                                    \
                a.lz_alpha[(int64_t)row * a.lz_steps + k] = al;                                                 \
                a.lz_beta[(int64_t)row * a.lz_steps + k] = bt;                                                  \
            }                                                                                                   \
            ++k;                                                                                                \
            if (bt < 1e-12) break;                                                                              \
            const double ib = 1.0 / bt;                                                                         \
            _Pragma("unroll") for (int s = 0; s < NS_; ++s) {                                                   \
                qp[s] = q[s];                                                                                   \
                q[s] = make_double2(vv[s].x * ib, vv[s].y * ib);                                                \
            }                                                                                                   \
            beta_prev = bt;                                                                                     \
        }                                                                                                       \
        if (TID_ == 0) {                                                                                        \
            a.iters[row] = k;                                                                                   \
            if (a.lz_norm2) a.lz_norm2[row] = nb;                                                               \
        }                                                                                                       \
        return;                                                                                                 \
    }

__global__ __launch_bounds__(kThreads) void cg_persistent_kernel(Args a) {
    extern __shared__ double2 lds2[];
    __shared__ double red[3 * kRedWaves];
    const Geom& g = a.g;
    double2* bufA = lds2;
    double2* bufB = lds2 + g.padded;
    // twiddle tables: LDS copies (when they fit behind the two buffers) are filled once
    double2* tw_lds_base = lds2 + 2 * g.padded;
    for (int a_ = 0; a_ < g.d; ++a_) {
        if (g.tw_lds_off[a_] < 0) continue;
        bool dup = false;
        for (int b_ = 0; b_ < a_; ++b_) dup = dup || (g.tw_lds_off[b_] == g.tw_lds_off[a_]);
        if (!dup)
            for (int q = threadIdx.x; q < g.F[a_]; q += kThreads) tw_lds_base[g.tw_lds_off[a_] + q] = g.tw[a_][q];
    }
    const int row = blockIdx.x;
    const int M = g.M;
    const int64_t base = (int64_t)row * M;

    // per-thread slices of the vectors (element t lives in thread t % kThreads, slot t / kThreads)
    double2 xv[kSlots], rv[kSlots], pv[kSlots], wsv[kSlots];
    double dg[kSlots];
    const bool precond = a.diag != nullptr || a.diag_scale != nullptr;
    int off_in[kSlots], off_out[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int t = threadIdx.x + s * kThreads;
        if (t < M) {
            xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x0[base + t];
            wsv[s] = a.ws[t];
            dg[s] = jacobi_entry(a, wsv[s], t);
            off_in[s] = grid_offset(g, t, 0);
            off_out[s] = grid_offset(g, t, 1);
        } else {
            xv[s] = wsv[s] = make_double2(0.0, 0.0);
            dg[s] = 1.0;
            off_in[s] = off_out[s] = 0;
        }
        rv[s] = pv[s] = make_double2(0.0, 0.0);
    }

    // spectrum values of this thread's butterfly in the fused middle stage (when it has one item per thread)
    V8 sp;
    sp.a0 = sp.a1 = sp.a2 = sp.a3 = sp.a4 = sp.a5 = sp.a6 = sp.a7 = make_double2(0.0, 0.0);
    bool use_sp = false;
    {
        const Pass& pm = g.fwd[g.npass - 1];
        const int R = pm.radix[pm.nstages - 1];
        const int nb = pm.n / R;
        const int items = nb << pm.lines_log2;
        use_sp = g.fuse_mid && items <= kThreads;
        if (use_sp && (int)threadIdx.x < items) {
            const int line = threadIdx.x & ((1 << pm.lines_log2) - 1);
            const int j = threadIdx.x >> pm.lines_log2;
            const int c1r = line & ((1 << pm.w1_log2) - 1), c0r = line >> pm.w1_log2;
            if (c1r < pm.hi[1] - pm.lo[1] && c0r < pm.hi[0] - pm.lo[0]) {
                const int k = j & (nb - 1);          // last stage: Ns = n / R = nb
                const int i0 = ((j - k) * R + k) * pm.vs_pos + (pm.lo[0] + c0r) * pm.vs_c0 + (pm.lo[1] + c1r) * pm.vs_c1;
                const int istep = nb * pm.vs_pos;
                if (R == 8) spectral_load_regs<0, 8>(sp, a.vhat, i0, istep);
                else if (R == 4) spectral_load_regs<0, 4>(sp, a.vhat, i0, istep);
                else spectral_load_regs<0, 2>(sp, a.vhat, i0, istep);
            }
        }
    }
    __syncthreads();      // twiddle copies visible

    // A u for this thread's slots: u -> LDS -> pruned FFT -> .* vhat -> pruned inverse FFT -> crop
#ifdef EFGP_CG_STAMPS
    long long stamp_prev = (long long)__builtin_readcyclecounter();
#endif
    auto apply_A = [&](const double2 (&u)[kSlots], double2 (&Au)[kSlots]) __attribute__((always_inline)) {
        EFGP_STAMP(7);
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int t = threadIdx.x + s * kThreads;
            if (t < M) bufA[off_in[s]] = cmulp(wsv[s], u[s]);
        }
        __syncthreads();
        EFGP_STAMP(0);
        double2* cur = bufA;
        double2* alt = bufB;
        for (int q = 0; q < g.npass; ++q) {
            const bool lastp = q == g.npass - 1;
            const Pass& pf = g.fwd[q];
            run_pass<false>(g, pf, 0, pf.nstages, cur, alt, pf.tw_lds >= 0 ? tw_lds_base + pf.tw_lds : pf.tw_glob,
                            lastp ? a.vhat : nullptr, lastp && g.fuse_mid, sp, use_sp);
            EFGP_STAMP(1 + q);
        }
        for (int q = 0; q < g.npass; ++q) {   // with the fused middle stage, inverse pass 0 starts at its stage 1
            const Pass& pi = g.inv[q];
            run_pass<true>(g, pi, (q == 0 && g.fuse_mid) ? 1 : 0, pi.nstages, cur, alt,
                           pi.tw_lds >= 0 ? tw_lds_base + pi.tw_lds : pi.tw_glob, nullptr, false, sp, false);
            EFGP_STAMP(4 + q);
        }
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int t = threadIdx.x + s * kThreads;
            if (t < M) {
                double2 Tu = cur[off_out[s]];
                double2 gg = cmulp(wsv[s], Tu);
                if (a.variant == 0) Au[s] = make_double2(gg.x + a.sigmasq * u[s].x, gg.y + a.sigmasq * u[s].y);
                else Au[s] = make_double2(gg.x / a.sigmasq + u[s].x, gg.y / a.sigmasq + u[s].y);
            } else {
                Au[s] = make_double2(0.0, 0.0);
            }
        }
        __syncthreads();     // the buffers are reused by the next application
        EFGP_STAMP(8);
    };

    EFGP_LANCZOS_BRANCH(kSlots, (int)threadIdx.x)

    // r = b - A x0, z = r / diag, p = z
    double2 Ap[kSlots];
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < (int)(sizeof(Ap) / sizeof(Ap[0])); ++s) Ap[s] = make_double2(0.0, 0.0);
    } else {
        apply_A(xv, Ap);
    }
    double rz = 0.0, bb = 0.0;
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int t = threadIdx.x + s * kThreads;
        if (t < M) {
            double2 bv = a.b[base + t];
            if (a.b_times_ws) bv = cmulp(wsv[s], bv);
            rv[s] = csub(bv, Ap[s]);
            pv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            rz += rv[s].x * pv[s].x + rv[s].y * pv[s].y;
            bb += bv.x * bv.x + bv.y * bv.y;
        }
    }
    block_sum_pair(rz, bb, red);
    const double bn = sqrt(bb);
    const double den = bn > 0.0 ? bn : 1.0;

    int it = 0;
    for (; it < a.max_iter;) {
        apply_A(pv, Ap);
        double pAp = 0.0;
#pragma unroll
        for (int s = 0; s < kSlots; ++s) pAp += pv[s].x * Ap[s].x + pv[s].y * Ap[s].y;
        pAp = block_sum2(pAp, red) + 1e-16;
        const double alpha = rz / pAp;
        double rr = 0.0, rzn = 0.0;
        double2 zv[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            xv[s].x += alpha * pv[s].x;
            xv[s].y += alpha * pv[s].y;
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            rr += rv[s].x * rv[s].x + rv[s].y * rv[s].y;
            rzn += rv[s].x * zv[s].x + rv[s].y * zv[s].y;
        }
        block_sum_pair(rr, rzn, red);
        ++it;
        const double rnorm = sqrt(rr);
        if (a.hist && row == 0 && threadIdx.x == 0 && it <= a.hist_cap) a.hist[it - 1] = rnorm / (den + 1e-16);
        const bool conv = a.early_stop && ((rnorm / (den + 1e-16) < a.tol) || (a.batched && rnorm < 1e-12));
        if (!a.batched && conv) break;                  // cg.py:132 (before the preconditioner / p update)
        const double beta = rzn / (rz + 1e-16);
#pragma unroll
        for (int s = 0; s < kSlots; ++s) pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
        rz = rzn;
        if (conv) break;                                // cg.py:229-241 (after the p update)
    }
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int t = threadIdx.x + s * kThreads;
        if (t < M) a.x[base + t] = xv[s];
    }
    if (threadIdx.x == 0) a.iters[row] = it;
}

// ------------------------------------------------------------------------------------------------
// Specialised kernel for the headline shape: d = 2, circulant grid 64 x 64 (mtot <= 32), radix-8
// Stockham stages with compile-time strides.  All addresses, twiddles and the thread's slice of the
// spectrum are computed once, outside the CG loop; a stage is 8 ds_read_b128 + ~100 fp64 ops +
// 8 ds_write_b128 with immediate offsets.  Same arithmetic as the generic kernel above.
// ------------------------------------------------------------------------------------------------
// (namespace s64, its constants and radix-8 helpers: cg_persistent_dev.hpp)
__global__ __launch_bounds__(kThreads) void cg_persistent_2d64_kernel(Args a) {
    using namespace s64;
    // Row pitch 72 (not s64::LD = 65): the eight butterflies of a row sit in EIGHT ADJACENT LANES of one wave (lane = row * 8 + j),
    // so that both radix-8 stages of a row transform run inside that wave with only a wave-level fence between them (no
    // workgroup barrier: 2 of the 10 barriers per iteration gone, and the three row waves no longer wait for each other).
    // With that lane map a 16-lane LDS group covers two rows x eight j: pitch = 8 mod 16 (in 16-byte elements) puts them on
    // 16 distinct slots.  Column passes read 64 consecutive elements per wave: conflict free at any pitch.
    constexpr int LD = 72, BUF = F * LD;
    constexpr int KS = 2;                   // M = n*n <= 1024 = KS * kThreads
    extern __shared__ double2 lds2[];
    __shared__ double red[3 * kRedWaves];
    double2* const bufA = lds2;
    double2* const bufB = lds2 + BUF;
    const int n = a.g.n[0];                 // block size per dimension (n0 == n1 for this kernel)
    const int M = a.g.M;
    const int row = blockIdx.x;
    const int64_t base = (int64_t)row * M;
    const int tid = threadIdx.x;

    // ---- iteration-invariant per-thread data -------------------------------------------------
    // row passes: lane = row * 8 + butterfly (rows 8w..8w+7 in wave w); column passes: 64 columns x 8 (all threads)
    const int j_row = tid & 7, r_row = tid >> 3;
    const bool row_act = r_row < n;
    const int c_col = tid & 63, j_col = tid >> 6;
    // valid leading inputs of the pruned first stages: positions j + 8t < n
    const int nv_row = j_row < n ? (n - 1 - j_row) / 8 + 1 : 0;
    const int nv_col = j_col < n ? (n - 1 - j_col) / 8 + 1 : 0;
    // crop window [n-1, 2n-1) masks of the pruned last inverse stages: position j + 8t
    unsigned keep_col = 0, keep_row = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int pc = j_col + 8 * t, pr = j_row + 8 * t;
        if (pc >= n - 1 && pc < 2 * n - 1) keep_col |= 1u << t;
        if (pr >= n - 1 && pr < 2 * n - 1) keep_row |= 1u << t;
    }
    double2 twr[7], twc[7], spec[8];
#pragma unroll
    for (int t = 1; t < 8; ++t) {
        twr[t - 1] = a.g.tw[0][(j_row & 7) * t];
        twc[t - 1] = a.g.tw[0][j_col * t];
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) spec[t] = a.vhat[(j_col + 8 * t) * F + c_col];

    double2 xv[KS], rv[KS], pv[KS], wsv[KS];
    double dg[KS];
    const bool precond = a.diag != nullptr || a.diag_scale != nullptr;
    int off_in[KS], off_out[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = tid + s * kThreads;
        if (t < M) {
            xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x0[base + t];
            wsv[s] = a.ws[t];
            dg[s] = jacobi_entry(a, wsv[s], t);
            const int i0 = t / n, i1 = t - i0 * n;
            off_in[s] = i0 * LD + i1;
            off_out[s] = (i0 + n - 1) * LD + (i1 + n - 1);
        } else {
            xv[s] = wsv[s] = make_double2(0.0, 0.0);
            dg[s] = 1.0;
            off_in[s] = off_out[s] = 0;
        }
        rv[s] = pv[s] = make_double2(0.0, 0.0);
    }
#ifdef EFGP_CG_STAMPS
    long long stamp_prev = (long long)__builtin_readcyclecounter();
#endif

    auto apply_A = [&](const double2 (&u)[KS], double2 (&Au)[KS]) __attribute__((always_inline)) {
        EFGP_STAMP(7);
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (tid + s * kThreads < M) bufA[off_in[s]] = cmulp(wsv[s], u[s]);
        __syncthreads();
        EFGP_STAMP(0);
        double2 v[8];
        // P1/P2: forward FFT along dim 1 of the n non-zero rows (A -> B -> A); a row lives in one wave: wave-level fence only
        if (row_act) {
            load8<8>(bufA + r_row * LD + j_row, nv_row, v);
            dft_fwd<8>(v);
            store8_all<1>(bufB + r_row * LD + j_row * 9, v);      // butterfly j at [9 j, 9 j + 8): both sides conflict free
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (row_act) {
            load8_all<9>(bufB + r_row * LD + j_row, v);
            twiddle8(v, twr);
            dft_fwd<8>(v);
            store8_all<8>(bufA + r_row * LD + j_row, v);
        }
        __syncthreads();
        EFGP_STAMP(1);
        // P3: forward FFT along dim 0, stage 1 (A -> B), rows >= n are zero
        load8<8 * LD>(bufA + j_col * LD + c_col, nv_col, v);
        dft_fwd<8>(v);
        store8_all<LD>(bufB + j_col * 8 * LD + c_col, v);
        __syncthreads();
        // P4: stage 2 of the forward column FFT, spectral multiply, stage 1 of the inverse column FFT (B -> A)
        load8_all<8 * LD>(bufB + j_col * LD + c_col, v);
        twiddle8(v, twc);
        dft_fwd<8>(v);
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = conjd(cmulp(v[t], spec[t]));
        dft_fwd<8>(v);
        conj8(v);
        store8_all<LD>(bufA + j_col * 8 * LD + c_col, v);
        __syncthreads();
        EFGP_STAMP(2);
        // P5: inverse column FFT stage 2 (A -> B), only rows of the crop window are stored
        load8_all<8 * LD>(bufA + j_col * LD + c_col, v);
        conj8(v);
        twiddle8(v, twc);
        dft_fwd<8>(v);
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (keep_col & (1u << t)) bufB[(j_col + 8 * t) * LD + c_col] = conjd(v[t]);
        __syncthreads();
        EFGP_STAMP(4);
        // P6/P7: inverse FFT along dim 1 of the n window rows (B -> A -> B), cropped columns at the end
        const int wrow = n - 1 + r_row;
        if (row_act) {
            load8_all<8>(bufB + wrow * LD + j_row, v);
            conj8(v);
            dft_fwd<8>(v);
            conj8(v);
            store8_all<1>(bufA + wrow * LD + j_row * 9, v);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (row_act) {
            load8_all<9>(bufA + wrow * LD + j_row, v);
            conj8(v);
            twiddle8(v, twr);
            dft_fwd<8>(v);
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (keep_row & (1u << t)) bufB[wrow * LD + j_row + 8 * t] = conjd(v[t]);
        }
        __syncthreads();
        EFGP_STAMP(5);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (tid + s * kThreads < M) {
                const double2 gg = cmulp(wsv[s], bufB[off_out[s]]);
                if (a.variant == 0) Au[s] = make_double2(gg.x + a.sigmasq * u[s].x, gg.y + a.sigmasq * u[s].y);
                else Au[s] = make_double2(gg.x / a.sigmasq + u[s].x, gg.y / a.sigmasq + u[s].y);
            } else {
                Au[s] = make_double2(0.0, 0.0);
            }
        }
        // no barrier here: the next LDS writes are reduction scratch (disjoint) and, behind that reduction's
        // barrier, bufA -- whose last readers (P7) are already behind the barrier above
        EFGP_STAMP(8);
    };

    EFGP_LANCZOS_BRANCH(KS, tid)

    double2 Ap[KS];
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < (int)(sizeof(Ap) / sizeof(Ap[0])); ++s) Ap[s] = make_double2(0.0, 0.0);
    } else {
        apply_A(xv, Ap);
    }
    double rz = 0.0, bb = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (tid + s * kThreads < M) {
            double2 bv = a.b[base + tid + s * kThreads];
            if (a.b_times_ws) bv = cmulp(wsv[s], bv);
            rv[s] = csub(bv, Ap[s]);
            pv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            rz += rv[s].x * pv[s].x + rv[s].y * pv[s].y;
            bb += bv.x * bv.x + bv.y * bv.y;
        }
    }
    block_sum_pair(rz, bb, red);
    const double bn = sqrt(bb);
    const double den = bn > 0.0 ? bn : 1.0;
    int it = 0;
    for (; it < a.max_iter;) {
        apply_A(pv, Ap);
        double pAp = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) pAp += pv[s].x * Ap[s].x + pv[s].y * Ap[s].y;
        pAp = block_sum2(pAp, red) + 1e-16;
        const double alpha = rz / pAp;
        double rr = 0.0, rzn = 0.0;
        double2 zv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xv[s].x += alpha * pv[s].x;
            xv[s].y += alpha * pv[s].y;
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            rr += rv[s].x * rv[s].x + rv[s].y * rv[s].y;
            rzn += rv[s].x * zv[s].x + rv[s].y * zv[s].y;
        }
        block_sum_pair(rr, rzn, red);
        ++it;
        const double rnorm = sqrt(rr);
        if (a.hist && row == 0 && threadIdx.x == 0 && it <= a.hist_cap) a.hist[it - 1] = rnorm / (den + 1e-16);
        const bool conv = a.early_stop && ((rnorm / (den + 1e-16) < a.tol) || (a.batched && rnorm < 1e-12));
        if (!a.batched && conv) break;
        const double beta = rzn / (rz + 1e-16);
#pragma unroll
        for (int s = 0; s < KS; ++s) pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
        rz = rzn;
        if (conv) break;
    }
#pragma unroll
    for (int s = 0; s < KS; ++s)
        if (tid + s * kThreads < M) a.x[base + tid + s * kThreads] = xv[s];
    if (tid == 0) a.iters[row] = it;
}

// The Hermitian specialisations (cg_herm64_kernel, cg_herm48_kernel, cg_herm48_pairs_kernel): cg_herm.hip

// ------------------------------------------------------------------------------------------------
// 1-D systems (round 3): the whole solve in ONE WAVE per system.  cg_persistent_kernel above spends ~8 us per iteration on a
// 1-D block of 63 unknowns (BASELINE configs[0] is such a model: mtot 35, F = 128): its passes are built for grids -- 1024
// threads, a workgroup barrier per radix stage, two-level block reductions -- and a single 128-point line leaves all but a few
// lanes idle at every barrier.  Here a system is one wave: the vectors in registers (<= 4 entries per lane: n <= 255, F <= 512),
// the line transform a radix-4 / radix-2 Stockham ping-pong in LDS with wave-level synchronisation only, the spectrum and the
// twiddles resident in LDS, dot products by wave reductions.  Same operator (zero-padded input at [0, n), product read at
// [n - 1, 2 n - 1)), recurrences and stopping rules as cg_persistent_kernel (cg.py:86-244).
// ------------------------------------------------------------------------------------------------
namespace l1d {
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// forward transform of the F-point line in `x` (F = 2^lg), scratch `y`; twiddles tw[q] = exp(-2 pi i q / F); returns the buffer
// that holds the result (natural order).  All 64 lanes of the wave take part.
__device__ __forceinline__ double2* wave_fft(double2* x, double2* y, int F, int lg, const double2* __restrict__ tw) {
    const int lane = threadIdx.x;
    int Ns = 1, rem = lg;
    while (rem >= 2) {
        const int nb = F >> 2, tstep = F / (Ns * 4);
        for (int j = lane; j < nb; j += 64) {
            const int k = j & (Ns - 1), j0 = ((j - k) << 2) + k;
            double2 v0 = x[j], v1 = x[j + nb], v2 = x[j + 2 * nb], v3 = x[j + 3 * nb];
            if (k != 0) {
                v1 = cmulp(v1, tw[k * tstep]);
                v2 = cmulp(v2, tw[2 * k * tstep]);
                v3 = cmulp(v3, tw[3 * k * tstep]);
            }
            const double2 t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3), d13 = csub(v1, v3);
            const double2 t3 = make_double2(d13.y, -d13.x);              // (v1 - v3) * (-i)
            y[j0] = cadd(t0, t2);
            y[j0 + Ns] = cadd(t1, t3);
            y[j0 + 2 * Ns] = csub(t0, t2);
            y[j0 + 3 * Ns] = csub(t1, t3);
        }
        wave_sync();
        double2* t = x;
        x = y;
        y = t;
        Ns <<= 2;
        rem -= 2;
    }
    if (rem == 1) {
        const int nb = F >> 1;                                           // Ns = F / 2: tstep = 1
        for (int j = lane; j < nb; j += 64) {
            const int k = j & (Ns - 1), j0 = ((j - k) << 1) + k;
            const double2 v0 = x[j];
            double2 v1 = x[j + nb];
            if (k != 0) v1 = cmulp(v1, tw[k]);
            y[j0] = cadd(v0, v1);
            y[j0 + Ns] = csub(v0, v1);
        }
        wave_sync();
        double2* t = x;
        x = y;
        y = t;
    }
    return x;
}
}  // namespace l1d

__global__ __launch_bounds__(64) void cg_line1d_kernel(Args a) {
    using namespace l1d;
    extern __shared__ double2 lds2[];
    const int F = a.g.F[0], n = a.g.n[0], M = a.g.M;
    const int lg = 31 - __clz(F);
    double2* const X = lds2;
    double2* const Y = lds2 + F;
    double2* const TW = Y + F;
    double2* const VH = TW + F;
    const int lane = threadIdx.x, row = blockIdx.x;
    const int64_t base = (int64_t)row * M;
    for (int q = lane; q < F; q += 64) {
        TW[q] = a.g.tw[0][q];
        VH[q] = a.vhat[q];
    }
    double2 xv[KS], rv[KS], pv[KS], wsv[KS];
    double dg[KS];
    const bool precond = a.diag != nullptr || a.diag_scale != nullptr;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = lane + 64 * s;
        if (t < M) {
            xv[s] = a.zero_x0 ? make_double2(0.0, 0.0) : a.x0[base + t];
            wsv[s] = a.ws[t];
            dg[s] = jacobi_entry(a, wsv[s], t);
        } else {
            xv[s] = wsv[s] = make_double2(0.0, 0.0);
            dg[s] = 1.0;
        }
        rv[s] = pv[s] = make_double2(0.0, 0.0);
    }
    wave_sync();
    auto apply_A = [&](const double2 (&u)[KS], double2 (&Au)[KS]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int t = lane + 64 * s;
            if (t < M) X[t] = cmulp(wsv[s], u[s]);
        }
        for (int q = n + lane; q < F; q += 64) X[q] = make_double2(0.0, 0.0);
        wave_sync();
        double2* R = wave_fft(X, Y, F, lg, TW);
        double2* O = R == X ? Y : X;
        for (int q = lane; q < F; q += 64) {
            const double2 m = cmulp(R[q], VH[q]);
            R[q] = make_double2(m.x, -m.y);                               // conjugate: the inverse transform by a forward one
        }
        wave_sync();
        const double2* Z = wave_fft(R, O, F, lg, TW);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int t = lane + 64 * s;
            if (t < M) {
                const double2 z = Z[n - 1 + t];
                const double2 gg = cmulp(wsv[s], make_double2(z.x, -z.y));
                if (a.variant == 0) Au[s] = make_double2(gg.x + a.sigmasq * u[s].x, gg.y + a.sigmasq * u[s].y);
                else Au[s] = make_double2(gg.x / a.sigmasq + u[s].x, gg.y / a.sigmasq + u[s].y);
            } else {
                Au[s] = make_double2(0.0, 0.0);
            }
        }
        wave_sync();                                                      // the buffers are rewritten by the next application
    };
    double2 Ap[KS];
    if (a.zero_x0) {
#pragma unroll
        for (int s = 0; s < KS; ++s) Ap[s] = make_double2(0.0, 0.0);
    } else {
        apply_A(xv, Ap);
    }
    double rz = 0.0, bb = 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = lane + 64 * s;
        if (t < M) {
            double2 bv = a.b[base + t];
            if (a.b_times_ws) bv = cmulp(wsv[s], bv);
            rv[s] = csub(bv, Ap[s]);
            pv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            rz += rv[s].x * pv[s].x + rv[s].y * pv[s].y;
            bb += bv.x * bv.x + bv.y * bv.y;
        }
    }
    rz = wave_sum(rz);
    bb = wave_sum(bb);
    const double bn = sqrt(bb);
    const double den = bn > 0.0 ? bn : 1.0;
    int it = 0;
    for (; it < a.max_iter;) {
        apply_A(pv, Ap);
        double pAp = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) pAp += pv[s].x * Ap[s].x + pv[s].y * Ap[s].y;
        pAp = wave_sum(pAp) + 1e-16;
        const double alpha = rz / pAp;
        double rr = 0.0, rzn = 0.0;
        double2 zv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            xv[s].x += alpha * pv[s].x;
            xv[s].y += alpha * pv[s].y;
            rv[s].x -= alpha * Ap[s].x;
            rv[s].y -= alpha * Ap[s].y;
            zv[s] = precond ? make_double2(rv[s].x / dg[s], rv[s].y / dg[s]) : rv[s];
            rr += rv[s].x * rv[s].x + rv[s].y * rv[s].y;
            rzn += rv[s].x * zv[s].x + rv[s].y * zv[s].y;
        }
        rr = wave_sum(rr);
        rzn = wave_sum(rzn);
        ++it;
        const double rnorm = sqrt(rr);
        if (a.hist && row == 0 && lane == 0 && it <= a.hist_cap) a.hist[it - 1] = rnorm / (den + 1e-16);
        const bool conv = a.early_stop && ((rnorm / (den + 1e-16) < a.tol) || (a.batched && rnorm < 1e-12));
        if (!a.batched && conv) break;                  // cg.py:132 (before the preconditioner / p update)
        const double beta = rzn / (rz + 1e-16);
#pragma unroll
        for (int s = 0; s < KS; ++s) pv[s] = make_double2(zv[s].x + beta * pv[s].x, zv[s].y + beta * pv[s].y);
        rz = rzn;
        if (conv) break;                                // cg.py:229-241 (after the p update)
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = lane + 64 * s;
        if (t < M) a.x[base + t] = xv[s];
    }
    if (lane == 0) a.iters[row] = it;
}

// Spectrum of the Toeplitz vector for the 64 x 64 circulant grid in ONE launch (efgpnd.py:1283-1290: pad to the FFT
// box, forward fftn): `factor * v` zero-padded into LDS, four radix-8 Stockham stages as in the solver above, result
// in natural order.  Replaces pad_scale_kernel + two rocFFT launches (~14 us of dependent 4-5 us launches per fit).
__device__ __forceinline__ void toeplitz_vhat_2d64_body(const double2* __restrict__ v, int L0, int L1, double factor,
                                                        double2* __restrict__ vhat, double2* lds2) {
    using namespace s64;
    double2* const bufA = lds2;
    double2* const bufB = lds2 + BUF;
    const int tid = threadIdx.x;
    for (int t = tid; t < F * F; t += kThreads) {
        const int i0 = t >> 6, i1 = t & 63;
        double2 x = make_double2(0.0, 0.0);
        if (i0 < L0 && i1 < L1) {
            x = v[i0 * L1 + i1];
            x.x *= factor;
            x.y *= factor;
        }
        bufA[i0 * LD + i1] = x;
    }
    const int c = tid & 63, j = tid >> 6;      // line (row, then column) and butterfly within the line
    double2 tw[7];
#pragma unroll
    for (int t = 1; t < 8; ++t) {
        double sn, cs;
        sincospi(-(double)(j * t) / 32.0, &sn, &cs);      // exp(-2 pi i j t / 64)
        tw[t - 1] = make_double2(cs, sn);
    }
    __syncthreads();
    double2 x[8];
    // dimension 1 (contiguous), all 64 rows: lane = row
    load8_all<8>(bufA + c * LD + j, x);
    dft_fwd<8>(x);
    store8_all<1>(bufB + c * LD + j * 8, x);
    __syncthreads();
    load8_all<8>(bufB + c * LD + j, x);
    twiddle8(x, tw);
    dft_fwd<8>(x);
    store8_all<8>(bufA + c * LD + j, x);
    __syncthreads();
    // dimension 0: lane = column
    load8_all<8 * LD>(bufA + j * LD + c, x);
    dft_fwd<8>(x);
    store8_all<LD>(bufB + j * 8 * LD + c, x);
    __syncthreads();
    load8_all<8 * LD>(bufB + j * LD + c, x);
    twiddle8(x, tw);
    dft_fwd<8>(x);
#pragma unroll
    for (int t = 0; t < 8; ++t) vhat[(j + 8 * t) * F + c] = x[t];
}
__global__ __launch_bounds__(kThreads) void toeplitz_vhat_2d64_kernel(const double2* __restrict__ v, int L0, int L1,
                                                                      double factor, double2* __restrict__ vhat) {
    extern __shared__ double2 lds2[];
    toeplitz_vhat_2d64_body(v, L0, L1, factor, vhat, lds2);
}

// The same for the 48 x 48 circulant grid of cg_herm48_kernel (round 4): vhat48_lines above on 512 threads (64 line slots, one pass).
__device__ __forceinline__ void toeplitz_vhat_2d48_body(const double2* __restrict__ v, int L0, int L1, double factor,
                                                        double2* __restrict__ vhat, double2* lds2) {
    h48::vhat48_lines<kThreads, false>(v, L0, L1, factor, vhat, lds2);
}
// both spectra of an operator in ONE launch (two workgroups on two CUs): a dependent launch costs more than either transform
__global__ __launch_bounds__(kThreads) void toeplitz_vhat_pair_kernel(const double2* __restrict__ v, int L0, int L1, double factor64,
                                                                      double2* __restrict__ vhat64, double factor48,
                                                                      double2* __restrict__ vhat48) {
    extern __shared__ double2 lds2[];
    if (vhat64 != nullptr && blockIdx.x == 0) toeplitz_vhat_2d64_body(v, L0, L1, factor64, vhat64, lds2);
    else toeplitz_vhat_2d48_body(v, L0, L1, factor48, vhat48, lds2);
}

// Batched variant for the lag-sum correlation of the stochastic variance (variance_ops.hip): transform b reads the
// L0 x L1 array src + b * src_stride (complex, or real doubles when REAL), zero-pads it to 64 x 64 and writes the forward
// transform in natural order to dst + b * dst_stride.  One workgroup per transform, no rocFFT (no run-time compilation).
template <bool REAL>
__global__ __launch_bounds__(kThreads) void fft2d64_batch_kernel(const void* __restrict__ src, int64_t src_stride, int L0, int L1,
                                                                 double2* __restrict__ dst, int64_t dst_stride) {
    using namespace s64;
    extern __shared__ double2 lds2[];
    double2* const bufA = lds2;
    double2* const bufB = lds2 + BUF;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int t = tid; t < F * F; t += kThreads) {
        const int i0 = t >> 6, i1 = t & 63;
        double2 x = make_double2(0.0, 0.0);
        if (i0 < L0 && i1 < L1) {
            if (REAL) x.x = ((const double*)src)[b * src_stride + i0 * L1 + i1];
            else x = ((const double2*)src)[b * src_stride + i0 * L1 + i1];
        }
        bufA[i0 * LD + i1] = x;
    }
    const int c = tid & 63, j = tid >> 6;
    double2 tw[7];
#pragma unroll
    for (int t = 1; t < 8; ++t) {
        double sn, cs;
        sincospi(-(double)(j * t) / 32.0, &sn, &cs);
        tw[t - 1] = make_double2(cs, sn);
    }
    __syncthreads();
    double2 x[8];
    load8_all<8>(bufA + c * LD + j, x);
    dft_fwd<8>(x);
    store8_all<1>(bufB + c * LD + j * 8, x);
    __syncthreads();
    load8_all<8>(bufB + c * LD + j, x);
    twiddle8(x, tw);
    dft_fwd<8>(x);
    store8_all<8>(bufA + c * LD + j, x);
    __syncthreads();
    load8_all<8 * LD>(bufA + j * LD + c, x);
    dft_fwd<8>(x);
    store8_all<LD>(bufB + j * 8 * LD + c, x);
    __syncthreads();
    load8_all<8 * LD>(bufB + j * LD + c, x);
    twiddle8(x, tw);
    dft_fwd<8>(x);
    double2* out = dst + b * dst_stride;
#pragma unroll
    for (int t = 0; t < 8; ++t) out[(j + 8 * t) * F + c] = x[t];
}

}  // namespace pcg

int fft2d64_batch_launch(const void* src, int src_is_real, int64_t src_stride, int L0, int L1, double2* dst, int64_t dst_stride,
                         int nbatch, hipStream_t stream) {
    using namespace pcg;
    const size_t lds = (size_t)2 * s64::BUF * sizeof(double2);
    const void* kernel = src_is_real ? (const void*)fft2d64_batch_kernel<true> : (const void*)fft2d64_batch_kernel<false>;
    if (const int rc = raise_dynamic_lds(kernel, lds, "64 x 64 batched transform")) return rc;
    if (src_is_real) hipLaunchKernelGGL(fft2d64_batch_kernel<true>, dim3(nbatch), dim3(kThreads), lds, stream, src, src_stride, L0, L1, dst, dst_stride);
    else hipLaunchKernelGGL(fft2d64_batch_kernel<false>, dim3(nbatch), dim3(kThreads), lds, stream, src, src_stride, L0, L1, dst, dst_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("64 x 64 batched transform launch failed: %s", hipGetErrorString(e));
        return EFGP_EHIP;
    }
    return EFGP_OK;
}

int toeplitz_vhat_fused_launch(const double2* v, int L0, int L1, double factor, double2* vhat, hipStream_t stream) {
    using namespace pcg;
    const size_t lds = (size_t)2 * s64::BUF * sizeof(double2);
    if (const int rc = raise_dynamic_lds((const void*)toeplitz_vhat_2d64_kernel, lds, "Toeplitz spectrum (64x64)")) return rc;
    hipLaunchKernelGGL(toeplitz_vhat_2d64_kernel, dim3(1), dim3(kThreads), lds, stream, v, L0, L1, factor, vhat);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("Toeplitz spectrum (64x64) launch failed: %s", hipGetErrorString(e));
        return EFGP_EHIP;
    }
    return EFGP_OK;
}

// vhat64 (may be null) and vhat48 in one launch; both are FFT(zero-padded v) / (their grid size), natural order
int toeplitz_vhat_pair_launch(const double2* v, int L0, int L1, double2* vhat64, double2* vhat48, hipStream_t stream) {
    using namespace pcg;
    const size_t lds = vhat64 ? (size_t)2 * s64::BUF * sizeof(double2) : (size_t)(48 * 49 + 64 * 72) * sizeof(double2);
    if (const int rc = raise_dynamic_lds((const void*)toeplitz_vhat_pair_kernel, lds, "Toeplitz spectra (64x64 + 48x48)")) return rc;
    hipLaunchKernelGGL(toeplitz_vhat_pair_kernel, dim3(vhat64 ? 2 : 1), dim3(kThreads), lds, stream, v, L0, L1, 1.0 / 4096.0, vhat64,
                       1.0 / 2304.0, vhat48);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("Toeplitz spectra (64x64 + 48x48) launch failed: %s", hipGetErrorString(e));
        return EFGP_EHIP;
    }
    return EFGP_OK;
}

namespace pcg {

// y[row] = post .* T(pre .* x[row]) on the 64 x 64 circulant grid in ONE launch, one workgroup per row: the operator part of
// cg_persistent_2d64_kernel's iteration (same lane maps, same pruned passes, same arithmetic) without the recurrences.
// The hyper-gradient applies T three times per step outside a solve (T g, T D'F*Z, T D V: efgpnd.py:150-153, :186-189, :203);
// through pad / two rocFFT plans / multiply / two rocFFT plans / crop that is 7 dependent launches each.
// pre / post: M-length complex diagonals or null; x may be real (x_is_real: M doubles per row).
struct ApplyArgs {
    int n, M;
    const double2* tw;       // exp(-2 pi i q / 64)
    const double2* vhat;     // [64][64], already divided by 4096
    const double2* pre;
    int pre_stride;          // entries between consecutive elements of pre (a column of an (M, H) array: H)
    const double2* post;
    const void* x;
    int x_is_real;
    double2* y;
};

__global__ __launch_bounds__(kThreads) void toeplitz_apply_2d64_kernel(ApplyArgs a) {
    using namespace s64;
    constexpr int LD = 72, BUF = F * LD;    // row pitch as in cg_persistent_2d64_kernel (8 mod 16)
    constexpr int KS = 2;
    extern __shared__ double2 lds2[];
    double2* const bufA = lds2;
    double2* const bufB = lds2 + BUF;
    const int n = a.n, M = a.M;
    const int64_t base = (int64_t)blockIdx.x * M;
    const int tid = threadIdx.x;
    const int j_row = tid & 7, r_row = tid >> 3;
    const bool row_act = r_row < n;
    const int c_col = tid & 63, j_col = tid >> 6;
    const int nv_row = j_row < n ? (n - 1 - j_row) / 8 + 1 : 0;
    const int nv_col = j_col < n ? (n - 1 - j_col) / 8 + 1 : 0;
    unsigned keep_col = 0, keep_row = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int pc = j_col + 8 * t, pr = j_row + 8 * t;
        if (pc >= n - 1 && pc < 2 * n - 1) keep_col |= 1u << t;
        if (pr >= n - 1 && pr < 2 * n - 1) keep_row |= 1u << t;
    }
    double2 twr[7], twc[7];
#pragma unroll
    for (int t = 1; t < 8; ++t) {
        twr[t - 1] = a.tw[j_row * t];
        twc[t - 1] = a.tw[j_col * t];
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = tid + s * kThreads;
        if (t < M) {
            double2 u = a.x_is_real ? make_double2(((const double*)a.x)[base + t], 0.0) : ((const double2*)a.x)[base + t];
            if (a.pre) u = cmulp(a.pre[(int64_t)t * a.pre_stride], u);
            const int i0 = t / n, i1 = t - i0 * n;
            bufA[i0 * LD + i1] = u;
        }
    }
    __syncthreads();
    double2 v[8];
    // forward along dim 1 of the n non-zero rows (A -> B -> A), a row lives in one wave
    if (row_act) {
        load8<8>(bufA + r_row * LD + j_row, nv_row, v);
        dft_fwd<8>(v);
        store8_all<1>(bufB + r_row * LD + j_row * 9, v);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (row_act) {
        load8_all<9>(bufB + r_row * LD + j_row, v);
        twiddle8(v, twr);
        dft_fwd<8>(v);
        store8_all<8>(bufA + r_row * LD + j_row, v);
    }
    __syncthreads();
    // forward along dim 0 (rows >= n are zero), spectrum, inverse along dim 0 keeping the crop window's rows
    load8<8 * LD>(bufA + j_col * LD + c_col, nv_col, v);
    dft_fwd<8>(v);
    store8_all<LD>(bufB + j_col * 8 * LD + c_col, v);
    __syncthreads();
    load8_all<8 * LD>(bufB + j_col * LD + c_col, v);
    twiddle8(v, twc);
    dft_fwd<8>(v);
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = conjd(cmulp(v[t], a.vhat[(j_col + 8 * t) * F + c_col]));
    dft_fwd<8>(v);
    conj8(v);
    store8_all<LD>(bufA + j_col * 8 * LD + c_col, v);
    __syncthreads();
    load8_all<8 * LD>(bufA + j_col * LD + c_col, v);
    conj8(v);
    twiddle8(v, twc);
    dft_fwd<8>(v);
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (keep_col & (1u << t)) bufB[(j_col + 8 * t) * LD + c_col] = conjd(v[t]);
    __syncthreads();
    // inverse along dim 1 of the n window rows (B -> A -> B), cropped columns
    const int wrow = n - 1 + r_row;
    if (row_act) {
        load8_all<8>(bufB + wrow * LD + j_row, v);
        conj8(v);
        dft_fwd<8>(v);
        conj8(v);
        store8_all<1>(bufA + wrow * LD + j_row * 9, v);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (row_act) {
        load8_all<9>(bufA + wrow * LD + j_row, v);
        conj8(v);
        twiddle8(v, twr);
        dft_fwd<8>(v);
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (keep_row & (1u << t)) bufB[wrow * LD + j_row + 8 * t] = conjd(v[t]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int t = tid + s * kThreads;
        if (t < M) {
            const int i0 = t / n, i1 = t - i0 * n;
            double2 g = bufB[(i0 + n - 1) * LD + (i1 + n - 1)];
            if (a.post) g = cmulp(a.post[t], g);
            a.y[base + t] = g;
        }
    }
}

}  // namespace pcg

int toeplitz_apply_fused_launch(const ToepGeom& g, const double2* tw64, const double2* vhat, const double2* pre, const double2* post,
                                const void* x, int x_is_real, double2* y, int rows, hipStream_t stream, int pre_stride) {
    using namespace pcg;
    const size_t lds = (size_t)2 * 64 * 72 * sizeof(double2);
    if (const int rc = raise_dynamic_lds((const void*)toeplitz_apply_2d64_kernel, lds, "Toeplitz apply (64x64)")) return rc;
    ApplyArgs a;
    a.n = (int)g.n[0];
    a.M = (int)g.M;
    a.tw = tw64;
    a.vhat = vhat;
    a.pre = pre;
    a.pre_stride = pre_stride;
    a.post = post;
    a.x = x;
    a.x_is_real = x_is_real;
    a.y = y;
    hipLaunchKernelGGL(toeplitz_apply_2d64_kernel, dim3(rows), dim3(kThreads), lds, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("Toeplitz apply (64x64) launch failed: %s", hipGetErrorString(e));
        return EFGP_EHIP;
    }
    return EFGP_OK;
}

namespace pcg {

#ifdef EFGP_CG_STAMPS
static long long* g_last_stamps = nullptr;
#endif
static const char* g_last_launch = "";       // label of the last single-launch solve that was enqueued (efgp_cg_last_launch)

static void radices_for(int n, Pass* p) {
    int k = 0;
    while ((1 << k) < n) ++k;
    p->nstages = 0;
    while (k >= 3 && (k != 4)) {
        p->radix[p->nstages++] = 8;
        k -= 3;
    }
    if (k == 4) {
        p->radix[p->nstages++] = 4;
        p->radix[p->nstages++] = 4;
        k = 0;
    }
    if (k == 2) p->radix[p->nstages++] = 4;
    if (k == 1) p->radix[p->nstages++] = 2;
}

}  // namespace pcg

extern "C" const char* efgp_cg_last_launch(void) { return pcg::g_last_launch; }

#ifdef EFGP_CG_STAMPS
extern "C" int efgp_debug_cg_stamps(long long* out16) {
    (void)hipDeviceSynchronize();
    if (!pcg::g_last_stamps) return -1;
    return hipMemcpy(out16, pcg::g_last_stamps, 16 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif

namespace pcg {

// An axis with a single mode has F = 1: no stage to run (radices_for gives nstages = 0).  As axis 0 it would own the fused
// middle stage -- the spectral multiply would be skipped and the spectrum registers loaded through radix[-1].  Such an axis has
// one lag and one cell: block, padded grid and spectrum keep their row-major order without it, so the kernels get the geometry
// of the remaining axes (exact).  Returns how many axes are left: a grid of one cell in all never comes here
// (efgp_toeplitz_create_ex).
static int squeeze_unit_axes(const ToepGeom& full, const double2* const* tw_full, ToepGeom* tg, const double2** twiddles) {
    *tg = full;
    tg->d = 0;
    for (int i = 0; i < full.d; ++i) {
        if (full.F[i] == 1) continue;
        tg->n[tg->d] = full.n[i];
        tg->F[tg->d] = full.F[i];
        twiddles[tg->d] = tw_full[i];
        ++tg->d;
    }
    for (int i = tg->d; i < 3; ++i) tg->n[i] = tg->F[i] = 1;
    return tg->d;
}

// Pass `p` over dimension `dim`, with the line ranges of the two other dimensions.  Forward (the last dimension goes first): lines
// restricted to the leading n-box of the dims not transformed yet.  Inverse (the first dimension goes first): outputs cropped to
// [n-1, 2n-1), later passes only visit cropped lines.
static void set_pass(const Geom& g, int dim, bool inverse, Pass& p) {
    p.dim = dim;
    p.n = g.F[dim];
    radices_for(p.n, &p);
    int oi = 0;
    for (int o = 0; o < 3; ++o) {
        if (o == dim) continue;
        p.other[oi] = o;
        p.lo[oi] = 0;
        if (o >= g.d) {
            p.hi[oi] = 1;
        } else if (o > dim) {           // forward: already transformed; inverse: still to come -- full range
            p.hi[oi] = g.F[o];
        } else if (!inverse) {          // not transformed yet: only the n-box is non-zero
            p.hi[oi] = g.n[o];
        } else {                        // already inverse-transformed and cropped
            p.lo[oi] = g.n[o] - 1;
            p.hi[oi] = 2 * g.n[o] - 1;
        }
        ++oi;
    }
    p.in_limit = inverse ? p.n : g.n[dim];
    p.out_lo = inverse ? g.n[dim] - 1 : 0;
    p.out_hi = inverse ? 2 * g.n[dim] - 1 : p.n;
}

// how the lanes walk the lines of each pass
static void order_lines(Geom& g) {
    auto ilog2 = [](int v) {
        int l = 0;
        while ((1 << l) < v) ++l;
        return l;
    };
    for (int q = 0; q < g.d; ++q) {
        for (Pass* p : {&g.fwd[q], &g.inv[q]}) {
            // `other[1]` must be the faster-varying (smaller stride) of the two so that lanes walk it first
            const int s0 = p->other[0] < g.d ? g.ld[p->other[0]] : 0;
            const int s1 = p->other[1] < g.d ? g.ld[p->other[1]] : 0;
            const bool swap = (p->other[1] >= g.d) ? (p->other[0] < g.d) : (p->other[0] < g.d && s0 < s1 && s0 > 0);
            if (swap) {
                std::swap(p->other[0], p->other[1]);
                std::swap(p->lo[0], p->lo[1]);
                std::swap(p->hi[0], p->hi[1]);
            }
            p->w1_log2 = ilog2(p->hi[1] - p->lo[1]);
            p->lines_log2 = p->w1_log2 + ilog2(p->hi[0] - p->lo[0]);
        }
    }
}

// LDS twiddle copies behind the two ping-pong buffers while they fit in the 160 KB budget, and every pass's strides in the padded
// grid and in the unpadded spectrum
static void place_twiddles_and_strides(Geom& g) {
    g.tw_lds_total = 0;
    const int lds_budget = 160 * 1024 - 256;
    for (int i = 0; i < 3; ++i) g.tw_lds_off[i] = -1;
    for (int i = 0; i < g.d; ++i) {
        int shared = -1;
        for (int b_ = 0; b_ < i; ++b_)
            if (g.F[b_] == g.F[i] && g.tw_lds_off[b_] >= 0) shared = g.tw_lds_off[b_];
        if (shared >= 0) {
            g.tw_lds_off[i] = shared;
            continue;
        }
        const size_t need = ((size_t)2 * g.padded + g.tw_lds_total + g.F[i]) * sizeof(double2);
        if (need <= (size_t)lds_budget) {
            g.tw_lds_off[i] = g.tw_lds_total;
            g.tw_lds_total += g.F[i];
        }
    }
    int vstride[3] = {0, 0, 0};
    int acc = 1;
    for (int i = g.d - 1; i >= 0; --i) {
        vstride[i] = acc;
        acc *= g.F[i];
    }
    for (int q = 0; q < g.d; ++q) {
        for (Pass* p : {&g.fwd[q], &g.inv[q]}) {
            p->vs_pos = vstride[p->dim];
            p->vs_c0 = p->other[0] < g.d ? vstride[p->other[0]] : 0;
            p->vs_c1 = p->other[1] < g.d ? vstride[p->other[1]] : 0;
            p->pstride = g.ld[p->dim];
            p->s0 = p->other[0] < g.d ? g.ld[p->other[0]] : 0;
            p->s1 = p->other[1] < g.d ? g.ld[p->other[1]] : 0;
            p->tw_lds = g.tw_lds_off[p->dim];
            p->tw_glob = g.tw[p->dim];
        }
    }
}

// The pass geometry of the generic kernel for a block without unit axes: dims sit in slots 0..d-1 and missing trailing F are 1, so
// the spectrum's flat index (i0*F1 + i1)*F2 + i2 holds
static void pass_geometry(const ToepGeom& tg, const double2* const* twiddles, Geom& g) {
    g.d = tg.d;
    for (int i = 0; i < 3; ++i) {
        g.n[i] = i < tg.d ? (int)tg.n[i] : 1;
        g.F[i] = i < tg.d ? (int)tg.F[i] : 1;
        g.tw[i] = i < tg.d ? twiddles[i] : nullptr;
    }
    // strides of the padded grid
    int stride = 1;
    for (int i = 2; i >= 0; --i) {
        if (i >= tg.d) {
            g.ld[i] = 0;
            continue;
        }
        g.ld[i] = stride;
        stride *= (i == tg.d - 1 && tg.d > 1) ? g.F[i] + 1 : g.F[i];
    }
    g.padded = stride;
    g.M = (int)tg.M;
    g.npass = tg.d;
    for (int q = 0; q < tg.d; ++q) {
        set_pass(g, tg.d - 1 - q, false, g.fwd[q]);
        Pass& p = g.inv[q];
        set_pass(g, q, true, p);
        // inverse passes use the forward radices in reverse order (so that the fused middle stage lines up)
        for (int i = 0; i < p.nstages / 2; ++i) std::swap(p.radix[i], p.radix[p.nstages - 1 - i]);
    }
    order_lines(g);
    // fused middle stage: forward last pass (dim 0) and inverse first pass (dim 0) share dimension and the
    // last forward radix equals the first inverse radix by construction; both visit the same lines (all of
    // the other dimensions' FFT range), so the fusion is always structurally valid when d >= 1
    g.fuse_mid = 1;
    place_twiddles_and_strides(g);
}

// the solve as the kernels take it (the geometry apart)
static void solve_args(const CgSolve& s, const double2* vhat, int* d_iters, const LanczosOut* lz, Args& a) {
    a.ws_out = nullptr;
    a.vsrc = nullptr;
    a.vhat_out = nullptr;
    a.ws = s.ws;
    a.diag = s.diag;
    a.diag_scale = s.diag_scale;
    a.b_times_ws = s.b_times_ws;
    a.zero_x0 = s.zero_x0;
    a.x0 = s.x0 ? s.x0 : s.x;
    a.vhat = vhat;
    a.sigmasq = s.sigmasq;
    a.variant = s.variant;
    a.tol = s.tol;
    a.early_stop = s.early_stop;
    a.batched = s.batched;
    a.max_iter = s.max_iter;
    a.b = s.b;
    a.x = s.x;
    a.iters = d_iters;
    a.hist = cg_history().buf;
    a.hist_cap = cg_history().capacity;
    a.lz_steps = lz ? lz->steps : 0;
    a.lz_alpha = lz ? lz->alpha : nullptr;
    a.lz_beta = lz ? lz->beta : nullptr;
    a.lz_norm2 = lz ? lz->norm2 : nullptr;
}

// kernel, workgroup size and dynamic LDS of a pick (one workgroup per system); the Hermitian picks: herm_launch (cg_herm.hip)
static PickLaunch launch_of(const PersistentChoice& c, const Geom& g) {
    switch (c.pick) {
        case PersistentPick::line1d:          // 1-D: one wave per system
            return {cg_line1d_kernel, 64, (size_t)4 * g.F[0] * sizeof(double2), "persistent CG (1-D)"};
        case PersistentPick::fast64:
            return {cg_persistent_2d64_kernel, kThreads, (size_t)2 * 64 * 72 * sizeof(double2), "persistent CG (64x64)"};
        default:
            break;
    }
    return {cg_persistent_kernel, kThreads, ((size_t)2 * g.padded + g.tw_lds_total) * sizeof(double2), "persistent CG"};
}

}  // namespace pcg

int persistent_cg_launch(const ToepGeom& full, const double2* const* tw_full, const double2* vhat, const Herm48Operands* h48,
                         const CgSolve& s, int* d_iters, hipStream_t stream, const LanczosOut* lz, const MeanFusedOperands* fuse) {
    using namespace pcg;
    ToepGeom tg;
    const double2* twiddles[3] = {nullptr, nullptr, nullptr};
    if (squeeze_unit_axes(full, tw_full, &tg, twiddles) == 0) {
        set_error("persistent CG: a grid of a single cell has no transform to run");
        return EFGP_EUNSUPPORTED;
    }
    Args a;
    pass_geometry(tg, twiddles, a.g);
    solve_args(s, vhat, d_iters, lz, a);
#ifdef EFGP_CG_STAMPS
    {
        static long long* d_stamps = nullptr;
        if (!d_stamps) (void)hipMalloc((void**)&d_stamps, 16 * sizeof(long long));
        (void)hipMemsetAsync(d_stamps, 0, 16 * sizeof(long long), stream);
        a.stamps = d_stamps;
        g_last_stamps = d_stamps;
    }
#endif
    PersistentChoice c;
    if (const int rc = pick_persistent(full, s, h48 != nullptr && h48->vhat != nullptr, lz != nullptr, fuse != nullptr, &c)) return rc;
    const bool herm = c.pick == PersistentPick::fused48 || c.pick == PersistentPick::herm48 || c.pick == PersistentPick::herm64;
    const PickLaunch l = herm ? herm_launch(c, s.variant, h48, fuse, a) : launch_of(c, a.g);
    g_last_launch = l.what;
    if (const int rc = raise_dynamic_lds((const void*)l.kernel, l.lds, l.what)) return rc;
    {
        KernelTimer timer("cg_solve", stream);
        hipLaunchKernelGGL(l.kernel, dim3(s.nbatch), dim3(l.threads), l.lds, stream, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("persistent CG launch failed: %s", hipGetErrorString(e));
        return EFGP_EHIP;
    }
    return EFGP_OK;
}

}  // namespace efgp
