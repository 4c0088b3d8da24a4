// The Toeplitz operator object and the few host functions that cross its translation units (internal to the library):
//   toeplitz_cg.hip : creation, the spectra ladder, the C ABI entries and the dispatch of a solve
//   cg_coop2d.hip   : the cooperative single-launch solve of the 2-D grids 96^2 .. 512^2
//   cg_multi.hip    : the multi-launch solver of every other grid
// Everything else in those files is static.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "cg_plan_host.hpp"
#include "common.hpp"
#include "toeplitz_cg.hpp"

struct efgp_toeplitz_s {
    int device = 0;
    efgp::DeviceCtx* ctx = nullptr;
    efgp::ToepGeom g;
    int64_t Ls[3] = {1, 1, 1};
    double2* vhat = nullptr;
    double2* tw[3] = {nullptr, nullptr, nullptr};   // exp(-2 pi i q / F[a]) tables for the persistent CG
    bool persistent_ok = false;
    bool lines_ok = false;       // 2-D, power-of-two F in [128, 512]: fused line-FFT CG iteration
    bool lines3_ok = false;      // 3-D, power-of-two F in [64, 256]: the same with five pruned line passes
    // 2-D blocks of up to 16 x 16 modes (circulant grids 8^2 .. 32^2): the CG solves run on a 64 x 64 embedding instead, through
    // the specialised 64 x 64 kernels (any F >= 2 n - 1 embeds the Toeplitz product exactly; measured 3.1 us per iteration
    // against 9-11 us of the generic kernel on the 32 x 32 grid).  fft_shape / efgp_toeplitz_apply keep the reference's grid.
    double2* vhat_c = nullptr;   // lines_ok grids: centred spectrum for the cooperative solve (center_spectrum_kernel)
    // Round 4: the cooperative solve runs on the smallest grid of the in-wave transforms (64 R or 48 R: 96, 128, 192, 256, 384, 512)
    // that holds 2 n - 1 -- 141 -> 192 instead of 256, 81 -> 96 instead of 128 (0.56 x the grid).  fft_shape, efgp_toeplitz_apply
    // and the multi-launch iteration keep the reference's power-of-two grid.
    bool coop_small = false;
    efgp::ToepGeom g_co;
    double2* vhat_co = nullptr;  // centred spectrum on g_co
    // ... and the spectrum on the reference's grid (`vhat`) is then made on first use (ensure_reference_spectrum) from a copy of
    // the Toeplitz vector: a fit only runs the cooperative solve, which never reads it (pad | two transform passes per operator)
    bool vhat_ready = true;
    double2* v_keep = nullptr;
    size_t v_keep_bytes = 0;
    double2* tw_co[2] = {nullptr, nullptr};
    double* vc3 = nullptr;       // lines3_ok grids: REAL centred spectrum of the Hermitian 3-D iteration, built on first use
    efgp::ToepGeom g_cg;
    double2* vhat_cg = nullptr;
    double2* tw_cg[3] = {nullptr, nullptr, nullptr};
    bool cg64 = false;
    // 2-D blocks of up to 23 x 23 modes (2 n - 1 <= 48): the HERMITIAN solves (the model's mean systems) run on the smallest
    // circulant grid, 48 x 48 (cg_herm48_kernel, round 4), from a third spectrum made in the same launch as the 64 x 64 one
    double2* vhat48 = nullptr;
    efgp::Herm48Operands h48 = {nullptr, nullptr};
    // deferred spectra (efgp_toeplitz_create_ex with EFGP_TOEPLITZ_DEFER_SPECTRA): creation launches nothing.  The fused mean solve
    // (efgp_cg_solve_mean_fused) makes vhat48 in its prologue; the first other use makes what is still missing (ensure_deferred_spectra)
    // from the caller's Toeplitz vector, which is not copied: the caller keeps it alive and unchanged while the operator lives
    bool pair_pending = false;   // the 64 x 64 spectrum (pair_target: vhat, or vhat_cg of the embedding) is still to be made
    bool vhat48_ready = true;
    const double2* v_ref = nullptr;
    double2* pair_target = nullptr;
};

namespace efgp {

inline dim3 grid_for(int64_t work, int rows, int threads, int cap = 1024) {
    int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((work + threads - 1) / threads, cap));
    return dim3(blocks, rows);
}

// ---- toeplitz_cg.hip ---------------------------------------------------------------------------------------------------------------
// pad[row][:] = 0 except the leading n-box which receives scale .* src[rows[row]] (scale may be null), times the real `factor`:
// the multi-launch solver pads x0 with it for r_0 = b - A x_0
__global__ void pad_scale_kernel(ToepGeom g, const double2* __restrict__ src, int64_t src_stride,
                                 const double2* __restrict__ scale, const int* __restrict__ rows,
                                 const int* __restrict__ row_active, double2* __restrict__ pad, double factor);
// the spectrum on the reference's grid, made on first use when the operator was created with a smaller cooperative grid
int ensure_reference_spectrum(efgp_toeplitz_s* op, hipStream_t stream);
// pad = FFT^-1( FFT(pad) .* vhat ) for `slots` rows
int circulant(efgp_toeplitz_s* op, double2* pad, int slots, hipStream_t stream);
// vhat_c = vhat rotated so that the circular convolution has its crop window at [0, n) (cooperative solve on the reference's grid)
bool ensure_centred_spectrum(efgp_toeplitz_s* op, hipStream_t stream);

// ---- cg_coop2d.hip -----------------------------------------------------------------------------------------------------------------
// what a synchronous caller needs after the enqueue: the status word, the shape that ran, the diagnostic stamps
struct CoopInfo {
    int* d_status = nullptr;
    CoopShape shape;
    double* stamps = nullptr;
    int dbg = 0;
};
// Enqueues the cooperative solve of `nbatch` systems on a 2-D 128^2..512^2 grid in the launch shape coop_shape gives.  Iteration
// counts go to d_iters (device, nbatch ints; -3 where a grid barrier died), *d_status (device int) is non-zero when one did.
// EFGP_EUNSUPPORTED when no launch shape fits.
int coop_enqueue(efgp_toeplitz_s* op, const CgSolve& s, int* d_iters, hipStream_t stream, CoopInfo* info, int nan_on_dead);
// diagnostic runs of the cooperative solve (EFGP_COOP_DBG=2): the phase shares of workgroup 0, system 0
int coop_print_stamps(const CoopInfo& ci, int iters0);

// ---- cg_multi.hip ------------------------------------------------------------------------------------------------------------------
// The multi-launch solve of s.nbatch systems on any grid; returns when they are solved.  The counts follow the reference's two
// conventions (cg.py:152 single; cg.py:193-199,243 batched: +1 for the terminating pass).
int solve_multi_launch(efgp_toeplitz_s* op, const CgSolve& s, int* iters_out, int* row_iters_out, hipStream_t stream);

}  // namespace efgp
