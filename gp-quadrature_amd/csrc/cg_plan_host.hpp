// Host-side planning of the Toeplitz operator and of the CG launches (cg_plan_host.cpp): what efgp_toeplitz_create_ex decides for a
// block, the launch shape of the cooperative solve and the kernel the persistent solve picks.  No HIP runtime call and no device
// pointer: tools/cg_plan_check.cpp links it without a device.  The constants the planners share with the kernels live here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "toeplitz_cg.hpp"

namespace efgp {

constexpr int kLineThreads = 256;             // threads of the line-transform and cooperative kernels (cg_multi.hip, cg_coop2d.hip)
constexpr int kCoopMaxG = 64;                 // most workgroups per system of the cooperative solve
constexpr int kCoopLoads = 16;                // grid elements a thread brings in per phase (lpbc F0 / 256 and lines F1 / 256 at most)

namespace pcg {
constexpr int kThreads = 512;
constexpr int kSlots = 4;            // vector elements per thread (M <= kSlots * kThreads)
constexpr int kMaxGrid = 4608;       // complex elements per ping-pong buffer (2 x 72 KB = 144 KB LDS)
namespace l1d {
constexpr int KS = 4;
}  // namespace l1d
}  // namespace pcg

// cells of the two fixed circulant grids of the small 2-D blocks: the 64 x 64 grid (own or embedding) and the 48 x 48 grid of
// the Hermitian solves; an operator's blocks are taken and freed by these sizes
constexpr int64_t kCells64 = 64 * 64;
constexpr int64_t kCells48 = 48 * 48;
constexpr size_t kSpectrum64Bytes = (size_t)kCells64 * sizeof(double2);
constexpr size_t kSpectrum48Bytes = (size_t)kCells48 * sizeof(double2);
inline size_t spectrum_bytes(const ToepGeom& g) { return (size_t)g.Ftot * sizeof(double2); }
inline size_t real_spectrum_bytes(const ToepGeom& g) { return (size_t)g.Ftot * sizeof(double); }

// every axis of F a power of two in [lo, hi]
bool pow2_axes_within(int dim, const int64_t* F, int64_t lo, int64_t hi);
// the geometry whose block is the lag box L (n := L, M := prod L) on g's grid: what the pad kernel needs to lay the Toeplitz
// vector out for its transform
ToepGeom lag_geometry(const ToepGeom& g, const int64_t* Ls);

// What efgp_toeplitz_create_ex decides for a block, before any allocation or launch (tests/_cg_routes.py::operator restates it).
// A step that fails at run time (a twiddle table, a pooled block) takes back the decisions that needed it.
struct OperatorPlan {
    ToepGeom g;                  // the reference's grid
    int64_t Ls[3];
    bool want48 = false;         // Hermitian solves of blocks up to 23 x 23 on the 48 x 48 grid: take its spectrum block
    bool vhat_fused = false;     // the own grid is 64 x 64: its spectrum comes from the one-launch kernels
    bool h48 = false;            // ... and a launch that makes a 64 x 64 spectrum (own grid or embedding) carries the 48 x 48 one
    bool defer_pair = false;     // that launch is left to the fused mean solve / first use (EFGP_TOEPLITZ_DEFER_SPECTRA)
    bool defer_ref = false;      // cooperative grids: keep the lags, make the reference grid's spectrum on first use
    bool eligible = false;       // persistent_cg_eligible(g)
    bool persistent_ok = false;  // ... and not a grid of one cell without the embedding
    bool lines_ok = false;       // 2-D, power-of-two F in [128, 512]
    bool lines3_ok = false;      // 3-D, power-of-two F in [64, 256]
    bool coop_small = false;     // a smaller grid of the ladder 96 .. 512 holds 2 n - 1: the cooperative solve runs on g_co
    ToepGeom g_co;
    bool embed64 = false;        // blocks up to 32 x 32 on grids below 64 x 64: the single-launch solves run on g_cg
    ToepGeom g_cg;
    // bytes of the pooled blocks the operator may own
    size_t vhat_bytes = 0, v_keep_bytes = 0, vhat_co_bytes = 0;
};
// flags: EFGP_TOEPLITZ_* of the C ABI.  Reads the creation-time hooks (EFGP_NO_CG48, EFGP_NO_CG64, EFGP_NO_CG_HERM,
// EFGP_NO_DEFER_SPECTRA, EFGP_NO_COOP_SMALL, EFGP_EAGER_REF_SPECTRUM, EFGP_NO_CG64_EMBED, EFGP_NO_VHAT64).
OperatorPlan plan_operator(int dim, const int64_t* Ls, int force_pow2, int flags);

// efgp_toeplitz_cg_shape: the grid a solve runs on, from what the operator holds (h48: the 48 x 48 operands; cg64: the 64 x 64
// embedding; g_co: the smaller cooperative grid, or null).  Reads EFGP_NO_CG48, EFGP_NO_COOP_SMALL and EFGP_NO_CG_COOP.
void cg_solve_shape(const ToepGeom& g, bool persistent_ok, bool h48, bool cg64, const ToepGeom* g_co, int hermitian, int64_t* shape_out);

// launch shape of the cooperative solve (cg_coop2d_kernel / cg_coop2d_herm_kernel) of nbatch systems on grid g
struct CoopShape {
    bool ok = false;             // a launch shape fits (else the caller goes to the multi-launch solver)
    bool herm = false;           // the Hermitian kernel: rows k0 >= 0 only, column pairs
    int G = 0;                   // workgroups per system
    int ks = 0;                  // vector entries per thread: 4 or 8
    int lpbc = 0;                // columns per LDS pass of the column phase
    int rows_wg = 0, cols_wg = 0;
    int lines = 0;               // rows per LDS pass of the row phases
    size_t lds = 0;              // dynamic LDS bytes
    bool spec_lds = false;       // Hermitian: the workgroup's slice of the spectrum stays in LDS
    int per = 0;                 // systems per launch (one workgroup per CU)
};
CoopShape coop_shape(const ToepGeom& g, int nbatch, bool hermitian, int num_cu, int max_lds);

// the kernel persistent_cg_launch runs, by the CALLER's shape (a block with a unit axis runs the generic kernel on its other axes)
enum class PersistentPick { fused48, herm48, herm64, line1d, fast64, generic };
struct PersistentChoice {
    PersistentPick pick = PersistentPick::generic;
    bool dense48 = false;        // 48 x 48 kernels: per-frequency Toeplitz products (one system, no EFGP_CG48_FFT2D)
};
// have_h48: the operator holds the 48 x 48 operands; lanczos / fuse: the modes of persistent_cg_launch.  EFGP_EUNSUPPORTED (with the
// error set) for a fuse request that is not a cold-start 48 x 48 Hermitian mean solve.
int pick_persistent(const ToepGeom& full, const CgSolve& s, bool have_h48, bool lanczos, bool fuse, PersistentChoice* out);

}  // namespace efgp
