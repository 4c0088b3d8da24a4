// Host-side planning of the raster transform (raster_dft.hip): the padded mode counts of the phase tables, the workspace a call takes
// and the slabs of the leading raster axis that keep it under a cap.  No HIP runtime call and no device pointer:
// tools/raster_plan_check.cpp links it without a device.  tests/_raster.py::plan restates it.
#pragma once
#include <cstdint>

namespace efgp {

constexpr int kRasterTile = 16;                                  // rows and columns of one MFMA output tile
constexpr int kRasterKStep = 4;                                  // K of v_mfma_f64_16x16x4_f64: the tables are padded to it
constexpr int64_t kRasterDefaultWorkspace = int64_t(256) << 20;  // the cap of max_workspace_bytes = 0
constexpr int64_t kRasterMaxModes = int64_t(1) << 20;            // per axis
constexpr int64_t kRasterMaxAxis = (int64_t(1) << 31) - 1;       // raster cells per axis (the raster itself may exceed 2^31 cells)
constexpr int kRasterMaxBatch = 1 << 16;

// Workspace layout of one call, in this order (every block a whole number of doubles):
//   per axis a: cos plane, sin plane, each (n_axis[a], Kpad[a]) doubles (the last axis's planes are stored mode-major: raster_dft.hip)
//   d = 1:      the scaled modes (nbatch, Kpad[0]) complex                                                   -- counted in table_bytes
//   d = 2:      T1 (nbatch, slab_rows, Kpad[1]) complex
//   d = 3:      T1 (nbatch, slab_rows, m1 * m2) complex, T2 (nbatch, slab_rows, n_axis[1], Kpad[2]) complex
struct RasterPlan {
    int dim = 0;
    int64_t Kpad[3] = {0, 0, 0};   // n_modes[a] rounded up to kRasterKStep
    int64_t table_bytes = 0;       // what does not depend on the slab height
    int64_t row_bytes = 0;         // intermediates per row of the leading raster axis (0 for d = 1)
    int64_t slab_rows = 0;         // a multiple of kRasterTile
    int64_t slabs = 0;
    int64_t workspace_bytes = 0;   // table_bytes + slab_rows * row_bytes
};

// EFGP_EINVAL with the error set for bad sizes and for a cap below table_bytes + kRasterTile * row_bytes (the message names the
// bytes needed).  max_workspace_bytes = 0: kRasterDefaultWorkspace.
int plan_raster(int dim, const int64_t* n_modes, const int64_t* n_axis, int nbatch, int64_t max_workspace_bytes, RasterPlan* out);

// The adjoint (type 1, raster_adjoint.hip): raster values in, a mode box out.  The last raster axis is contracted first (a GEMM),
// then the leading axes.  The reduction over the leading raster axis is split into partial sums over kRasterChunk rows each, added
// in chunk order; a slab is a whole number of chunks, so the sums do not depend on the slab plan.
constexpr int kRasterChunk = kRasterTile;
// The GEMM cuts a last raster axis longer than this into segments of this many cells, one workgroup column each, whose sums are
// added in segment order: a function of the axis length alone.
constexpr int64_t kRasterSegment = 256;
inline int64_t raster_segments(int64_t n_last) { return (n_last + kRasterSegment - 1) / kRasterSegment; }

// Workspace layout of one type-1 call, in this order, in the fields of RasterPlan:
//   per axis a: cos plane, sin plane, each (n_axis[a], Kpad[a]) doubles, all row-major
//   d = 1:      the GEMM's segments (nbatch, S, m0) complex where S = raster_segments(n_axis[0]) > 1   -- counted in table_bytes
//   d = 2:      T1 (nbatch, slab_rows, m1) complex, partial sums (nbatch, slab_rows / kRasterChunk, m0, m1) complex,
//               segments (nbatch, slab_rows, S, m1) complex where S = raster_segments(n_axis[1]) > 1
//   d = 3:      T1 (nbatch, slab_rows, n_axis[1], m2) complex, T2 (nbatch, slab_rows, m1 * m2) complex,
//               partial sums (nbatch, slab_rows / kRasterChunk, m0 * m1 * m2) complex,
//               segments (nbatch, slab_rows, n_axis[1], S, m2) complex where S = raster_segments(n_axis[2]) > 1
// The same refusals as plan_raster.
int plan_raster_type1(int dim, const int64_t* n_modes, const int64_t* n_axis, int nbatch, int64_t max_workspace_bytes, RasterPlan* out);

}  // namespace efgp
