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

}  // namespace efgp
