// Type-2 transform onto a rectilinear raster (raster_dft.hip): the output points are the tensor product of d coordinate vectors, so
// the transform separates into one contraction per axis with per-axis phase tables -- no spreading window, no tolerance.
#pragma once
#include <cstdint>

#include "common.hpp"
#include "raster_plan_host.hpp"

namespace efgp {

struct RasterCall {
    int dim = 0;
    int64_t m[3] = {1, 1, 1};        // modes per axis
    int64_t n[3] = {1, 1, 1};        // raster cells per axis
    double h[3] = {0, 0, 0};
    double xcen[3] = {0, 0, 0};
    const double* axes = nullptr;    // device: the d coordinate vectors, concatenated
    const double2* f = nullptr;      // device: (nbatch, prod m)
    const double2* scale = nullptr;  // device: (prod m) or null
    int nbatch = 1;
    int isign = +1;
    int modeord = 0;
    double* out = nullptr;           // device: (nbatch, n...)
};

// Enqueues the whole transform on `stream` with the workspace `ws` (plan.workspace_bytes) laid out as raster_plan_host.hpp says.
int raster_type2_enqueue(const RasterCall& c, const RasterPlan& plan, void* ws, hipStream_t stream);

// The phase tables of one axis (raster_table_kernel): cos / sin planes of exp(isign 2 pi i h k (x[j] - xcen)), n x Kpad doubles each,
// zero in the columns m <= s < Kpad; by_mode: stored mode-major (element (j, s) at s * n + j), else row-major.
void raster_table_enqueue(hipStream_t stream, const double* x, int64_t n, int64_t m, int64_t Kpad, double h, double xcen, int isign, int modeord,
                          int by_mode, double* cosp, double* sinp);

// The adjoint (raster_adjoint.hip): raster values in, a mode box out,
//     out[b, k] = sum_j values[b, j] * cell_scale[j] * exp(isign 2 pi i sum_a h[a] k_a (axis_a[j_a] - xcen[a])).
struct RasterAdjointCall {
    int dim = 0;
    int64_t m[3] = {1, 1, 1};
    int64_t n[3] = {1, 1, 1};
    double h[3] = {0, 0, 0};
    double xcen[3] = {0, 0, 0};
    const double* axes = nullptr;        // device: the d coordinate vectors, concatenated
    const double* values = nullptr;      // device: (nbatch, n...)
    const double* cell_scale = nullptr;  // device: (n...) or null; a cell whose scale is 0 is left out whatever its value holds
    int nbatch = 1;
    int isign = -1;
    int modeord = 0;
    double2* out = nullptr;              // device: (nbatch, m...)
};

// Enqueues the transform on `stream` with the workspace `ws` (plan.workspace_bytes, from plan_raster_type1).
int raster_type1_enqueue(const RasterAdjointCall& c, const RasterPlan& plan, void* ws, hipStream_t stream);

}  // namespace efgp
