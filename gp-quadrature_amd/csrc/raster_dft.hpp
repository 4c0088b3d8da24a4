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

}  // namespace efgp
