// Planning of the raster transform on the host (see raster_plan_host.hpp).  Pure arithmetic: no HIP runtime call, no device pointer.
#include "raster_plan_host.hpp"

#include <algorithm>

#include "common.hpp"

namespace efgp {

int plan_raster(int dim, const int64_t* n_modes, const int64_t* n_axis, int nbatch, int64_t max_workspace_bytes, RasterPlan* out) {
    EFGP_REQUIRE(out != nullptr, "raster plan: null output");
    EFGP_REQUIRE(dim >= 1 && dim <= 3 && n_modes && n_axis, "raster plan: dim must be 1, 2 or 3 with a mode count and a length per axis");
    EFGP_REQUIRE(nbatch >= 1 && nbatch <= kRasterMaxBatch, "raster plan: nbatch %d outside 1..%d", nbatch, kRasterMaxBatch);
    EFGP_REQUIRE(max_workspace_bytes >= 0, "raster plan: max_workspace_bytes must be >= 0 (0: the default cap)");
    for (int a = 0; a < dim; ++a) {
        EFGP_REQUIRE(n_modes[a] >= 1 && n_modes[a] <= kRasterMaxModes, "raster plan: n_modes[%d] = %lld outside 1..%lld", a, (long long)n_modes[a],
                     (long long)kRasterMaxModes);
        EFGP_REQUIRE(n_axis[a] >= 1 && n_axis[a] <= kRasterMaxAxis, "raster plan: n_axis[%d] = %lld outside 1..%lld", a, (long long)n_axis[a],
                     (long long)kRasterMaxAxis);
    }
    RasterPlan p;
    p.dim = dim;
    // the sizes above bound every product below by 2^16 * 2^4 * (2^40 + 2^51): summed in 128 bits, refused beyond 2^62
    typedef unsigned __int128 u128;
    const u128 limit = u128(1) << 62;
    const u128 cplx = 2 * sizeof(double);
    u128 tables = 0;
    for (int a = 0; a < dim; ++a) {
        p.Kpad[a] = (n_modes[a] + kRasterKStep - 1) / kRasterKStep * kRasterKStep;
        tables += u128(2) * sizeof(double) * (u128)n_axis[a] * (u128)p.Kpad[a];
    }
    u128 row = 0;
    if (dim == 1) tables += cplx * (u128)nbatch * (u128)p.Kpad[0];
    else if (dim == 2) row = cplx * (u128)nbatch * (u128)p.Kpad[1];
    else row = cplx * (u128)nbatch * ((u128)n_modes[1] * (u128)n_modes[2] + (u128)n_axis[1] * (u128)p.Kpad[2]);
    const u128 least = tables + (u128)kRasterTile * row;
    EFGP_REQUIRE(least < limit, "raster plan: the workspace of one tile-row slab does not fit 62 bits");
    const int64_t cap = max_workspace_bytes > 0 ? max_workspace_bytes : kRasterDefaultWorkspace;
    EFGP_REQUIRE((u128)cap >= least,
                 "raster plan: max_workspace_bytes = %lld cannot hold the phase tables and one slab of %d rows: %lld bytes needed", (long long)cap,
                 kRasterTile, (long long)(int64_t)least);
    p.table_bytes = (int64_t)tables;
    p.row_bytes = (int64_t)row;
    const int64_t whole = (n_axis[0] + kRasterTile - 1) / kRasterTile * kRasterTile;
    p.slab_rows = whole;
    if (p.row_bytes > 0) p.slab_rows = std::min(whole, (cap - p.table_bytes) / p.row_bytes / kRasterTile * kRasterTile);
    p.slabs = (n_axis[0] + p.slab_rows - 1) / p.slab_rows;
    p.workspace_bytes = p.table_bytes + p.slab_rows * p.row_bytes;
    *out = p;
    return EFGP_OK;
}

int plan_raster_type1(int dim, const int64_t* n_modes, const int64_t* n_axis, int nbatch, int64_t max_workspace_bytes, RasterPlan* out) {
    EFGP_REQUIRE(out != nullptr, "raster type-1 plan: null output");
    EFGP_REQUIRE(dim >= 1 && dim <= 3 && n_modes && n_axis, "raster type-1 plan: dim must be 1, 2 or 3 with a mode count and a length per axis");
    EFGP_REQUIRE(nbatch >= 1 && nbatch <= kRasterMaxBatch, "raster type-1 plan: nbatch %d outside 1..%d", nbatch, kRasterMaxBatch);
    EFGP_REQUIRE(max_workspace_bytes >= 0, "raster type-1 plan: max_workspace_bytes must be >= 0 (0: the default cap)");
    for (int a = 0; a < dim; ++a) {
        EFGP_REQUIRE(n_modes[a] >= 1 && n_modes[a] <= kRasterMaxModes, "raster type-1 plan: n_modes[%d] = %lld outside 1..%lld", a,
                     (long long)n_modes[a], (long long)kRasterMaxModes);
        EFGP_REQUIRE(n_axis[a] >= 1 && n_axis[a] <= kRasterMaxAxis, "raster type-1 plan: n_axis[%d] = %lld outside 1..%lld", a,
                     (long long)n_axis[a], (long long)kRasterMaxAxis);
    }
    RasterPlan p;
    p.dim = dim;
    // every product below is at most 2^16 * 2^4 * (2^23 * 2^51 + 2^60): summed in 128 bits, refused beyond 2^62
    typedef unsigned __int128 u128;
    const u128 limit = u128(1) << 62;
    const u128 cplx = 2 * sizeof(double);
    u128 tables = 0, modes = 1;
    for (int a = 0; a < dim; ++a) {
        p.Kpad[a] = (n_modes[a] + kRasterKStep - 1) / kRasterKStep * kRasterKStep;
        tables += u128(2) * sizeof(double) * (u128)n_axis[a] * (u128)p.Kpad[a];
        modes *= (u128)n_modes[a];
    }
    // a chunk of kRasterChunk rows holds one partial box of `modes` complex: cplx / kRasterChunk = 1 byte per row and mode
    static_assert(2 * sizeof(double) == kRasterChunk, "one byte of partial sums per row and mode");
    const u128 S = (u128)raster_segments(n_axis[dim - 1]);
    const u128 seg = S > 1 ? S : 0;               // copies of the GEMM's output kept per segment of a long last axis
    u128 row = 0;
    if (dim == 1) tables += cplx * (u128)nbatch * seg * (u128)n_modes[0];
    else if (dim == 2) row = (u128)nbatch * (cplx * (1 + seg) * (u128)n_modes[1] + modes);
    else row = (u128)nbatch * (cplx * ((1 + seg) * (u128)n_axis[1] * (u128)n_modes[2] + (u128)n_modes[1] * (u128)n_modes[2]) + modes);
    const u128 least = tables + (u128)kRasterTile * row;
    EFGP_REQUIRE(least < limit, "raster type-1 plan: the workspace of one tile-row slab does not fit 62 bits");
    const int64_t cap = max_workspace_bytes > 0 ? max_workspace_bytes : kRasterDefaultWorkspace;
    EFGP_REQUIRE((u128)cap >= least,
                 "raster type-1 plan: max_workspace_bytes = %lld cannot hold the phase tables and one slab of %d rows: %lld bytes needed",
                 (long long)cap, kRasterTile, (long long)(int64_t)least);
    p.table_bytes = (int64_t)tables;
    p.row_bytes = (int64_t)row;
    const int64_t whole = (n_axis[0] + kRasterTile - 1) / kRasterTile * kRasterTile;
    p.slab_rows = whole;
    if (p.row_bytes > 0) p.slab_rows = std::min(whole, (cap - p.table_bytes) / p.row_bytes / kRasterTile * kRasterTile);
    p.slabs = (n_axis[0] + p.slab_rows - 1) / p.slab_rows;
    p.workspace_bytes = p.table_bytes + p.slab_rows * p.row_bytes;
    *out = p;
    return EFGP_OK;
}

}  // namespace efgp
