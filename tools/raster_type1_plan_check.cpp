// Stand-alone host program for the type-1 planner of csrc/raster_plan_host.cpp (plan_raster_type1): the padded mode counts, the
// table and per-row bytes, the slab height and the slab count of a raster type-1 transform under a workspace cap.  No device involved.
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/raster_type1_plan_check.cpp gp-quadrature_amd/csrc/raster_plan_host.cpp -o raster_type1_plan_check
//   ./raster_type1_plan_check < cases      one case per line: dim m0 m1 m2 n0 n1 n2 nbatch max_workspace_bytes (unused axes: 1)
//
// One line per case: ok=1 Kpad=AxBxC table_bytes=.. row_bytes=.. slab_rows=.. slabs=.. workspace_bytes=.., or ok=0 for a case the
// planner refuses (its message goes to stderr).  On every accepted case the program asserts what the launcher relies on: the slabs
// cover the leading axis, the slab height is a whole number of tiles and of reduction chunks, the partial sums of a slab are whole
// complex numbers and the workspace stays under the cap.  tests/test_raster_type1_host.py holds the output to
// tests/_raster_adjoint.py::plan.
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../gp-quadrature_amd/csrc/raster_plan_host.hpp"
#include "../include/efgp_hip.h"

namespace efgp {
void set_error(const char* fmt, ...) {          // what csrc/common.cpp provides inside the library
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    std::fputc('\n', stderr);
    va_end(ap);
}
}  // namespace efgp

using namespace efgp;

static int fails = 0;
static int g_case = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond) && ++fails <= 20) std::fprintf(stderr, "FAILED %s (line %d), case %d\n", #cond, __LINE__, g_case); \
    } while (0)

int main() {
    int dim, nbatch;
    long long m[3], n[3], cap;
    while (std::scanf("%d %lld %lld %lld %lld %lld %lld %d %lld", &dim, &m[0], &m[1], &m[2], &n[0], &n[1], &n[2], &nbatch, &cap) == 9) {
        ++g_case;
        const int64_t mm[3] = {m[0], m[1], m[2]}, nn[3] = {n[0], n[1], n[2]};
        RasterPlan p;
        const int rc = plan_raster_type1(dim, mm, nn, nbatch, cap, &p);
        if (rc != EFGP_OK) {
            CHECK(rc == EFGP_EINVAL);
            std::printf("ok=0\n");
            continue;
        }
        const int64_t limit = cap > 0 ? cap : kRasterDefaultWorkspace;
        CHECK(p.slab_rows >= kRasterTile && p.slab_rows % kRasterTile == 0 && p.slab_rows % kRasterChunk == 0);
        CHECK(p.slabs >= 1 && p.slabs * p.slab_rows >= nn[0] && (p.slabs - 1) * p.slab_rows < nn[0]);
        CHECK(p.workspace_bytes == p.table_bytes + p.slab_rows * p.row_bytes && p.workspace_bytes <= limit);
        CHECK(p.table_bytes % 16 == 0 && (p.slab_rows * p.row_bytes) % 16 == 0);
        for (int a = 0; a < dim; ++a) CHECK(p.Kpad[a] >= mm[a] && p.Kpad[a] < mm[a] + kRasterKStep && p.Kpad[a] % kRasterKStep == 0);
        std::printf("ok=1 Kpad=");
        for (int a = 0; a < dim; ++a) std::printf("%s%lld", a ? "x" : "", (long long)p.Kpad[a]);
        std::printf(" table_bytes=%lld row_bytes=%lld slab_rows=%lld slabs=%lld workspace_bytes=%lld\n", (long long)p.table_bytes,
                    (long long)p.row_bytes, (long long)p.slab_rows, (long long)p.slabs, (long long)p.workspace_bytes);
    }
    if (fails) std::fprintf(stderr, "%d checks FAILED\n", fails);
    return fails ? 1 : 0;
}
