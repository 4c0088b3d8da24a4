// Stand-alone host program for the planners of csrc/cg_plan_host.cpp: what efgp_toeplitz_create_ex decides for a block, the grid a
// solve runs on, the kernel the persistent solve picks (pick=; lz_pick= in Lanczos mode) and the launch shape of the cooperative solve.  No device involved.
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/cg_plan_check.cpp gp-quadrature_amd/csrc/cg_plan_host.cpp gp-quadrature_amd/csrc/es_kernel.cpp -o cg_plan_check
//   ./cg_plan_check < cases      one case per line: dim n0 n1 n2 hermitian nbatch num_cu max_lds (n of the unused axes: 1)
//   ./cg_plan_check --sweep      every cooperative launch shape of blocks 33..256 per axis (takes minutes under the sanitizers)
//
// Hooks (EFGP_NO_*, EFGP_COOP_*) come from the environment, as in the library.  tests/test_cg_plan_host.py holds the case output
// to tests/_cg_routes.py.  The sweep asserts on every shape it reports ok what coop_enqueue relies on, that the general kernel with
// 4 entries per thread is never asked for a single workgroup per system (it has no such instantiation), and prints a digest.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../gp-quadrature_amd/csrc/cg_plan_host.hpp"
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
#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond) && ++fails <= 20)                                                                                        \
            std::fprintf(stderr, "FAILED %s (line %d): block %lld x %lld x %lld, grid %lld x %lld, %d systems, hermitian %d, max_lds %d\n", #cond, \
                         __LINE__, g_at[0], g_at[1], g_at[2], g_at[3], g_at[4], (int)g_at[5], (int)g_at[6], (int)g_at[7]);                \
    } while (0)
static long long g_at[8] = {};          // the case a failed check is reported for

static void print_grid(const char* key, int d, const int64_t* F) {
    std::printf(" %s=", key);
    for (int a = 0; a < d; ++a) std::printf("%s%lld", a ? "x" : "", (long long)F[a]);
}

static const char* pick_name(PersistentPick p) {
    static const char* names[] = {"fused48", "herm48", "herm64", "line1d", "fast64", "generic"};
    return names[(int)p];
}

static void print_coop(const char* key, const CoopShape& sh) {
    std::printf(" %s=ok:%d,herm:%d,G:%d,ks:%d,lpbc:%d,rows_wg:%d,cols_wg:%d,lines:%d,lds:%zu,spec_lds:%d,per:%d", key, (int)sh.ok, (int)sh.herm,
                sh.G, sh.ks, sh.lpbc, sh.rows_wg, sh.cols_wg, sh.lines, sh.lds, (int)sh.spec_lds, sh.per);
}

static void run_case(int dim, const int64_t* n, int herm, int nbatch, int num_cu, int max_lds) {
    int64_t Ls[3];
    for (int a = 0; a < 3; ++a) Ls[a] = 2 * n[a] - 1;
    const OperatorPlan pl = plan_operator(dim, Ls, /*force_pow2*/ 1, 0);
    print_grid("F", dim, pl.g.F);
    std::printf(" persistent_ok=%d cg64=%d h48=%d lines_ok=%d lines3_ok=%d", (int)pl.persistent_ok, (int)pl.embed64, (int)pl.h48, (int)pl.lines_ok,
                (int)pl.lines3_ok);
    if (pl.lines_ok) print_grid("coop_grid", 2, pl.coop_small ? pl.g_co.F : pl.g.F);
    int64_t shape[3];
    cg_solve_shape(pl.g, pl.persistent_ok, pl.h48, pl.embed64, pl.coop_small ? &pl.g_co : nullptr, herm, shape);
    print_grid("cg_shape", dim, shape);
    if (pl.persistent_ok && std::getenv("EFGP_NO_PERSISTENT_CG") == nullptr) {
        CgSolve s;
        s.hermitian = herm;
        s.nbatch = nbatch;
        PersistentChoice c;
        const ToepGeom& grid = pl.embed64 ? pl.g_cg : pl.g;
        CHECK(pick_persistent(grid, s, pl.h48, false, false, &c) == EFGP_OK);
        std::printf(" pick=%s dense48=%d", pick_name(c.pick), (int)c.dense48);
        print_grid("pick_grid", dim, grid.F);
        PersistentChoice lz;          // the same solve in Lanczos mode (efgp_lanczos): no line1d, no Hermitian kernel
        CHECK(pick_persistent(grid, s, pl.h48, true, false, &lz) == EFGP_OK);
        std::printf(" lz_pick=%s", pick_name(lz.pick));
    } else if (pl.lines_ok) {
        print_coop("coop", coop_shape(pl.coop_small ? pl.g_co : pl.g, nbatch, herm != 0, num_cu, max_lds));
    }
    std::printf("\n");
}

// what coop_enqueue and the kernels rely on in a shape reported ok
static void check_shape(const ToepGeom& g, const CoopShape& sh, int num_cu, int max_lds) {
    const int F0 = (int)g.F[0], F1 = (int)g.F[1], n0 = (int)g.n[0], n1 = (int)g.n[1];
    const int nrow = sh.herm ? (n0 + 1) / 2 : n0, ncol = sh.herm ? F1 / 2 : F1;
    CHECK(sh.G >= 1 && sh.G <= kCoopMaxG && sh.G <= num_cu);
    CHECK(sh.cols_wg * sh.G == ncol && sh.lpbc >= 1 && sh.cols_wg % sh.lpbc == 0);       // a whole pass count per workgroup
    CHECK(sh.rows_wg * sh.G >= nrow && sh.lines >= 1 && sh.lines <= sh.rows_wg);
    CHECK(sh.lds + 2048 <= (size_t)max_lds);
    CHECK(sh.per >= 1 && (int64_t)sh.G * sh.per <= num_cu);                                // every workgroup of a launch resident
    CHECK((sh.ks == 4 || sh.ks == 8) && sh.rows_wg * n1 <= sh.ks * kLineThreads);          // the vector entries a thread holds
    CHECK(sh.herm ? sh.lpbc * nrow <= (kCoopLoads / 2) * kLineThreads : sh.lpbc * F0 <= kCoopLoads * kLineThreads);   // ... and loads
    CHECK(sh.lines * F1 <= kCoopLoads * kLineThreads);
    CHECK(!(!sh.herm && sh.ks == 4 && sh.G == 1));                                         // cg_coop2d_kernel<4, true> does not exist
}

static uint64_t g_digest = 1469598103934665603ull;      // FNV-1a over every field of every shape
static void digest(uint64_t v) {
    for (int i = 0; i < 8; ++i) {
        g_digest ^= (v >> (8 * i)) & 0xff;
        g_digest *= 1099511628211ull;
    }
}

static int sweep() {
    const int num_cu = 256;
    long long shapes = 0, ok = 0, kernels[2][2][2] = {};
    for (int n0 = 33; n0 <= 256; ++n0) {
        for (int n1 = 33; n1 <= 256; ++n1) {
            const int64_t Ls[3] = {2 * n0 - 1, 2 * n1 - 1, 1};
            const OperatorPlan pl = plan_operator(2, Ls, 1, 0);
            CHECK(pl.lines_ok);
            for (int small = 0; small <= (pl.coop_small ? 1 : 0); ++small) {
                const ToepGeom& g = small ? pl.g_co : pl.g;
                for (int max_lds : {65536, 163840})
                    for (int herm = 0; herm <= 1; ++herm)
                        for (int nb = 1; nb <= 600; ++nb) {
                            const CoopShape sh = coop_shape(g, nb, herm != 0, num_cu, max_lds);
                            ++shapes;
                            for (uint64_t v : {(uint64_t)sh.ok, (uint64_t)sh.herm, (uint64_t)sh.G, (uint64_t)sh.ks, (uint64_t)sh.lpbc, (uint64_t)sh.rows_wg,
                                               (uint64_t)sh.cols_wg, (uint64_t)sh.lines, (uint64_t)sh.lds, (uint64_t)sh.spec_lds, (uint64_t)sh.per})
                                digest(v);
                            if (!sh.ok) continue;
                            ++ok;
                            ++kernels[sh.herm][sh.ks == 8][sh.G == 1];
                            const long long at[8] = {n0, n1, 1, g.F[0], g.F[1], nb, herm, max_lds};
                            for (int i = 0; i < 8; ++i) g_at[i] = at[i];
                            check_shape(g, sh, num_cu, max_lds);
                        }
            }
        }
    }
    std::printf("sweep: %lld shapes, %lld ok, digest %016llx\n", shapes, ok, (unsigned long long)g_digest);
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < 2; ++k)
            for (int s = 0; s < 2; ++s)
                std::printf("  %s<%d, %s>: %lld\n", h ? "cg_coop2d_herm_kernel" : "cg_coop2d_kernel", k ? 8 : 4, s ? "true" : "false", kernels[h][k][s]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--sweep") {
        sweep();
    } else {
        int dim, herm, nbatch, num_cu, max_lds;
        long long n[3];
        while (std::scanf("%d %lld %lld %lld %d %d %d %d", &dim, &n[0], &n[1], &n[2], &herm, &nbatch, &num_cu, &max_lds) == 8) {
            const int64_t nn[3] = {n[0], n[1], n[2]};
            const long long at[8] = {n[0], n[1], n[2], 0, 0, nbatch, herm, max_lds};
            for (int i = 0; i < 8; ++i) g_at[i] = at[i];
            CHECK(dim >= 1 && dim <= 3 && n[0] >= 1 && n[1] >= 1 && n[2] >= 1 && nbatch >= 1);
            if (fails) break;
            run_case(dim, nn, herm, nbatch, num_cu, max_lds);
        }
    }
    if (fails) std::fprintf(stderr, "%d checks FAILED\n", fails);
    return fails ? 1 : 0;
}
