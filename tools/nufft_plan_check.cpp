// Stand-alone host program for the planners of csrc/nufft_plan_host.cpp: the window rule, the tile geometry, the level of the point
// layout a pass wants, the route of one type-1 pass and of one type-2 call.  No device involved.
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/nufft_plan_check.cpp gp-quadrature_amd/csrc/nufft_plan_host.cpp gp-quadrature_amd/csrc/es_kernel.cpp -o nufft_plan_check
//   ./nufft_plan_check < cases     one case per line, every field a number but the first:
//       t1     dim nm0 nm1 nm2              tol N channels  batch normal dense layout span0 span1 span2 num_cu max_lds
//       t1pair dim nm0 nm1 nm2 nb0 nb1 nb2  tol N channels  batch normal dense layout span0 span1 span2 num_cu max_lds
//       t2     dim nm0 nm1 nm2              tol N real_only batch normal dense layout span0 span1 span2 num_cu max_lds
//     (mode counts of the unused axes: 1; t1pair: the two boxes of the fit's pair pass, the window is made for the larger; dense: 1
//     takes the dense rule's window whatever N; layout: 0 no point layout, 1 | 8 a layout and that band height forced, -1 a layout and
//     the unforced rule; span: extent of the points per axis in periods; a pass on the layout also prints the chunk length of its level)
//   ./nufft_plan_check --sweep     the products listed at sweep() (a second unsanitized, two under the sanitizers)
//
// Hooks (EFGP_NO_*, EFGP_CELLSORT, EFGP_DENSE_POINTS, EFGP_G2M_V1 ...) come from the environment, as in the library; only
// EFGP_MFMA_BAND_CELLS is set from the case's layout field.  tests/test_nufft_plan_host.py holds the case output to
// tests/_nufft_routes.py.  The sweep asserts on every plan what the drivers and kernels of nufft.hip rely on and prints a digest.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>

#include "../gp-quadrature_amd/csrc/line_fft.hpp"
#include "../gp-quadrature_amd/csrc/nufft_plan_host.hpp"
#include "../gp-quadrature_amd/csrc/points_layout.hpp"
#include "../gp-quadrature_amd/csrc/spread_mfma.hpp"

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
static std::string g_at;          // the case a failed check is reported for
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond) && ++fails <= 20) std::fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, g_at.c_str()); \
    } while (0)

static const char* kSpreaders[] = {"layout", "cells", "tiles", "lds_pad_raw48", "lds_pad_61", "lds_plain", "global"};
static const char* kAfter[] = {"g2m_from_acc", "g2m", "pruned_from_acc", "pruned", "fft"};
static const char* kGrids[] = {"image", "direct", "pruned", "fft"};
static const char* kGathers[] = {"tiles", "pair", "halo", "lds", "l2"};

static void print_axes(const char* key, int d, const int64_t* v) {
    std::printf(" %s=", key);
    for (int a = 0; a < d; ++a) std::printf("%s%lld", a ? "x" : "", (long long)v[a]);
}
static void print_tile(int d, const TileGeom& t) {
    int64_t nt[3], T[3];
    for (int a = 0; a < 3; ++a) {
        nt[a] = t.nt[a];
        T[a] = t.T[a];
    }
    print_axes("tile_nt", d, nt);
    print_axes("tile_T", d, T);
    std::printf(" nbins=%d", t.nbins);
}

struct Case {
    bool type2 = false, pair = false;
    int dim = 1;
    int64_t nm[3] = {1, 1, 1}, nmb[3] = {1, 1, 1};
    double tol = 1e-6;
    long long N = 0;
    int chan = 1;            // channels (type 1), real_only (type 2)
    int batch = 1, normal = 0, dense = 0, layout = 0;
    double span[3] = {1, 1, 1};
    int num_cu = 256, max_lds = 163840;
};

static NufftSite site_of(const Case& c) {
    NufftSite s;
    s.dim = c.dim;
    s.npts = c.N;
    s.tol = c.tol;
    s.num_cu = c.num_cu;
    s.max_lds = c.max_lds;
    for (int a = 0; a < 3; ++a) {
        s.h[a] = 1.0;              // one period per unit: the points lie in [0, span]
        s.hi[a] = c.span[a];
    }
    s.has_layout = c.layout != 0;
    return s;
}

// windows are designed once per (dimension, box, tolerance, rule): the sweep asks for each many times
static const WindowPlan& window_of(int dim, const int64_t* box, double tol, bool dense) {
    static std::map<std::tuple<int, int64_t, int64_t, int64_t, double, bool>, WindowPlan> cache;
    const auto key = std::make_tuple(dim, box[0], box[1], box[2], tol, dense);
    auto it = cache.find(key);
    if (it == cache.end()) {
        it = cache.emplace(key, WindowPlan()).first;
        plan_window(dim, box, tol, dense, &it->second);
    }
    return it->second;
}

static void force_band(int layout) {
    if (layout > 0) setenv("EFGP_MFMA_BAND_CELLS", std::to_string(layout).c_str(), 1);
    else unsetenv("EFGP_MFMA_BAND_CELLS");
}

struct Planned {
    const WindowPlan* w;
    Type1Plan t1;
    Type2Plan t2;
};

static Planned plan_case(const Case& c) {
    Planned out;
    int64_t box[3];
    for (int a = 0; a < 3; ++a) box[a] = c.pair ? std::max(c.nm[a], c.nmb[a]) : c.nm[a];
    out.w = &window_of(c.dim, box, c.tol, c.dense != 0 || window_dense(c.dim, c.N));
    const NufftSite s = site_of(c);
    force_band(c.layout);
    if (c.type2) {
        out.t2 = plan_type2(s, out.w->nf, out.w->p, c.nm, c.batch, c.chan != 0);
    } else {
        ModeBoxes req;
        req.part = c.pair ? 4 : 0;
        for (int a = 0; a < 3; ++a) {
            req.nma[a] = c.nm[a];
            req.nmb[a] = c.pair ? c.nmb[a] : 1;
        }
        out.t1 = plan_type1(s, out.w->nf, out.w->p, c.chan, c.normal != 0, c.batch, &req);
    }
    return out;
}

static void print_case(const Case& c, const Planned& pl) {
    const int d = c.dim;
    const WindowPlan& w = *pl.w;
    print_axes("nf", d, w.nf);
    std::printf(" W=%d degree=%d dense=%d", w.p.w, w.p.degree, (int)w.dense);
    if (c.type2) {
        const Type2Plan& r = pl.t2;
        std::printf(" grid=%s gather=%s cplx=%d direct=%d halo=%d pair=%d image=%d lds_bytes=%zu pair_bytes=%zu use_lds=%d nwg=%d class_order=%d"
                    " fine_bytes=%zu ccells=%lld region=%lld",
                    kGrids[(int)r.grid], kGathers[(int)r.gather], (int)r.cplx, (int)r.direct_grid, (int)r.use_halo, (int)r.use_pair, (int)r.use_image,
                    r.lds_bytes, r.pair_bytes, (int)r.use_lds, r.nwg, (int)r.class_order, r.fine_bytes, (long long)r.ccells, (long long)r.region);
        print_axes("nc", d, r.nc);
        if (r.gather == Gather::tiles) print_tile(d, r.tile);
    } else {
        const Type1Plan& p = pl.t1;
        std::printf(" spreader=%s after=%s use_lds=%d lds_bytes=%zu nwg=%d nslab=%d per=%lld pad_bytes=%zu class_order=%d sum_bits=%d sum_points=%lld"
                    " level_bands=%d band_cells=%d work_cells=%lld g2m_two_launch=%d g2m_split=%d g2m_h=%dx%d",
                    kSpreaders[(int)p.spreader], kAfter[(int)p.after], (int)p.use_lds, p.lds_bytes, p.nwg, p.nslab, (long long)p.per, p.pad_bytes,
                    (int)p.class_order, p.sum_bits, (long long)p.sum_points, p.level.nbands, p.level.band_cells, (long long)p.work_cells,
                    (int)p.g2m_two_launch, p.g2m_split, p.g2m_h[0], p.g2m_h[1]);
        print_axes("nc", d, p.nc);
        if (p.spreader == Spreader::tiles || p.spreader == Spreader::cells) print_tile(d, p.tile);
        if (p.spreader == Spreader::layout) std::printf(" chunk_len=%d", chunk_length(c.N, c.num_cu));      // what points_layout.hip cuts the bands into
    }
    std::printf("\n");
}

// ---- what the drivers and kernels rely on ---------------------------------------------------------------------------------------
static void check_tile(const TileGeom& t, int d, const int64_t* nf, int W, int channels, int max_lds, bool single_cells) {
    CHECK((size_t)t.ext[0] * t.ext[1] * t.ext[2] * channels * 8 <= (size_t)max_lds - 4096);
    CHECK(t.nbins >= 1 && t.nbins <= 16384 && t.W == W && t.d == d);
    int bins = 1;
    for (int a = 0; a < d; ++a) {
        CHECK(t.nf[a] == nf[a] && t.T[a] >= 1 && t.nt[a] >= 1 && (int64_t)t.T[a] * t.nt[a] >= nf[a] && t.ext[a] == t.T[a] + W - 1);
        CHECK(!single_cells || t.T[a] == 1);
        bins *= t.nt[a];
    }
    CHECK(bins == t.nbins);
}

static void check_crop(int d, const int64_t* nc, const int64_t* nf, bool pruned) {
    bool smaller = false;
    for (int a = 0; a < d; ++a) {
        CHECK(nc[a] >= 1 && nc[a] <= nf[a]);
        smaller = smaller || nc[a] < nf[a];
    }
    CHECK(!pruned || smaller);
    CHECK(!pruned || own_fft_supported(d, nf));
}

static void check_type1(const Case& c, const Planned& pl) {
    const Type1Plan& p = pl.t1;
    const WindowPlan& w = *pl.w;
    const int64_t cells = w.nf[0] * w.nf[1] * w.nf[2];
    const int W = w.p.w;
    switch (p.spreader) {
        case Spreader::layout:
            CHECK(c.dim == 2 && W <= kMfmaMaxW && p.level.nbands >= 1 && p.level.nbands <= kMaxBands &&
                  (p.level.nbands & (p.level.nbands - 1)) == 0 && (p.level.band_cells == 1 || p.level.band_cells == 8));
            CHECK(c.N >= 32768 && c.N < ((int64_t)1 << 31) && p.sum_bits == 61 && p.sum_points == c.N);
            break;
        case Spreader::cells:
            CHECK(c.dim == 2 && W <= kCellMaxW && cells <= 16384 && w.p.degree <= W + 4 && !c.normal && c.N > 0);
            check_tile(p.tile, c.dim, w.nf, W, c.chan, c.max_lds, true);
            break;
        case Spreader::tiles:
            CHECK(!p.use_lds && c.N >= 32768 && p.sum_bits == 61 && p.sum_points == c.N);
            check_tile(p.tile, c.dim, w.nf, W, c.chan, c.max_lds, false);
            break;
        default: {
            const bool raw48 = p.spreader == Spreader::lds_pad_raw48, pad = raw48 || p.spreader == Spreader::lds_pad_61;
            CHECK(p.use_lds == (p.spreader != Spreader::global));
            CHECK(p.nwg >= 1 && (int64_t)p.nwg * p.per >= c.N && p.nslab == (p.use_lds ? p.nwg : 1));
            if (p.use_lds) {
                CHECK(c.N > 0 && (int64_t)p.nslab * p.per >= c.N && p.nslab <= 512);      // reduce_slabs_kernel adds at most 512 raw slabs
                CHECK(p.lds_bytes == (size_t)c.chan * cells * 8 && p.lds_bytes <= (size_t)c.max_lds);
            }
            if (pad) CHECK(p.pad_bytes + 4608 <= (size_t)c.max_lds && p.pad_bytes >= p.lds_bytes);
            CHECK(raw48 ? (p.sum_bits == 46 && p.sum_points == p.per && !c.normal) : (p.sum_bits == 61 && p.sum_points == c.N));
            CHECK(!p.class_order || (pad && c.dim >= 2 && c.N >= (int64_t)kOrderWindow * 64));
        }
    }
    const bool g2m = p.after == AfterSpread::g2m || p.after == AfterSpread::g2m_from_acc;
    const bool pruned = p.after == AfterSpread::pruned || p.after == AfterSpread::pruned_from_acc;
    if (g2m) {
        CHECK(c.dim == 2 && w.nf[0] <= kG2MMaxNf && w.nf[1] <= kG2MMaxNf && p.g2m_h[0] <= kG2MMaxH && p.g2m_h[1] <= kG2MMaxH);
        CHECK(p.g2m_h[0] == std::max(c.nm[0] / 2, c.pair ? c.nmb[0] / 2 : (int64_t)0) && p.g2m_h[1] == std::max(c.nm[1] / 2, c.pair ? c.nmb[1] / 2 : (int64_t)0));
        CHECK(p.g2m_split >= 1 && p.g2m_split <= 16 && (p.g2m_split == 1 || !p.g2m_two_launch));
        CHECK(p.g2m_split == 1 || ((int64_t)(p.g2m_h[0] / 2 + 1) * c.batch * p.g2m_split <= 4096 && (size_t)(p.g2m_h[0] / 2 + 1) * c.batch * 4 <= 65536));
        CHECK((256 + (size_t)kG2RRows * w.nf[1]) * 16 <= 65536);                           // grid_rows_kernel's LDS needs no opt-in
    }
    CHECK((p.after == AfterSpread::g2m_from_acc) == (g2m && p.spreader == Spreader::layout));
    CHECK(p.after != AfterSpread::pruned_from_acc || p.spreader == Spreader::layout || p.spreader == Spreader::tiles);
    if (pruned) {
        check_crop(c.dim, p.nc, w.nf, true);
        int64_t wk = c.batch;
        for (int a = 0; a < c.dim; ++a) wk *= a == c.dim - 1 ? p.nc[a] : w.nf[a];
        CHECK(p.work_cells == wk);
    }
}

static void check_type2(const Case& c, const Planned& pl) {
    const Type2Plan& r = pl.t2;
    const WindowPlan& w = *pl.w;
    const int64_t cells = w.nf[0] * w.nf[1] * w.nf[2];
    CHECK(r.cplx == (c.chan == 0));
    CHECK(!r.direct_grid || (c.chan != 0 && c.batch == 1 && c.dim == 2 && w.nf[0] <= kDftMaxNf && w.nf[1] <= kDftMaxNf && c.nm[0] <= 64 && c.nm[1] <= 64));
    CHECK(!r.use_image || (r.use_pair && r.direct_grid && r.pair_bytes <= (size_t)kPairFillTrips * kInterpThreads * 16));
    CHECK(!r.use_pair || (r.use_halo && c.dim == 2 && r.lds_bytes == r.pair_bytes));
    CHECK(!r.use_halo || !r.cplx);
    CHECK((r.grid == GridSource::image) == r.use_image && (r.grid == GridSource::direct) == (r.direct_grid && !r.use_image));
    CHECK(r.grid != GridSource::image || r.gather == Gather::pair);
    check_crop(c.dim, r.nc, w.nf, r.grid == GridSource::pruned);
    CHECK(r.fine_bytes >= (size_t)c.batch * cells * 16 && (!r.use_image || r.fine_bytes >= r.pair_bytes));
    CHECK(r.use_lds == (r.lds_bytes <= (size_t)c.max_lds));
    if (r.gather == Gather::tiles) {
        CHECK(!r.use_lds && c.N >= 32768);
        check_tile(r.tile, c.dim, w.nf, w.p.w, r.cplx ? 2 : 1, c.max_lds, false);
    } else {
        CHECK((r.gather == Gather::pair) == r.use_pair && (r.gather == Gather::halo) == (r.use_halo && !r.use_pair));
        CHECK((r.gather == Gather::l2) == !r.use_lds && r.nwg >= 1);
        CHECK(!r.class_order || (r.gather == Gather::halo && c.dim >= 2 && c.N >= (int64_t)kOrderWindow * 64));
    }
}

static uint64_t g_digest = 1469598103934665603ull;      // FNV-1a over every field of every plan
static void digest(uint64_t v) {
    for (int i = 0; i < 8; ++i) {
        g_digest ^= (v >> (8 * i)) & 0xff;
        g_digest *= 1099511628211ull;
    }
}
static void digest_tile(const TileGeom& t) {
    for (int a = 0; a < 3; ++a) {
        digest((uint64_t)t.nt[a]);
        digest((uint64_t)t.T[a]);
    }
}

static std::string describe(const Case& c) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s d=%d box %lld x %lld x %lld tol %.0e N %lld chan/real %d batch %d layout %d num_cu %d max_lds %d",
                  c.type2 ? "t2" : "t1", c.dim, (long long)c.nm[0], (long long)c.nm[1], (long long)c.nm[2], c.tol, c.N, c.chan, c.batch, c.layout,
                  c.num_cu, c.max_lds);
    return buf;
}

// 1-D to 3-D boxes of these mode counts x tolerances x point counts x channels x LDS sizes x CU counts, one request of the box
// itself; 2-D plans on a point layout (span 1.2 x 1.03 periods, unforced band rule), dense by the library's rule (N = 4e6 in 2-D);
// type 2: complex and real outputs, one row and two.
static int sweep() {
    const int64_t counts[] = {1, 2, 12, 23, 45, 70, 129, 300};
    const double tols[] = {1e-4, 1e-7, 1e-12};
    const long long Ns[] = {0, 1, 3000, 32767, 32768, 65536, 262144, 4000000};
    long long plans = 0, spreaders[7] = {}, afters[5] = {}, grids[4] = {}, gathers[5] = {};
    for (int dim = 1; dim <= 3; ++dim)
        for (int64_t n0 : counts)
            for (int64_t n1 : counts)
                for (int64_t n2 : counts) {
                    if ((dim < 2 && n1 != 1) || (dim < 3 && n2 != 1)) continue;
                    for (double tol : tols)
                        for (long long N : Ns)
                            for (int chan : {1, 2})
                                for (int max_lds : {65536, 163840})
                                    for (int num_cu : {64, 256}) {
                                        Case c;
                                        c.dim = dim;
                                        c.nm[0] = n0;
                                        c.nm[1] = n1;
                                        c.nm[2] = n2;
                                        c.tol = tol;
                                        c.N = N;
                                        c.chan = chan;
                                        c.layout = dim == 2 ? -1 : 0;
                                        c.span[0] = 1.2;
                                        c.span[1] = c.span[2] = 1.0 + 2.0 / 70;
                                        c.num_cu = num_cu;
                                        c.max_lds = max_lds;
                                        g_at = describe(c);
                                        Planned pl = plan_case(c);
                                        check_type1(c, pl);
                                        const Type1Plan& p = pl.t1;
                                        ++plans;
                                        ++spreaders[(int)p.spreader];
                                        ++afters[(int)p.after];
                                        for (uint64_t v : {(uint64_t)pl.w->nf[0], (uint64_t)pl.w->nf[1], (uint64_t)pl.w->nf[2], (uint64_t)pl.w->p.w,
                                                           (uint64_t)pl.w->p.degree, (uint64_t)p.spreader, (uint64_t)p.after, (uint64_t)p.use_lds,
                                                           (uint64_t)p.lds_bytes, (uint64_t)p.nwg, (uint64_t)p.nslab, (uint64_t)p.per, (uint64_t)p.pad_bytes,
                                                           (uint64_t)p.class_order, (uint64_t)p.sum_bits, (uint64_t)p.sum_points, (uint64_t)p.level.nbands,
                                                           (uint64_t)p.level.band_cells, (uint64_t)p.nc[0], (uint64_t)p.nc[1], (uint64_t)p.nc[2],
                                                           (uint64_t)p.work_cells, (uint64_t)p.g2m_h[0], (uint64_t)p.g2m_h[1], (uint64_t)p.g2m_two_launch,
                                                           (uint64_t)p.g2m_split})
                                            digest(v);
                                        if (p.spreader == Spreader::tiles || p.spreader == Spreader::cells) digest_tile(p.tile);
                                        c.type2 = true;
                                        c.chan = chan == 1;           // one channel: real outputs
                                        for (int batch : {1, 2}) {
                                            c.batch = batch;
                                            g_at = describe(c);
                                            pl = plan_case(c);
                                            check_type2(c, pl);
                                            const Type2Plan& r = pl.t2;
                                            ++plans;
                                            ++grids[(int)r.grid];
                                            ++gathers[(int)r.gather];
                                            for (uint64_t v : {(uint64_t)r.grid, (uint64_t)r.gather, (uint64_t)r.cplx, (uint64_t)r.direct_grid, (uint64_t)r.use_halo,
                                                               (uint64_t)r.use_pair, (uint64_t)r.use_image, (uint64_t)r.lds_bytes, (uint64_t)r.pair_bytes,
                                                               (uint64_t)r.nc[0], (uint64_t)r.nc[1], (uint64_t)r.nc[2], (uint64_t)r.ccells, (uint64_t)r.region,
                                                               (uint64_t)r.use_lds, (uint64_t)r.nwg, (uint64_t)r.class_order, (uint64_t)r.fine_bytes})
                                                digest(v);
                                            if (r.gather == Gather::tiles) digest_tile(r.tile);
                                        }
                                    }
                }
    std::printf("sweep: %lld plans, digest %016llx\n", plans, (unsigned long long)g_digest);
    for (int i = 0; i < 7; ++i) std::printf("  spreader %s: %lld\n", kSpreaders[i], spreaders[i]);
    for (int i = 0; i < 5; ++i) std::printf("  after %s: %lld\n", kAfter[i], afters[i]);
    for (int i = 0; i < 4; ++i) std::printf("  grid %s: %lld\n", kGrids[i], grids[i]);
    for (int i = 0; i < 5; ++i) std::printf("  gather %s: %lld\n", kGathers[i], gathers[i]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--sweep") {
        sweep();
    } else {
        char kind[16];
        while (std::scanf("%15s", kind) == 1) {
            Case c;
            c.type2 = std::strcmp(kind, "t2") == 0;
            c.pair = std::strcmp(kind, "t1pair") == 0;
            g_at = kind;
            CHECK(c.type2 || c.pair || std::strcmp(kind, "t1") == 0);
            long long nm[6] = {1, 1, 1, 1, 1, 1};
            bool ok = !fails && std::scanf("%d %lld %lld %lld", &c.dim, &nm[0], &nm[1], &nm[2]) == 4;
            if (ok && c.pair) ok = std::scanf("%lld %lld %lld", &nm[3], &nm[4], &nm[5]) == 3;
            ok = ok && std::scanf("%lf %lld %d %d %d %d %d %lf %lf %lf %d %d", &c.tol, &c.N, &c.chan, &c.batch, &c.normal, &c.dense, &c.layout,
                                  &c.span[0], &c.span[1], &c.span[2], &c.num_cu, &c.max_lds) == 12;
            CHECK(ok);
            if (fails) break;
            for (int a = 0; a < 3; ++a) {
                c.nm[a] = nm[a];
                c.nmb[a] = nm[3 + a];
            }
            g_at = describe(c);
            CHECK(c.dim >= 1 && c.dim <= 3 && c.N >= 0 && c.batch >= 1 && c.tol > 0 && c.num_cu >= 1 && c.max_lds > 4608);
            for (int a = 0; a < 3; ++a) CHECK(c.nm[a] >= 1 && c.nmb[a] >= 1 && (a < c.dim || (c.nm[a] == 1 && c.nmb[a] == 1)));
            CHECK(c.type2 || c.chan == 1 || c.chan == 2);
            if (fails) break;
            const Planned pl = plan_case(c);
            if (c.type2) check_type2(c, pl);
            else check_type1(c, pl);
            print_case(c, pl);
        }
    }
    if (fails) std::fprintf(stderr, "%d checks FAILED\n", fails);
    return fails ? 1 : 0;
}
