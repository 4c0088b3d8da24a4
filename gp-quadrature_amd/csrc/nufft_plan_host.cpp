// Planning of the NUFFT passes on the host (see nufft_plan_host.hpp).  Pure arithmetic and environment hooks: no HIP runtime call,
// no device pointer is read.
#include "nufft_plan_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "line_fft.hpp"
#include "points_layout.hpp"
#include "spread_mfma.hpp"

namespace efgp {

static bool hook(const char* name) { return std::getenv(name) != nullptr; }

// ---- the in-house FFT's sizes (line_fft.hpp) ------------------------------------------------------------------------------------
bool fft_factorize(int64_t n, int* fac, int* nfac) {
    int k = 0;
    while (n % 4 == 0 && k < kFftMaxFactors) {
        fac[k++] = 4;
        n /= 4;
    }
    for (int r : {2, 3, 5})
        while (n % r == 0 && k < kFftMaxFactors) {
            fac[k++] = r;
            n /= r;
        }
    *nfac = k;
    return n == 1;
}

bool own_fft_supported(int rank, const int64_t* n) {
    static const bool off = std::getenv("EFGP_FFT_ROCFFT") != nullptr;        // test / comparison hook: every transform through hipFFT
    if (off || rank < 1 || rank > 3) return false;
    for (int a = 0; a < rank; ++a) {
        int fac[kFftMaxFactors], nf;
        if (n[a] < 1 || n[a] > kFftMaxLine || !fft_factorize(n[a], fac, &nf)) return false;
    }
    return true;
}

bool modes_to_grid_real_eligible(int nf0, int nf1, int nm0, int nm1) {
    return nf0 <= kDftMaxNf && nf1 <= kDftMaxNf && nm0 <= 64 && nm1 <= 64 && !hook("EFGP_NO_DIRECT_DFT");
}

// ---- window rule ----------------------------------------------------------------------------------------------------------------
// from 4e6 points on a 2-D plan takes the finer grid / narrower window (N = 1e7, mtot = 23: spread + gather 316 -> 276 us on
// the same box).  The accumulator -> modes step behind them grows with the grid: as ONE launch it went from 20 to 47-60 us
// (180 x 180 cells) and ate the gain -- the two-launch form (grid_rows_kernel + rows_modes_kernel) takes 12 / 17 us.
bool window_dense(int dim, int64_t npts) {
    const char* dense_env = std::getenv("EFGP_DENSE_POINTS");           // experiments: another threshold for the dense-sigma rule
    const int64_t dense_from = dense_env ? std::max<int64_t>(1, std::atoll(dense_env)) : kDensePoints;
    return dim == 2 && npts >= dense_from && !hook("EFGP_NO_DENSE_SIGMA");
}

void plan_window(int dim, const int64_t* n_modes, double tol, bool dense, WindowPlan* out) {
    out->dense = dense;
    double sigma_min = 1e30;
    for (int a = 0; a < 3; ++a) {
        out->nm[a] = a < dim ? n_modes[a] : 1;
        out->nf[a] = a < dim ? es_fine_size(n_modes[a], tol, dim, dense) : 1;
        if (a < dim) sigma_min = std::min(sigma_min, (double)out->nf[a] / (double)out->nm[a]);
    }
    es_make_params(tol, sigma_min, &out->p, dim);
}

// ---- tile geometry --------------------------------------------------------------------------------------------------------------
bool make_tile_geom(const NufftSite& s, const int64_t* nf, int W, int channels, size_t lds_budget, TileGeom* out, int force_tile) {
    TileGeom t;
    const int d = s.dim;
    t.d = d;
    t.W = W;
    // largest cubic-ish tile whose (T+W-1)^d * channels * 8 B fits the LDS budget
    const double cells_max = (double)lds_budget / (8.0 * channels);
    int ext = (int)std::floor(std::pow(cells_max, 1.0 / d));
    while (ext > W && std::pow((double)ext, d) > cells_max) --ext;
    int Tmax = ext - (W - 1);
    if (force_tile > 0) Tmax = force_tile;
    if (Tmax < 1 || (force_tile == 0 && Tmax < 2)) return false;
    t.nbins = 1;
    for (int a = 0; a < 3; ++a) {
        if (a < d) {
            t.nf[a] = (int)nf[a];
            t.nt[a] = (t.nf[a] + Tmax - 1) / Tmax;
            t.T[a] = (t.nf[a] + t.nt[a] - 1) / t.nt[a];
            t.ext[a] = t.T[a] + W - 1;
            t.scale[a] = s.h[a] * (double)nf[a];
            t.xcen[a] = s.xcen[a];
            t.nbins *= t.nt[a];
        } else {
            t.nf[a] = 1;
            t.nt[a] = 1;
            t.T[a] = 1;
            t.ext[a] = 1;
            t.scale[a] = 0.0;
            t.xcen[a] = 0.0;
        }
    }
    if (t.nbins > 16384) return false;          // LDS histograms of the binning kernels (2 x 64 KB)
    *out = t;
    return true;
}

bool tile_class_order_wanted(int dim, int64_t npts, const TileGeom& t) {
    return t.T[0] > 1 && dim >= 2 && npts >= (int64_t)kOrderWindow * 16 && !hook("EFGP_NO_CLASS_ORDER");
}

// ---- level of the point layout --------------------------------------------------------------------------------------------------
LevelWanted plan_level(const NufftSite& s, const int64_t* nf, int W) {
    LevelWanted none;
    none.nbands = 0;
    if (!s.has_layout || s.dim != 2 || W > kMfmaMaxW || s.npts < 32768 || hook("EFGP_NO_MFMA_SPREAD")) return none;
    const double scale[2] = {s.h[0] * (double)nf[0], s.h[1] * (double)nf[1]};
    double span[2], far = 0.0;
    for (int a = 0; a < 2; ++a) {
        span[a] = (s.hi[a] - s.lo[a]) * std::fabs(scale[a]);
        far = std::max(far, std::max(std::fabs(s.hi[a] - s.xcen[a]), std::fabs(s.lo[a] - s.xcen[a])) * std::fabs(scale[a]));
    }
    if (!(far < 1e9) || !(scale[0] > 0.0) || !(scale[1] > 0.0)) return none;      // cell indices are kept in 32-bit ints
    const char* force = std::getenv("EFGP_MFMA_BAND_CELLS");
    const int forced = force ? std::atoi(force) : 0;
    auto have_level = [&](int nbands) {
        for (int i = 0; i < s.nlevels; ++i)
            if (s.level_bands[i] == nbands) return true;
        return false;
    };
    LevelWanted want = none;
    for (int hb : {1, 8}) {
        if (forced && forced != hb) continue;
        int n = 1;
        while (span[1] / n > (double)hb - 1e-6 && n <= kMaxBands) n *= 2;
        if (n > kMaxBands) continue;
        const double per_run = (double)s.npts / ((double)n * std::max(1.0, span[0]));
        if (per_run < (forced ? 1.0 : (hb == 1 ? 192.0 : 24.0))) continue;
        want.nbands = n;
        want.band_cells = hb;
        if (hb == 8) {
            // A level costs a sort of the N points (2 ms at N = 1e6) and 28 B per point.  A gradient step makes two plans on one
            // model -- the Toeplitz box (4 m + 1 modes) and the probe box (mtot modes) on a grid half as fine -- whose coarsest
            // levels differ by a factor two: the probe plan takes the pair plan's level when it exists (bands 2-4 cells high instead
            // of 4-8: a few more run ends per band, no second sort; round 4: the layout-building step 4.3 -> 2.4 ms).
            bool have = have_level(n);
            for (int f = 2; !have && f <= 4; f *= 2) {
                const double per_run_f = (double)s.npts / ((double)(n * f) * std::max(1.0, span[0]));
                if (n * f > kMaxBands || per_run_f < 24.0) break;
                if (have_level(n * f)) {
                    want.nbands = n * f;
                    have = true;
                }
            }
        }
        break;
    }
    return want;
}

// Chunk length: every resident wave gets R chunks of at most ~1536 points (R rounds keep the tail of the grid-stride loop
// short); multiples of 64 (one point per lane per batch).  The spreader runs 8 waves per CU (band levels up to 8 cells high) or
// 12 (one-cell bands, dense point sets): from 4e6 points on the chunk count is sized for 24 waves per CU, a multiple of both
// (N = 1e7: 12 k chunks of 832 points = 4.0 / 5.9 rounds).  Smaller sets keep the 8-wave sizing: every chunk end is a tile
// flush (256 atomics), which must stay rare next to the points.
int chunk_length(int64_t npts, int num_cu) {
    const int64_t waves = (int64_t)num_cu * (npts >= 4000000 ? 24 : 8);
    const int64_t rounds = std::max<int64_t>(1, (npts + waves * 1536 - 1) / (waves * 1536));
    int64_t len = (npts + waves * rounds - 1) / (waves * rounds);
    len = (len + 63) / 64 * 64;
    return (int)std::max<int64_t>(64, len);
}

// ---- one type-1 pass ------------------------------------------------------------------------------------------------------------
static int64_t cells_of(const int64_t* nf) { return nf[0] * nf[1] * nf[2]; }

static bool g2m_eligible(const NufftSite& s, const int64_t* nf, const ModeBoxes* req) {
    if (!req || s.dim != 2 || hook("EFGP_NO_GRID_TO_MODES")) return false;
    if (nf[0] > kG2MMaxNf || nf[1] > kG2MMaxNf) return false;
    for (int a = 0; a < 2; ++a) {
        if (req->nma[a] / 2 > kG2MMaxH) return false;
        if (req->part == 4 && req->nmb[a] / 2 > kG2MMaxH) return false;
    }
    return true;
}

// the launch form of grid-to-modes
static void plan_g2m(const int64_t* nf, const ModeBoxes& req, int nbatch, Type1Plan* pl) {
    for (int a = 0; a < 2; ++a) pl->g2m_h[a] = (int)std::max(req.nma[a] / 2, req.part == 4 ? req.nmb[a] / 2 : (int64_t)0);
    pl->g2m_two_launch = !hook("EFGP_G2M_V1");       // round 3: rows of the accumulator over the chip, then one workgroup per column pair
    pl->g2m_split = 1;
    if (pl->g2m_two_launch) return;
    const unsigned tiles = (unsigned)(pl->g2m_h[0] / 2 + 1);
    const bool small = nf[0] <= 128 && nf[1] <= 128;
    // stage-1 split, measured (rocprofv3, launch average): 96 x 96 grid 20.0 / 27.7 / 32.4 / 45.7 us at 1 / 2 / 4 / 8 workgroups
    // per tile -- the shares' round trip through memory (two device-scope fences, an atomic) costs more than a quarter of stage 1
    // saves; 180 x 180 grid 59.8 / 51.2 / 47.5 / 56.2 us.
    int split = small ? 1 : 4;
    if (const char* e = std::getenv("EFGP_G2M_SPLIT")) split = std::max(1, std::min(16, std::atoi(e)));
    while (split > 1 && (int64_t)tiles * nbatch * split > 4096) split /= 2;
    if (split > 1 && (size_t)tiles * nbatch * sizeof(unsigned int) > 65536) split = 1;       // the tickets' 64 KB
    pl->g2m_split = split;
}

// What follows the spread (transform_fine): grid-to-modes when the grid is small, else the in-house pruned transform when the
// caller said which modes it wants -- every pass keeps only the bins of the (larger) mode box -- else the FFT in place.
// has_acc: the spreader left its sums in one int64 accumulator that the pruned transform's first pass can read itself.
static void plan_after_spread(const NufftSite& s, const int64_t* nf, const ModeBoxes* req, int nbatch, bool has_acc, bool g2m_reads_acc,
                              Type1Plan* pl) {
    if (g2m_eligible(s, nf, req)) {
        pl->after = g2m_reads_acc ? AfterSpread::g2m_from_acc : AfterSpread::g2m;
        plan_g2m(nf, *req, nbatch, pl);
        return;
    }
    pl->after = AfterSpread::fft;
    if (req && own_fft_supported(s.dim, nf) && !hook("EFGP_NO_PRUNED_FFT")) {
        int64_t wk = nbatch;
        bool smaller = false;
        for (int a = 0; a < s.dim; ++a) {
            int64_t hmax = req->nma[a] / 2;
            if (req->part == 4) hmax = std::max(hmax, req->nmb[a] / 2);
            pl->nc[a] = std::min<int64_t>(2 * hmax + 1, nf[a]);
            smaller = smaller || pl->nc[a] < nf[a];
            wk *= a == s.dim - 1 ? pl->nc[a] : nf[a];
        }
        if (smaller) {
            const bool fuse = has_acc && nf[s.dim - 1] > 1 && !hook("EFGP_NO_FFT_FROM_ACC");
            pl->after = fuse ? AfterSpread::pruned_from_acc : AfterSpread::pruned;
            pl->work_cells = wk;
        }
    }
}

// fine grids inside LDS: one slab per workgroup; grids beyond LDS with few points: global atomics on one slab.  Also the route of
// a plan without points.
static void plan_lds_or_global(const NufftSite& s, const int64_t* nf, const EsParams& p, int channels, bool normal, Type1Plan* pl) {
    const int64_t cells = cells_of(nf);
    const int64_t want = (s.npts + kSpreadThreads - 1) / kSpreadThreads;
    if (pl->use_lds) {
        const int per_cu = std::max(1, std::min(2, (int)((size_t)s.max_lds / std::max<size_t>(pl->lds_bytes, 1))));
        // LDS-atomic bound: spread the points over as many CUs as there are full 1024-point chunks (each workgroup also
        // pays a 147-KB zero + flush, ~5 us, so not below one point per thread)
        pl->nwg = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)s.num_cu * per_cu, want));
    } else {
        pl->nwg = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)s.num_cu * 8, want));
    }
    pl->nslab = pl->use_lds ? pl->nwg : 1;
    pl->per = (s.npts + pl->nwg - 1) / std::max(pl->nwg, 1);
    // padded-row variant when the padded grid still fits LDS; 48-bit raw accumulation when its rounding
    // floor (points per workgroup * 2^-47 relative to max|c|) stays two orders below the requested tolerance
    const int64_t nlast = nf[s.dim - 1];
    pl->pad_bytes = (size_t)channels * (size_t)(cells / nlast) * (size_t)(nlast + p.w - 1) * sizeof(double);
    const bool use_pad = pl->use_lds && pl->pad_bytes + 4608 <= (size_t)s.max_lds && !hook("EFGP_NO_PAD");   // + class lists
    const bool raw48 = use_pad && (double)pl->per * std::ldexp(1.0, -47) <= 0.01 * s.tol && !hook("EFGP_NO_RAW48") &&
                       !normal;     // normals: max|c| is 8.6 typical magnitudes, the raw floor would be that much coarser
    pl->spreader = raw48 ? Spreader::lds_pad_raw48 : use_pad ? Spreader::lds_pad_61 : pl->use_lds ? Spreader::lds_plain : Spreader::global;
    // raw48: every workgroup's sums stay below 2^46 and reduce_slabs_kernel adds at most 512 of them in int64.
    // Otherwise the bound must hold for the SUM OVER ALL SLABS (reduce_slabs_kernel adds them in plain int64):
    // bounding only one workgroup's share let same-sign strengths (the all-ones channel, clustered points) wrap
    // the total, e.g. 1-D, N = 1e6, tol <= 1e-9: 512 slabs x 2^61 / 1954 points each.
    pl->sum_bits = raw48 ? 46 : 61;
    pl->sum_points = raw48 ? pl->per : s.npts;
    // per-plan bank-balanced order (d >= 2, enough points for the one-off pass to pay)
    pl->class_order = use_pad && s.dim >= 2 && s.npts >= (int64_t)kOrderWindow * 64 && !hook("EFGP_NO_CLASS_ORDER");
}

Type1Plan plan_type1(const NufftSite& s, const int64_t* nf, const EsParams& p, int channels, bool normal, int nbatch, const ModeBoxes* req,
                     bool allow_layout) {
    Type1Plan pl;
    const int64_t cells = cells_of(nf);
    pl.lds_bytes = (size_t)channels * (size_t)cells * sizeof(double);
    pl.use_lds = pl.lds_bytes <= (size_t)s.max_lds && s.npts > 0;
    const size_t tile_budget = (size_t)s.max_lds - 4096;
    if (allow_layout) pl.level = plan_level(s, nf, p.w);
    else pl.level.nbands = 0;
    // 2-D with many points per fine-grid cell: register accumulation over base-cell-sorted points.
    // Opt-in (EFGP_CELLSORT=1): the kernel itself is 1.2-1.7x faster than the LDS-atomic spreader at >= 250 points
    // per cell, but the per-plan counting sort it needs (0.15 ms at N=1e6, 0.6 ms at N=1e7) only pays off after
    // several passes over the same plan; see LABNOTES.md section 4.1.
    const char* cellsort = std::getenv("EFGP_CELLSORT");
    if (pl.level.nbands) {
        // the global int64 grid sums over ALL points: the scale is bounded with N
        pl.spreader = Spreader::layout;
        pl.sum_bits = 61;
        pl.sum_points = s.npts;
        plan_after_spread(s, nf, req, nbatch, true, true, &pl);
    } else if (cellsort && cellsort[0] == '1' && !normal && s.dim == 2 && p.w <= kCellMaxW && p.degree <= p.w + 4 && cells <= 16384 &&
               s.npts > 0 && make_tile_geom(s, nf, p.w, channels, tile_budget, &pl.tile, 1)) {
        pl.spreader = Spreader::cells;
        plan_after_spread(s, nf, req, nbatch, false, false, &pl);
    } else if (!pl.use_lds && s.npts >= 32768 && !hook("EFGP_NO_TILES") && make_tile_geom(s, nf, p.w, channels, tile_budget, &pl.tile)) {
        // grids beyond LDS with many points (else global atomics): bound the scale with N instead of points per workgroup
        pl.spreader = Spreader::tiles;
        pl.sum_bits = 61;
        pl.sum_points = s.npts;
        plan_after_spread(s, nf, req, nbatch, true, false, &pl);
    } else {
        plan_lds_or_global(s, nf, p, channels, normal, &pl);
        plan_after_spread(s, nf, req, nbatch, false, false, &pl);
    }
    return pl;
}

// ---- one type-2 call ------------------------------------------------------------------------------------------------------------
Type2Plan plan_type2(const NufftSite& s, const int64_t* nf, const EsParams& p, const int64_t* n_modes, int nbatch, bool real_only) {
    Type2Plan r;
    const size_t max_lds = (size_t)s.max_lds;
    const int64_t cells = cells_of(nf);
    r.direct_grid = real_only && nbatch == 1 && s.dim == 2 && modes_to_grid_real_eligible((int)nf[0], (int)nf[1], (int)n_modes[0], (int)n_modes[1]);
    r.cplx = !real_only;
    r.lds_bytes = (size_t)cells * (r.cplx ? 2 * sizeof(double) : sizeof(double));
    size_t halo_cells = 1;
    for (int a = 0; a < s.dim; ++a) halo_cells *= (size_t)(nf[a] + p.w - 1);
    r.use_halo = !r.cplx && halo_cells * sizeof(double) <= max_lds && !hook("EFGP_NO_HALO");
    if (r.use_halo) r.lds_bytes = halo_cells * sizeof(double);
    r.pair_bytes = s.dim == 2 ? interp_pair_lds_bytes((int)nf[0], (int)nf[1], p.w) : 0;
    r.use_pair = r.use_halo && s.dim == 2 && r.pair_bytes <= max_lds && !hook("EFGP_NO_PAIR_GATHER");
    if (r.use_pair) r.lds_bytes = r.pair_bytes;
    r.use_image = r.direct_grid && r.use_pair && r.pair_bytes <= (size_t)kPairFillTrips * kInterpThreads * 2 * sizeof(double) &&
                  !hook("EFGP_NO_GATHER_IMAGE");
    const size_t fine_bytes = (size_t)nbatch * (size_t)cells * 2 * sizeof(double);
    r.fine_bytes = r.use_image ? std::max(fine_bytes, r.pair_bytes) : fine_bytes;

    // the fine grid from the modes: one dense-DFT launch (with or without the gather's image), else corrected modes + the in-house
    // pruned transform -- the corrected modes go to a compact array (the 2 (nm/2) + 1 lowest bins per axis), the passes expand it
    // axis by axis, slowest first -- else corrected modes on the full grid + the FFT in place
    r.region = nbatch;
    bool smaller = false;
    for (int a = 0; a < s.dim; ++a) {
        r.nc[a] = std::min<int64_t>(2 * (n_modes[a] / 2) + 1, nf[a]);
        smaller = smaller || r.nc[a] < nf[a];
        r.ccells *= r.nc[a];
        r.region *= a == s.dim - 1 ? r.nc[a] : nf[a];
    }
    if (r.direct_grid) r.grid = r.use_image ? GridSource::image : GridSource::direct;
    else r.grid = smaller && own_fft_supported(s.dim, nf) && !hook("EFGP_NO_PRUNED_FFT") ? GridSource::pruned : GridSource::fft;

    // the fine grid to the points: tiles when the grid is beyond LDS and the points are many; else the pair, the halo or the plain
    // gather, from LDS when the grid fits and through L2 when not
    r.use_lds = r.lds_bytes <= max_lds;
    if (!r.use_lds && s.npts >= 32768 && !hook("EFGP_NO_TILES") && make_tile_geom(s, nf, p.w, r.cplx ? 2 : 1, max_lds - 4096, &r.tile)) {
        r.gather = Gather::tiles;
        return r;
    }
    r.gather = r.use_pair ? Gather::pair : r.use_halo ? Gather::halo : r.use_lds ? Gather::lds : Gather::l2;
    const int thr = r.use_lds ? kInterpThreads : kInterpThreadsGlobal;
    const int64_t want = (s.npts + thr - 1) / thr;
    if (r.use_lds) {
        const int per_cu = std::max(1, std::min(4, (int)(max_lds / std::max<size_t>(r.lds_bytes, 1))));
        // each workgroup pays one fine-grid copy into LDS: keep >= 2 points per thread
        const int64_t cap = std::max<int64_t>(1, s.npts / (2 * kInterpThreads));
        r.nwg = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((int64_t)s.num_cu * per_cu, want), cap));
    } else {
        r.nwg = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)s.num_cu * 8, want));
    }
    r.class_order = r.use_halo && !r.use_pair && s.dim >= 2 && s.npts >= (int64_t)kOrderWindow * 64 && !hook("EFGP_NO_CLASS_ORDER");
    return r;
}

}  // namespace efgp
