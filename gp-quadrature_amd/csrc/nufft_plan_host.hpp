// Host-side planning of the NUFFT passes (nufft_plan_host.cpp): the window rule, the tile geometry, the level of the point layout a
// pass wants, the route of one type-1 pass and of one type-2 call.  Plain numbers in, plain numbers out: no HIP runtime call, no
// device pointer, no DeviceCtx -- tools/nufft_plan_check.cpp links it without a device and tests/test_nufft_plan_host.py holds it to
// tests/_nufft_routes.py.  The drivers of nufft.hip execute these plans.  The constants the planner shares with the kernels live
// here (or in the header that already had them: kSpreadThreads, kInterpThreads, kMfmaMaxW, kMaxBands, kFftMaxLine).
// Every hook is read per call.
#pragma once
#include <cstddef>
#include <cstdint>

#include "es_kernel.hpp"
#include "nufft_dev.hpp"

namespace efgp {

constexpr int64_t kDensePoints = 4000000;    // a 2-D plan from this many points on takes the finer grid / narrower window
constexpr int kOrderWindow = 4096;           // points per window of the bank-balanced processing orders (class_order_kernel)
constexpr int kCellMaxW = 8;                 // cell-sorted spreader: RH^2 accumulators per channel + RH (DEG+1) coefficients in registers
constexpr int kG2MMaxNf = 256;               // grid-to-modes kernels: cells per axis of the fine grid
constexpr int kG2MMaxH = 32;                 // ... and modes k in [-32, 32] per axis
constexpr int kG2RRows = 4;                  // rows of the accumulator per workgroup of grid_rows_kernel
constexpr int kDftMaxNf = 128;               // modes_to_grid_real_kernel (small_dft.hip): cells per axis
// LDS fill of interp_real2_pair_kernel from its image: trips of 16 bytes per thread that cover the 160 KB of a CU
constexpr int kPairFillTrips = (160 * 1024 / 16 + kInterpThreads - 1) / kInterpThreads;
constexpr int kMaxLevels = 16;               // levels of a point layout: one per power-of-two band count up to kMaxBands

// Rows and even row pitch of one parity copy of interp_real2_pair_kernel, and the bytes of the two copies: the size of its
// LDS and of the image that modes_to_grid_real_kernel writes for it.
inline int interp_pair_rows(int nf0, int W) { return nf0 + W - 1; }
inline int interp_pair_pitch(int nf1, int W) { return (nf1 + 2 * ((W + 1) / 2) + 1) & ~1; }
inline size_t interp_pair_lds_bytes(int nf0, int nf1, int W) {
    return 2 * (size_t)interp_pair_rows(nf0, W) * (size_t)interp_pair_pitch(nf1, W) * sizeof(double);
}

struct TileGeom {      // tiles of the fine grid (spread_tile_kernel, interp_tile_kernel; single cells: spread_cell_kernel)
    int d;
    int nf[3];
    int T[3];        // tile size in cells
    int nt[3];       // tiles per dimension
    int ext[3];      // T + W - 1: cells an LDS tile spans per dimension (1 for unused dims)
    int nbins;
    int W;
    double scale[3];
    double xcen[3];
};

// A plan and its device as the planner sees them.
struct NufftSite {
    int dim = 0;
    int64_t npts = 0;
    double tol = 0.0;
    double h[3] = {0, 0, 0}, xcen[3] = {0, 0, 0};
    int num_cu = 0, max_lds = 0;
    // the model's point layout, when the plan was made on one: extent of the points and the band counts of the levels it holds
    bool has_layout = false;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    int nlevels = 0;
    int level_bands[kMaxLevels] = {};
};

// ---- window rule: what get_window decides before it looks into its cache, and what it designs on a miss -----------------------
// dense: a 2-D plan over kDensePoints points or more (EFGP_DENSE_POINTS: another threshold; EFGP_NO_DENSE_SIGMA: never)
bool window_dense(int dim, int64_t npts);
struct WindowPlan {
    bool dense = false;
    int64_t nm[3] = {1, 1, 1}, nf[3] = {1, 1, 1};     // fine grid = next 2^a 3^b 5^c size >= 2 n_modes (>= 32) per axis
    EsParams p;                                        // from the smallest upsampling ratio nf / nm
};
void plan_window(int dim, const int64_t* n_modes, double tol, bool dense, WindowPlan* out);

// ---- tile geometry: the largest cubic-ish tile whose (T + W - 1)^d * channels * 8 B fit lds_budget ----------------------------
// force_tile > 0: use that tile size (1 = bins are single cells, for the cell-sorted spreader).  False: no such geometry.
bool make_tile_geom(const NufftSite& s, const int64_t* nf, int W, int channels, size_t lds_budget, TileGeom* out, int force_tile = 0);
// the bank-balanced order inside the tiles (tile_class_order_kernel) repays its pass over the sorted points: tiles proper (the
// single-cell bins of the cell-sorted spreader have one class), d >= 2, 16 windows of points or more, no EFGP_NO_CLASS_ORDER
bool tile_class_order_wanted(int dim, int64_t npts, const TileGeom& t);

// ---- level of the point layout the MFMA spreader wants for this fine grid ------------------------------------------------------
// nbands = 0: none (no layout, not 2-D, window wider than the register tile, cell indices beyond 32 bits, too few points per run to
// amortise the tile flushes, EFGP_NO_MFMA_SPREAD).  band_cells = bound on the height of the level's bands in fine cells: 1 for dense
// point sets (>= 192 points per run at one-cell bands: the spreader then needs W + 1 tile columns, fits three waves per SIMD and
// stores seven zeros less per point), else 8 (>= 24 points per run; the tile's 16 columns hold the 8-cell stencil at offsets 0..8).
// EFGP_MFMA_BAND_CELLS = 1 | 8 forces one (from one point per run on).
struct LevelWanted {
    int nbands = 0;
    int band_cells = 8;
};
LevelWanted plan_level(const NufftSite& s, const int64_t* nf, int W);

// chunk length of a level of the point layout (points_layout.hip cuts every band into chunks of at most this many sorted points)
int chunk_length(int64_t npts, int num_cu);

// ---- one type-1 pass ------------------------------------------------------------------------------------------------------------
// The mode boxes the caller wants from the transformed grid (G2MRequest without its pointers): part = 0 | 3 | 4 as in G2MArgs,
// nmb only for part == 4.
struct ModeBoxes {
    int part = 0;
    int64_t nma[3] = {1, 1, 1}, nmb[3] = {1, 1, 1};
};
// The route tests run in this order; the first whose predicate holds takes the pass.
enum class Spreader { layout, cells, tiles, lds_pad_raw48, lds_pad_61, lds_plain, global };
enum class AfterSpread {
    g2m_from_acc,       // grid-to-modes straight from the layout route's int64 accumulator
    g2m,                // ... from the reduced complex grid
    pruned_from_acc,    // pruned transform whose first pass reads (and clears) the int64 accumulator
    pruned,             // pruned transform of the converted grid
    fft                 // full FFT in place
};
struct Type1Plan {
    Spreader spreader = Spreader::global;
    AfterSpread after = AfterSpread::fft;
    LevelWanted level;           // layout
    TileGeom tile{};             // tiles, cells (single-cell bins)
    // LDS slabs / global atomics
    bool use_lds = false;        // the fine grid of all channels fits LDS and there are points
    size_t lds_bytes = 0;
    int nwg = 1, nslab = 1;
    int64_t per = 0;             // points per workgroup
    size_t pad_bytes = 0;        // LDS of the padded-row spreader
    bool class_order = false;    // the plan's bank-balanced processing order is wanted
    // fixed-point scale: the integer sums take sum_bits bits and add up the strengths of at most sum_points points (0 bits: the
    // route adds doubles)
    int sum_bits = 0;
    int64_t sum_points = 0;
    // what follows: crop extents and work cells of the pruned transform; half-widths and form of grid-to-modes
    int64_t nc[3] = {1, 1, 1}, work_cells = 0;
    int g2m_h[2] = {0, 0};
    bool g2m_two_launch = true;  // grid_rows_kernel + rows_modes_kernel; false (EFGP_G2M_V1): grid_to_modes_kernel with g2m_split
    int g2m_split = 1;
};
// channels: real channels per fine grid; normal: generated normal strengths; req: null when the caller extracts the modes itself
// from the full grid; allow_layout = false: the plan of a pass whose layout level could not be made.
Type1Plan plan_type1(const NufftSite& s, const int64_t* nf, const EsParams& p, int channels, bool normal, int nbatch, const ModeBoxes* req,
                     bool allow_layout = true);

// ---- one type-2 call ------------------------------------------------------------------------------------------------------------
enum class GridSource {
    image,      // one dense-DFT launch that writes the pair gather's LDS image
    direct,     // one dense-DFT launch that writes the real fine grid
    pruned,     // corrected modes + the in-house pruned transform
    fft         // corrected modes on the full grid + the FFT in place
};
enum class Gather { tiles, pair, halo, lds, l2 };
struct Type2Plan {
    // how the gather will hold the fine grid in LDS: decided before the grid is filled, the grid kernel may write the gather's image
    bool cplx = false;
    bool direct_grid = false;    // small 2-D real-output transforms: the real fine grid by ONE dense-DFT launch instead of precorrect + two FFT kernels
    bool use_halo = false;       // real outputs: halo-padded LDS copy when it fits (no wrap arithmetic in the gather)
    bool use_pair = false;       // 2-D real outputs whose two parity copies fit LDS: aligned 16-byte reads, no processing order
    bool use_image = false;      // ... and the grid kernel writes those two copies itself, laid out as the gather holds them: the fill is a flat copy
    size_t lds_bytes = 0, pair_bytes = 0;
    GridSource grid = GridSource::fft;
    int64_t nc[3] = {1, 1, 1}, ccells = 1, region = 0;      // pruned: kept bins per axis, their product, cells of the work region
    Gather gather = Gather::l2;
    TileGeom tile{};             // tiles
    bool use_lds = false;
    int nwg = 1;
    bool class_order = false;
    size_t fine_bytes = 0;       // what to ask SLOT_FINE for
};
Type2Plan plan_type2(const NufftSite& s, const int64_t* nf, const EsParams& p, const int64_t* n_modes, int nbatch, bool real_only);

// small_dft.hip's dense DFT takes this grid and mode box (EFGP_NO_DIRECT_DFT: never)
bool modes_to_grid_real_eligible(int nf0, int nf1, int nm0, int nm1);

}  // namespace efgp
