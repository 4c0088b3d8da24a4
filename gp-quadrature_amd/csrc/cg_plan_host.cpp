// Planning of the Toeplitz operator and of the CG launches on the host (see cg_plan_host.hpp).  Pure arithmetic and environment
// hooks: no HIP runtime call, no device pointer is read.
#include "cg_plan_host.hpp"

#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "es_kernel.hpp"

namespace efgp {

static bool hook(const char* name) { return std::getenv(name) != nullptr; }

bool pow2_axes_within(int dim, const int64_t* F, int64_t lo, int64_t hi) {
    for (int a = 0; a < dim; ++a)
        if (F[a] < lo || F[a] > hi || (F[a] & (F[a] - 1)) != 0) return false;
    return true;
}

ToepGeom lag_geometry(const ToepGeom& g, const int64_t* Ls) {
    ToepGeom gv = g;
    gv.M = 1;
    for (int a = 0; a < 3; ++a) {
        gv.n[a] = Ls[a];
        gv.M *= gv.n[a];
    }
    return gv;
}

bool persistent_cg_eligible(const ToepGeom& tg) {
    int64_t padded = 1;
    for (int a = 0; a < tg.d; ++a) {
        if (tg.F[a] & (tg.F[a] - 1)) return false;
        if (tg.F[a] > 4096) return false;
    }
    // padded leading dimension on the fastest axis when d > 1
    for (int a = 0; a < tg.d; ++a) padded *= (a == tg.d - 1 && tg.d > 1) ? tg.F[a] + 1 : tg.F[a];
    if (padded > pcg::kMaxGrid) return false;
    if (tg.M > (int64_t)pcg::kSlots * pcg::kThreads) return false;
    return true;
}

bool toeplitz_vhat_fused_eligible(const ToepGeom& g) { return g.d == 2 && g.F[0] == 64 && g.F[1] == 64 && !hook("EFGP_NO_VHAT64"); }

bool toeplitz_apply_fused_eligible(const ToepGeom& g) {
    return g.d == 2 && g.F[0] == 64 && g.F[1] == 64 && g.n[0] == g.n[1] && g.n[0] <= 32 && g.M <= 2 * pcg::kThreads &&
           !hook("EFGP_NO_APPLY64");
}

OperatorPlan plan_operator(int dim, const int64_t* Ls, int force_pow2, int flags) {
    OperatorPlan pl;
    ToepGeom& g = pl.g;
    g.d = dim;
    g.M = 1;
    g.Ftot = 1;
    for (int a = 0; a < 3; ++a) {
        pl.Ls[a] = a < dim ? Ls[a] : 1;
        g.n[a] = a < dim ? (Ls[a] + 1) / 2 : 1;                       // efgpnd.py:1259
        g.F[a] = a < dim ? (force_pow2 ? next_pow2(Ls[a]) : next_smooth_even(Ls[a])) : 1;   // :1269
        g.M *= g.n[a];
        g.Ftot *= g.F[a];
    }
    const bool eligible = pl.eligible = persistent_cg_eligible(g);
    const bool square = dim == 2 && g.n[0] == g.n[1] && g.F[0] == g.F[1];
    // Hermitian solves of blocks up to 23 x 23 run on the 48 x 48 circulant grid: its spectrum rides in the launch that makes the
    // 64 x 64 one (this grid's, or the embedding's)
    pl.want48 = square && (g.n[0] & 1) && g.n[0] <= 23 && g.F[0] <= 64 && eligible && !hook("EFGP_NO_CG48") && !hook("EFGP_NO_CG64") &&
                !hook("EFGP_NO_CG_HERM");
    // deferred: the launch that would make the 64 x 64 and 48 x 48 spectra together is left to the fused mean solve and to first use
    pl.defer_pair = (flags & EFGP_TOEPLITZ_DEFER_SPECTRA) && pl.want48 && !hook("EFGP_NO_DEFER_SPECTRA");
    pl.vhat_fused = toeplitz_vhat_fused_eligible(g);
    pl.lines_ok = dim == 2 && pow2_axes_within(dim, g.F, 128, 512);
    pl.lines3_ok = dim == 3 && pow2_axes_within(dim, g.F, 64, 256);
    // 2-D grids of the cooperative solve (128..512 per axis): when a smaller cooperative grid exists nothing on the fit path reads
    // the reference grid's spectrum -- keep a copy of v and make it on first use
    pl.defer_ref = pl.lines_ok && !hook("EFGP_NO_COOP_SMALL") && !hook("EFGP_EAGER_REF_SPECTRUM");
    // the cooperative solve runs on the smallest grid of the in-wave transforms (64 R or 48 R) that holds 2 n - 1
    if (pl.lines_ok && !hook("EFGP_NO_COOP_SMALL")) {
        static const int64_t ladder[] = {96, 128, 192, 256, 384, 512};
        pl.g_co = g;
        pl.g_co.Ftot = 1;
        for (int a = 0; a < 2; ++a) {
            for (int64_t c : ladder)
                if (c >= pl.Ls[a]) {
                    pl.g_co.F[a] = c;
                    break;
                }
            pl.coop_small = pl.coop_small || pl.g_co.F[a] < g.F[a];
            pl.g_co.Ftot *= pl.g_co.F[a];
        }
    }
    // 2-D blocks of up to 32 x 32 modes on grids below 64 x 64: the single-launch solves run on a 64 x 64 embedding
    pl.embed64 = square && eligible && g.F[0] < 64 && pl.Ls[0] <= 63 && !hook("EFGP_NO_CG64_EMBED") && !hook("EFGP_NO_CG64");
    if (pl.embed64) {
        pl.g_cg = g;
        pl.g_cg.F[0] = pl.g_cg.F[1] = 64;
        pl.g_cg.Ftot = kCells64;
    }
    pl.h48 = pl.want48 && (pl.vhat_fused || pl.embed64);
    // a single mode on a grid of one cell (and no 64 x 64 embedding): the single-launch kernels have no transform stage to run
    // there (persistent_cg_launch); the multi-launch solver skips axes of extent 1 in its transforms and solves the scalar system
    pl.persistent_ok = eligible && !(g.Ftot == 1 && !pl.embed64);
    pl.vhat_bytes = spectrum_bytes(g);
    pl.v_keep_bytes = (size_t)lag_geometry(g, pl.Ls).M * sizeof(double2);
    pl.vhat_co_bytes = pl.coop_small ? spectrum_bytes(pl.g_co) : 0;
    return pl;
}

void cg_solve_shape(const ToepGeom& g, bool persistent_ok, bool h48, bool cg64, const ToepGeom* g_co, int hermitian, int64_t* shape_out) {
    for (int a = 0; a < g.d; ++a) shape_out[a] = g.F[a];
    if (g.d == 2 && persistent_ok) {
        if (hermitian && h48 && !hook("EFGP_NO_CG48")) shape_out[0] = shape_out[1] = 48;
        else if (cg64) shape_out[0] = shape_out[1] = 64;
    } else if (g_co && !hook("EFGP_NO_COOP_SMALL") && !hook("EFGP_NO_CG_COOP")) {
        for (int a = 0; a < 2; ++a) shape_out[a] = g_co->F[a];
    }
}

// Few systems: G = 32-64 workgroups per system (latency); many systems (variance / trace probes): as few workgroups per system as
// the registers allow, G = 1 when the mode block has <= 2048 entries -- no grid barrier, one system per CU (throughput).
CoopShape coop_shape(const ToepGeom& g, int nbatch, bool hermitian, int num_cu, int max_lds) {
    const int F0 = (int)g.F[0], F1 = (int)g.F[1], n0 = (int)g.n[0], n1 = (int)g.n[1];
    // Hermitian systems (the caller's promise, checked by the kernel): rows k0 >= 0 only, column pairs (cg_coop2d_herm_kernel)
    const bool herm = hermitian && (n0 & 1) && (n1 & 1) && n0 >= 3 && std::getenv("EFGP_NO_CG_COOP_HERM") == nullptr;
    const int nrow = herm ? (n0 + 1) / 2 : n0;            // rows of the mode block the workgroups share out
    const int ncol = herm ? F1 / 2 : F1;                  // column lines (pairs) they share out
    // workgroups per system: as many as the latency shape uses (16 / 32 / 64) while the whole batch stays resident (one
    // workgroup per CU), never fewer than the registers need (8 vector entries per thread)
    int G_lat = F1 / 8;      // 16 / 32 / 64 (measured at 128^2: 19.9 us per iteration with 16 workgroups, 22.7 with 32, 20.6 with 8)
    if (herm && F1 <= 256) G_lat = F1 / 16;   // half the work per system: 8 / 16 workgroups measured best at 128^2 / 256^2, 64 at 512^2
    if (const char* ed = std::getenv("EFGP_COOP_GDIV")) G_lat = std::max(1, F1 / std::max(1, std::atoi(ed)));  // experiments: G = F1 / div
    if (const char* eg = std::getenv("EFGP_COOP_G")) G_lat = std::max(1, std::min(G_lat, std::atoi(eg)));   // experiments
    // the workgroup counts a grid offers: G_lat halved while it stays whole (16 8 4 2 1; 12 6 3 1 on the 48 R grids)
    auto halve = [](int Gv) { return Gv > 1 ? ((Gv & 1) ? 1 : Gv / 2) : 1; };
    int G_min = G_lat;       // the smallest count whose rows still fit a workgroup's registers (8 vector entries per thread)
    while (G_min > 1 && ((nrow + halve(G_min) - 1) / halve(G_min)) * n1 <= 8 * kLineThreads) G_min = halve(G_min);
    if (const char* eg = std::getenv("EFGP_COOP_GMIN")) {                                                       // experiments
        int Gv = G_lat;
        while (Gv > G_min && halve(Gv) >= std::atoi(eg)) Gv = halve(Gv);
        G_min = std::max(G_min, Gv);
    }
    int G = G_lat;
    while (G > G_min && (int64_t)G * nbatch > num_cu) G = halve(G);
    const int ks = ((nrow + G - 1) / G) * n1 <= 4 * kLineThreads ? 4 : 8;
    // columns per LDS pass: as many as the workgroup owns, the per-thread load registers (16) and the LDS allow -- a pass of
    // 8 columns leaves one work item per thread and stage (latency bound: 134 us per iteration of a 128^2 system on one CU
    // with 8, 4 items with 32).  Hermitian: a line is a column PAIR and a thread loads two values per (k0, line) slot.
    const int load_cap = herm ? (kCoopLoads / 2) * kLineThreads / nrow : kCoopLoads * kLineThreads / F0;
    int lpbc = 1;
    while (lpbc * 2 <= std::min(ncol / G, load_cap)) lpbc <<= 1;
    // LDS of a column pass: two images of lpbc lines (+ the Hermitian kernel's slice of the spectrum).  (Until late in round 4 the
    // bound was four images: half the columns per pass -- 96^2, one system per workgroup: 50 -> 42 us per iteration; 384^2
    // general: 30.7 -> 26.9.)
    const size_t lds_factor = std::getenv("EFGP_COOP_LDSF") ? (size_t)std::atoi(std::getenv("EFGP_COOP_LDSF")) : (herm ? 3 : 2);
    while (lpbc > 4 && (lds_factor * lpbc * (F0 + 1) + (size_t)F0 + (size_t)F1) * sizeof(double2) + 2048 > (size_t)max_lds) lpbc >>= 1;
    while (lpbc > 1 && (ncol / G) % lpbc) lpbc >>= 1;           // a pass count per workgroup must be whole (48 R grids: 3 * 2^k lines)
    bool shape_ok = G <= kCoopMaxG && ((nrow + G - 1) / G) * n1 <= ks * kLineThreads && ncol % (G * lpbc) == 0;
    const int rows_wg = (nrow + G - 1) / G, cols_wg = ncol / G;
    int lines = std::min(rows_wg, kCoopLoads * kLineThreads / F1);
    auto lds_for = [&](int ln) {
        const size_t bufsz = (size_t)std::max(ln * (F1 + 1), lpbc * (F0 + 1));
        return (2 * bufsz + (size_t)F1 + (F0 == F1 ? 0 : (size_t)F0)) * sizeof(double2);
    };
    while (lines > 1 && lds_for(lines) + 2048 > (size_t)max_lds) --lines;
    size_t lds = lds_for(lines);
    // Hermitian, one column pass per workgroup: its slice of the spectrum stays in LDS (16-32 KB)
    const size_t spec_bytes = (size_t)F0 * lpbc * sizeof(double2);
    const bool spec_lds = herm && cols_wg == lpbc && lds + spec_bytes + 2048 <= (size_t)max_lds &&
                          std::getenv("EFGP_NO_COOP_SPEC_LDS") == nullptr;
    if (spec_lds) lds += spec_bytes;
    shape_ok = shape_ok && lds + 2048 <= (size_t)max_lds && G <= num_cu &&
               (herm ? lpbc * nrow <= (kCoopLoads / 2) * kLineThreads : lpbc * F0 <= kCoopLoads * kLineThreads);
    const int cap = std::max(1, num_cu / G);                      // systems resident at once (one workgroup per CU)
    const int per = std::min(cap, nbatch);
    CoopShape sh;
    sh.ok = shape_ok;
    sh.herm = herm;
    sh.G = G;
    sh.ks = ks;
    sh.lpbc = lpbc;
    sh.rows_wg = rows_wg;
    sh.cols_wg = cols_wg;
    sh.lines = lines;
    sh.lds = lds;
    sh.spec_lds = spec_lds;
    sh.per = per;
    return sh;
}

int pick_persistent(const ToepGeom& full, const CgSolve& s, bool have_h48, bool lanczos, bool fuse, PersistentChoice* out) {
    const int64_t n = full.n[0], F = full.F[0];
    // the specialised kernels are picked by the caller's shape: a block with a unit axis runs the generic kernel on its other axes
    const bool fast64 = full.d == 2 && F == 64 && full.F[1] == 64 && n == full.n[1] && n <= 32 && !hook("EFGP_NO_CG64");
    const bool herm64 = fast64 && s.hermitian && !lanczos && (n & 1) && n <= 31 && !hook("EFGP_NO_CG_HERM");
    // blocks of up to 23 x 23 modes: the smallest circulant grid, 48 x 48 (the operator holds a second spectrum for it)
    const bool herm48 = herm64 && have_h48 && n <= 23 && !hook("EFGP_NO_CG48");
    if (fuse && !(herm48 && s.variant == 0 && s.nbatch == 1 && s.zero_x0 && s.b_times_ws && !s.diag)) {
        set_error("fused mean solve: the system is not a cold-start 48 x 48 Hermitian mean solve");
        return EFGP_EUNSUPPORTED;
    }
    // EFGP_CG48_FFT2D=1: the round 4 operator application (packed column transforms) instead of the per-frequency Toeplitz products.
    // Batches keep it too: the resident coefficients take the kernel to 256 + 16 registers, one workgroup per CU instead of two.
    out->dense48 = s.nbatch == 1 && !hook("EFGP_CG48_FFT2D");
    if (herm48) out->pick = fuse ? PersistentPick::fused48 : PersistentPick::herm48;
    else if (herm64) out->pick = PersistentPick::herm64;
    else if (full.d == 1 && !lanczos && n <= 64 * pcg::l1d::KS - 1 && F >= 8 && F <= 512 && (F & (F - 1)) == 0 && !hook("EFGP_NO_CG_LINE1D"))
        out->pick = PersistentPick::line1d;          // 1-D: one wave per system
    else out->pick = fast64 ? PersistentPick::fast64 : PersistentPick::generic;
    return EFGP_OK;
}

}  // namespace efgp
