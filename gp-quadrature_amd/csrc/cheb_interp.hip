// Tensor-product barycentric interpolation from a small node box to many points behind the C ABI:
//   efgp_cheb_interp   out[p] = sum_{i_0..i_{d-1}} prod_a w_a[i_a](x_p) V[i_0, .., i_{d-1}]   (pg_classifier.py:894-942, 1000-1003)
// The Chebyshev route of the PG estimators' predictive variance evaluates the exact variance at n^d nodes and interpolates it at every
// test point; the reference builds an (npts, n) matrix per axis on the host and contracts them with einsum.  Here one thread owns one
// point: the nodes, weights and node values sit in LDS (at most 3 KB + 32 KB per workgroup, every lane reads the same address: a
// broadcast), and the per-axis weights never exist as an array.  Per axis the first pass finds the node the point sits on (if any) and
// the normaliser S_a = sum_l c_l / (x - x_l); the contraction then recomputes the raw weight c_k / (x - x_k) where it uses it and
// divides each partial sum by its axis's S_a (the nested second barycentric formula), so a thread keeps 2 d scalars instead of
// sum_a n_a weights that a dynamically indexed private array would send to scratch.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace efgp {

constexpr int CHEB_MAX_AXIS = 64;        // nodes per axis
constexpr int CHEB_MAX_BOX = 4096;       // node values: 32 KB of LDS
constexpr double CHEB_HIT = 1e-14;       // |x - x_k| <= CHEB_HIT: the point is the node (pg_classifier.py:899, 907)

struct ChebGeom {
    int n0, n1, n2;      // nodes per slot, real axes right-aligned (unused leading slots hold one node), last slot fastest
    int dim;
    int total;           // n0 n1 n2
};

// hit = the first node (ascending) within CHEB_HIT of x, else -1; S = sum_l c_l / (x - x_l), 1 on a hit
__device__ __forceinline__ void cheb_axis_prepare(const double* nd, const double* wt, int n, double x, int& hit, double& S) {
    int h = -1;
    double s = 0.0;
    for (int k = 0; k < n; ++k) {
        const double diff = x - nd[k];
        if (h < 0 && fabs(diff) <= CHEB_HIT) h = k;
        s += wt[k] / diff;
    }
    hit = h;
    S = h >= 0 ? 1.0 : s;
}

// raw weight of node k: one-hot on a hit, else c_k / (x - x_k)
__device__ __forceinline__ double cheb_raw(const double* nd, const double* wt, int k, double x, int hit) {
    const double r = wt[k] / (x - nd[k]);
    return hit >= 0 ? (k == hit ? 1.0 : 0.0) : r;
}

__global__ __launch_bounds__(256) void cheb_interp_kernel(ChebGeom g, const double* __restrict__ nodes, const double* __restrict__ weights,
                                                          const double* __restrict__ values, const double* __restrict__ x, int64_t npts,
                                                          int clamp_nonneg, double* __restrict__ out) {
    __shared__ double s_val[CHEB_MAX_BOX];
    __shared__ double s_nd[3 * CHEB_MAX_AXIS];
    __shared__ double s_wt[3 * CHEB_MAX_AXIS];
    const int tid = threadIdx.x;
    for (int i = tid; i < g.total; i += 256) s_val[i] = values[i];
    // slot s holds axis s - (3 - dim); an unused slot is one node at 0 with weight 1, which a coordinate of 0 hits
    if (tid < CHEB_MAX_AXIS) {
        const int src1 = g.dim >= 3 ? g.n0 : 0, src2 = src1 + (g.dim >= 2 ? g.n1 : 0);
        if (tid < g.n0) {
            s_nd[tid] = g.dim >= 3 ? nodes[tid] : 0.0;
            s_wt[tid] = g.dim >= 3 ? weights[tid] : 1.0;
        }
        if (tid < g.n1) {
            s_nd[CHEB_MAX_AXIS + tid] = g.dim >= 2 ? nodes[src1 + tid] : 0.0;
            s_wt[CHEB_MAX_AXIS + tid] = g.dim >= 2 ? weights[src1 + tid] : 1.0;
        }
        if (tid < g.n2) {
            s_nd[2 * CHEB_MAX_AXIS + tid] = nodes[src2 + tid];
            s_wt[2 * CHEB_MAX_AXIS + tid] = weights[src2 + tid];
        }
    }
    __syncthreads();
    const double* nd0 = s_nd;
    const double* nd1 = s_nd + CHEB_MAX_AXIS;
    const double* nd2 = s_nd + 2 * CHEB_MAX_AXIS;
    const double* wt0 = s_wt;
    const double* wt1 = s_wt + CHEB_MAX_AXIS;
    const double* wt2 = s_wt + 2 * CHEB_MAX_AXIS;
    for (int64_t p = (int64_t)blockIdx.x * 256 + tid; p < npts; p += (int64_t)gridDim.x * 256) {
        const double* xp = x + p * g.dim;
        const double x2 = xp[g.dim - 1];
        const double x1 = g.dim >= 2 ? xp[g.dim - 2] : 0.0;
        const double x0 = g.dim >= 3 ? xp[0] : 0.0;
        int h0, h1, h2;
        double S0, S1, S2;
        cheb_axis_prepare(nd0, wt0, g.n0, x0, h0, S0);
        cheb_axis_prepare(nd1, wt1, g.n1, x1, h1, S1);
        cheb_axis_prepare(nd2, wt2, g.n2, x2, h2, S2);
        double acc0 = 0.0;
        for (int i0 = 0; i0 < g.n0; ++i0) {
            double acc1 = 0.0;
            for (int i1 = 0; i1 < g.n1; ++i1) {
                const double* row = s_val + (i0 * g.n1 + i1) * g.n2;
                double acc2 = 0.0;
                for (int i2 = 0; i2 < g.n2; ++i2) acc2 += cheb_raw(nd2, wt2, i2, x2, h2) * row[i2];
                acc1 += cheb_raw(nd1, wt1, i1, x1, h1) * (acc2 / S2);
            }
            acc0 += cheb_raw(nd0, wt0, i0, x0, h0) * (acc1 / S1);
        }
        const double v = acc0 / S0;
        out[p] = (clamp_nonneg && v < 0.0) ? 0.0 : v;                 // clamp_min(0): a NaN stays a NaN
    }
}

}  // namespace efgp

using namespace efgp;

extern "C" int efgp_cheb_interp(int device, int dim, const int64_t* n_nodes, const double* nodes, const double* bary_weights,
                                const double* node_values, const double* x_new, int64_t npts, int clamp_nonneg, double* out,
                                void* stream_) {
    EFGP_REQUIRE(dim >= 1 && dim <= 3, "efgp_cheb_interp: dim must be 1, 2 or 3 (got %d)", dim);
    EFGP_REQUIRE(n_nodes, "efgp_cheb_interp: null n_nodes");
    int64_t total = 1;
    for (int a = 0; a < dim; ++a) {
        EFGP_REQUIRE(n_nodes[a] >= 2 && n_nodes[a] <= CHEB_MAX_AXIS, "efgp_cheb_interp: n_nodes[%d] = %lld must be 2..%d", a,
                     (long long)n_nodes[a], CHEB_MAX_AXIS);
        total *= n_nodes[a];
    }
    EFGP_REQUIRE(total <= CHEB_MAX_BOX, "efgp_cheb_interp: the product of n_nodes, %lld, exceeds %d node values", (long long)total,
                 CHEB_MAX_BOX);
    EFGP_REQUIRE(npts >= 0, "efgp_cheb_interp: npts must be >= 0 (got %lld)", (long long)npts);
    if (npts == 0) return EFGP_OK;
    EFGP_REQUIRE(nodes, "efgp_cheb_interp: null nodes");
    EFGP_REQUIRE(bary_weights, "efgp_cheb_interp: null bary_weights");
    EFGP_REQUIRE(node_values, "efgp_cheb_interp: null node_values");
    EFGP_REQUIRE(x_new, "efgp_cheb_interp: null x_new");
    EFGP_REQUIRE(out, "efgp_cheb_interp: null out");
    if (!device_ctx(device)) return EFGP_EHIP;
    DeviceGuard guard(device, (hipStream_t)stream_);
    ChebGeom g;
    g.dim = dim;
    g.n0 = dim >= 3 ? (int)n_nodes[0] : 1;
    g.n1 = dim >= 2 ? (int)n_nodes[dim - 2] : 1;
    g.n2 = (int)n_nodes[dim - 1];
    g.total = (int)total;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((npts + 255) / 256, 1024));
    hipLaunchKernelGGL(cheb_interp_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, g, nodes, bary_weights, node_values, x_new, npts,
                       clamp_nonneg, out);
    EFGP_HIP_CHECK(hipGetLastError());
    return EFGP_OK;
}
