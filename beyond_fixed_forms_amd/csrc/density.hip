// 3-D instances clustered by density, DBSCAN with a deterministic border rule (include/bff_hip.h: bff_dbscan_*;
// DESIGN.md section 7j).  An instance is a bit row over the cloud; its points are counted against their neighbours within
// eps in the same row, the core points are joined by the lock-free union-find of the split, every border point follows
// its nearest core neighbour, and the tail of the split (bff_split_count, bff_split_emit with every point its own cell)
// turns the clusters into bit rows.  The walk over a point's 27 cells, the element index and the forest's prefix, init
// and flatten kernels are shared with spatial.hip and nearest.hip: cells.h.
//
// Data layout in HBM
//   points   f64 [N][stride >= 3]   the cloud in the caller's point order (x, y, z first): the queries
//   cloud    f64 [M'][3]            the finite points gathered into (cell, point index) order: the candidates of a cell
//                                   are contiguous (the index of the lift, nearest.hip)
//   order    i32 [M']               the point index of every gathered point;  offs i32 [V + 1];  keys i64 [V], ascending
//   rows     u64 [K][nw]            the instances; bits at positions >= N are ignored
//   finite   u64 [vw]               vw = ceil(N / 64): bit p = point p has a cell
//   set      u64 [K][vw]            rows & finite, the bits at positions >= N zero: the elements
//   prefix   i32 [K][vw]            set bits of set[k] below word w;  elem_offs i32 [K + 1]: set bits of the rows before k
//   core     u64 [K][vw]            bit p of row k = p is a core point of row k
//   parent   i32 [T]                per element (numbered in (row, point) order:
//                                   e = elem_offs[k] + prefix[k][p >> 6] + popcount(set[k][p >> 6] below bit p)):
//                                   core -> the smallest core element of its cluster, border -> that of its nearest core
//                                   neighbour's cluster, noise -> -1
// No [K][N] integer array exists: what is per (row, point) is a bit, what is per element is indexed by e.
// Work shape: one wave per 64-bit word of a row, lane = point, in the caller's point order.
#include "cells.h"

namespace bff {

// d2 of the statement: every operation rounded (-ffp-contract=off); the squares make it symmetric in its two points
__device__ __forceinline__ bool den_near(const CellIndex &ix, double eps2, const double (&x)[3], int64_t i, double &d)
{
    const double dx = x[0] - ix.cloud[i * 3], dy = x[1] - ix.cloud[i * 3 + 1], dz = x[2] - ix.cloud[i * 3 + 2];
    d = (dx * dx + dy * dy) + dz * dz;
    return d <= eps2;
}

// one thread per word of set: the row's word masked by the finite points and by N
__global__ __launch_bounds__(256) void dbscan_mask_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                           int64_t n_points, const uint64_t *__restrict__ finite, int64_t vw,
                                                           uint64_t *__restrict__ set)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)n_rows * vw) return;
    const int64_t k = g / vw, w = g % vw;
    const int64_t left = n_points - w * 64;
    const uint64_t tail = left >= 64 ? ~0ull : (left > 0 ? (1ull << left) - 1 : 0);
    set[g] = rows[k * nw + w] & finite[w] & tail;
}

// ---------------------------------------------------------------------------------------------------------------------
// The point passes share one shape: one wave per 64-bit word of set, lane = point.
struct DenWord {
    int k;                                                         // the row
    int64_t w;                                                     // the word
    uint64_t word;                                                 // set[k][w]
    bool on;                                                       // this lane's point is an element
    int64_t p;                                                     // the point
    double x[3];
};

// wave-uniform false: no such word, or a zero word
__device__ __forceinline__ bool den_word(const uint64_t *__restrict__ set, int n_rows, int64_t vw, int64_t n_points,
                                         const double *__restrict__ points, int64_t stride, DenWord &dw)
{
    const int64_t g = (int64_t)blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);
    if (g >= (int64_t)n_rows * vw) return false;
    dw.k = (int)(g / vw);
    dw.w = g % vw;
    dw.word = set[g];
    if (dw.word == 0) return false;
    dw.p = dw.w * kWave + lane_id();
    dw.on = ((dw.word >> lane_id()) & 1) && dw.p < n_points;       // bff_dbscan_elements leaves no bit at a position >= N
    dw.x[0] = dw.x[1] = dw.x[2] = 0.0;
    if (dw.on) {
#pragma unroll
        for (int a = 0; a < 3; ++a) dw.x[a] = points[dw.p * stride + a];
    }
    return true;
}

// bit s of row k of a [K][vw] bit array; s is an entry of `order` and is checked before it is followed
__device__ __forceinline__ bool den_bit(const uint64_t *__restrict__ bits, int64_t vw, int k, int64_t n_points, int32_t s)
{
    if ((uint32_t)s >= (uint64_t)n_points) return false;
    return (bits[(int64_t)k * vw + (s >> 6)] >> (s & 63)) & 1;
}

// core: the count stops at min_samples (core is a threshold).  The row's bit is tested before the distance.
__global__ __launch_bounds__(256) void dbscan_core_kernel(const uint64_t *__restrict__ set, int n_rows, int64_t vw,
                                                           int64_t n_points, const double *__restrict__ points, int64_t stride,
                                                           CellIndex ix, double eps2, int min_samples, uint64_t *__restrict__ core)
{
    DenWord dw;
    if (!den_word(set, n_rows, vw, n_points, points, stride, dw)) return;     // core was cleared: a zero word stays zero
    int count = 0;
    if (dw.on) {
        for_candidates(ix, dw.x, [&](int64_t i) {
            double d;
            if (den_bit(set, vw, dw.k, n_points, ix.order[i]) && den_near(ix, eps2, dw.x, i, d)) ++count;
            return count >= min_samples;
        });
    }
    const uint64_t votes = __ballot(dw.on && count >= min_samples);
    if (lane_id() == 0) core[(int64_t)dw.k * vw + dw.w] = votes;    // one writer per word
}

// every core point against its core neighbours of a smaller index (the relation is symmetric: the other half is theirs)
__global__ __launch_bounds__(256) void dbscan_union_kernel(const uint64_t *__restrict__ set, const uint64_t *__restrict__ core,
                                                            const int32_t *__restrict__ prefix, const int32_t *__restrict__ elem_offs,
                                                            int n_rows, int64_t vw, int64_t n_points,
                                                            const double *__restrict__ points, int64_t stride, CellIndex ix, double eps2,
                                                            int n_elems, int32_t *__restrict__ parent)
{
    DenWord dw;
    if (!den_word(set, n_rows, vw, n_points, points, stride, dw)) return;
    if (!dw.on || !((core[(int64_t)dw.k * vw + dw.w] >> lane_id()) & 1)) return;
    const int e = element_of(set, prefix, elem_offs, vw, dw.k, dw.p);
    if ((unsigned)e >= (unsigned)n_elems) return;                   // elem_offs of another call: nothing is followed
    for_candidates(ix, dw.x, [&](int64_t i) {
        const int32_t s = ix.order[i];
        double d;
        // core is a subset of set: the element below exists
        if ((int64_t)s < dw.p && den_bit(core, vw, dw.k, n_points, s) && den_near(ix, eps2, dw.x, i, d)) {
            const int e2 = element_of(set, prefix, elem_offs, vw, dw.k, s);
            if ((unsigned)e2 < (unsigned)n_elems) uf_union(parent, e, e2);
        }
        return false;
    });
}

// After the flatten (a kernel boundary).  A non-core element takes the root of its nearest core neighbour (equal d2 to
// the smallest point index: the nine ranges are not in index order), or -1.  It writes its own slot only and reads core
// elements' slots only, which nobody writes here: nothing races.
__global__ __launch_bounds__(256) void dbscan_border_kernel(const uint64_t *__restrict__ set, const uint64_t *__restrict__ core,
                                                             const int32_t *__restrict__ prefix, const int32_t *__restrict__ elem_offs,
                                                             int n_rows, int64_t vw, int64_t n_points,
                                                             const double *__restrict__ points, int64_t stride, CellIndex ix, double eps2,
                                                             int n_elems, int32_t *parent)
{
    DenWord dw;
    if (!den_word(set, n_rows, vw, n_points, points, stride, dw)) return;
    if (!dw.on || ((core[(int64_t)dw.k * vw + dw.w] >> lane_id()) & 1)) return;
    const int e = element_of(set, prefix, elem_offs, vw, dw.k, dw.p);
    if ((unsigned)e >= (unsigned)n_elems) return;
    double best = INFINITY;
    int32_t best_s = -1;
    for_candidates(ix, dw.x, [&](int64_t i) {
        const int32_t s = ix.order[i];
        double d;
        if (den_bit(core, vw, dw.k, n_points, s) && den_near(ix, eps2, dw.x, i, d) &&
            (d < best || (d == best && (best_s < 0 || s < best_s))))
            best = d, best_s = s;
        return false;
    });
    int root = -1;
    if (best_s >= 0) {
        const int e2 = element_of(set, prefix, elem_offs, vw, dw.k, best_s);
        if ((unsigned)e2 < (unsigned)n_elems) root = parent[e2];
    }
    parent[e] = root;
}

static int den_sizes(const char *what, int32_t n_rows, int64_t n_points)
{
    BFF_REQUIRE(n_rows >= 0 && n_points >= 0, "%s: bad sizes (n_rows, n_points)", what);
    BFF_LIMIT(n_points < (1ll << 31), "%s: n_points: at most 2^31 - 1 points", what);
    // every element is a set bit of `set`: its index stays below 2^31
    BFF_LIMIT((int64_t)n_rows * ceil_div(n_points, 64) * 64 < (1ll << 31), "%s: n_rows x n_points = %lld x %lld, at most 2^31 - 1 bits",
              what, (long long)n_rows, (long long)n_points);
    return BFF_OK;
}

static int den_numbers(const char *what, int64_t n_voxels, int64_t n_source, int64_t n_points, int64_t stride, double cell,
                       double eps)
{
    BFF_REQUIRE(n_voxels >= 0 && n_source >= 0, "%s: bad sizes (n_voxels, n_source)", what);
    BFF_REQUIRE(stride >= 3, "%s: stride: at least 3 doubles per point", what);
    BFF_REQUIRE(eps > 0.0 && std::isfinite(eps), "%s: eps must be a finite number > 0", what);
    BFF_REQUIRE(cell >= eps && std::isfinite(cell), "%s: cell must be a finite number >= eps", what);
    BFF_REQUIRE(n_voxels <= n_source && n_source <= n_points, "%s: n_voxels <= n_source <= n_points expected, got %lld, %lld, %lld",
                what, (long long)n_voxels, (long long)n_source, (long long)n_points);
    return BFF_OK;
}

static unsigned den_word_blocks(int32_t n_rows, int64_t vw) { return (unsigned)ceil_div((int64_t)n_rows * vw, 256 / kWave); }

}  // namespace bff

using namespace bff;

extern "C" int bff_dbscan_elements(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const uint64_t *finite,
                                   uint64_t *set, int32_t *prefix, int32_t *row_total, void *stream)
{
    BFF_REQUIRE(nw >= 0, "bff_dbscan_elements: bad sizes (nw)");
    int rc = den_sizes("bff_dbscan_elements", n_rows, n_points);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(nw >= ceil_div(n_points, 64), "bff_dbscan_elements: nw: rows of %lld words for %lld points", (long long)nw,
                (long long)n_points);
    if (n_rows == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(rows && finite, "bff_dbscan_elements: null pointer (rows, finite)");
    BFF_REQUIRE(set && prefix && row_total, "bff_dbscan_elements: null pointer (set, prefix, row_total)");
    hipStream_t st = as_stream(stream);
    const int64_t vw = ceil_div(n_points, 64);
    dbscan_mask_kernel<<<(unsigned)ceil_div((int64_t)n_rows * vw, 256), 256, 0, st>>>(rows, n_rows, nw, n_points, finite, vw, set);
    elements_prefix(set, n_rows, vw, prefix, row_total, st);
    return launched("bff_dbscan_elements");
}

extern "C" int bff_dbscan_core(const uint64_t *set, int32_t n_rows, int64_t n_points, const double *points, int64_t stride,
                               const double *cloud, const int64_t *keys, const int32_t *offs, const int32_t *order,
                               int64_t n_voxels, int64_t n_source, const double *lo_host, double cell, double eps,
                               int32_t min_samples, uint64_t *core, void *stream)
{
    int rc = den_sizes("bff_dbscan_core", n_rows, n_points);
    if (rc == BFF_OK) rc = den_numbers("bff_dbscan_core", n_voxels, n_source, n_points, stride, cell, eps);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(min_samples >= 1, "bff_dbscan_core: min_samples must be >= 1");
    if (n_rows == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(core, "bff_dbscan_core: null pointer (core)");
    BFF_REQUIRE(n_voxels == 0 || (set && points), "bff_dbscan_core: null pointer (set, points)");
    CellIndex ix;
    rc = cell_index("bff_dbscan_core", cloud, keys, offs, order, n_voxels, n_source, lo_host, cell, ix);
    if (rc != BFF_OK) return rc;
    hipStream_t st = as_stream(stream);
    const int64_t vw = ceil_div(n_points, 64);
    hipError_t e = hipMemsetAsync(core, 0, sizeof(uint64_t) * (size_t)n_rows * (size_t)vw, st);
    if (e != hipSuccess) return fail((int)e, "bff_dbscan_core: memset: %s", hipGetErrorString(e));
    if (n_voxels == 0) return BFF_OK;                               // no finite point: no element
    dbscan_core_kernel<<<den_word_blocks(n_rows, vw), 256, 0, st>>>(set, n_rows, vw, n_points, points, stride, ix, eps * eps, min_samples, core);
    return launched("bff_dbscan_core");
}

extern "C" int bff_dbscan_link(const uint64_t *set, const uint64_t *core, const int32_t *prefix, const int32_t *elem_offs,
                               int32_t n_rows, int64_t n_points, const double *points, int64_t stride, const double *cloud,
                               const int64_t *keys, const int32_t *offs, const int32_t *order, int64_t n_voxels,
                               int64_t n_source, const double *lo_host, double cell, double eps, int32_t n_elems,
                               int32_t *parent, void *stream)
{
    int rc = den_sizes("bff_dbscan_link", n_rows, n_points);
    if (rc == BFF_OK) rc = den_numbers("bff_dbscan_link", n_voxels, n_source, n_points, stride, cell, eps);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(n_elems >= 0, "bff_dbscan_link: bad sizes (n_elems)");
    if (n_rows == 0 || n_points == 0 || n_elems == 0 || n_voxels == 0) return BFF_OK;
    BFF_REQUIRE(parent, "bff_dbscan_link: null pointer (parent)");
    BFF_REQUIRE(set && core && prefix && elem_offs && points, "bff_dbscan_link: null pointer (set, core, prefix, elem_offs, points)");
    CellIndex ix;
    rc = cell_index("bff_dbscan_link", cloud, keys, offs, order, n_voxels, n_source, lo_host, cell, ix);
    if (rc != BFF_OK) return rc;
    hipStream_t st = as_stream(stream);
    const int64_t vw = ceil_div(n_points, 64);
    const unsigned wb = den_word_blocks(n_rows, vw);
    forest_init(parent, n_elems, st);
    dbscan_union_kernel<<<wb, 256, 0, st>>>(set, core, prefix, elem_offs, n_rows, vw, n_points, points, stride, ix, eps * eps, n_elems, parent);
    forest_flatten(parent, n_elems, st);
    dbscan_border_kernel<<<wb, 256, 0, st>>>(set, core, prefix, elem_offs, n_rows, vw, n_points, points, stride, ix, eps * eps, n_elems, parent);
    return launched("bff_dbscan_link");
}
