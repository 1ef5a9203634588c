// Shared by the 3-D stages: what more than one of spatial.hip, nearest.hip and density.hip needs of the voxel grid (the
// cell of a point, the search over the cells' keys, the walk over a point's 27 cells) and of the forest over a bit
// array's elements.  Anything a single unit uses stays in that unit.
#pragma once

#include <cmath>

#include "rows.h"

namespace bff {

constexpr int kCellBits = 21;                                      // bits per axis in a key q0 + (q1 << 21) + (q2 << 42)
constexpr int64_t kCellAxis = 1ll << kCellBits;                    // cells per axis

// the cell coordinate of x on one axis: IEEE subtraction, IEEE division, floor (the units are compiled with
// -ffp-contract=off), on the device and in the host's checks alike
__host__ __device__ inline double cell_coord(double x, double lo, double cell) { return floor((x - lo) / cell); }

// the first position with keys[pos] >= want; keys is ascending
__device__ __forceinline__ int64_t keys_lower_bound(const int64_t *__restrict__ keys, int64_t n, int64_t want)
{
    int64_t a = 0, b = n;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (keys[m] < want) a = m + 1; else b = m;
    }
    return a;
}

// The search index of a cloud (lift.nearest_index): the points that have a cell gathered into (cell, point index) order,
// so that the candidates of a cell are contiguous.
struct CellIndex {
    const double *cloud;                                           // f64 [M'][3]
    const int64_t *keys;                                           // i64 [V], the distinct keys, ascending
    const int32_t *offs;                                           // i32 [V + 1]: cell v is [offs[v], offs[v + 1])
    const int32_t *order;                                          // i32 [M']: the point index of every gathered point
    int64_t n_voxels, n_source;                                    // V, M'
    double lo[3], cell;
};

// The candidates of a point: the gathered points of the 27 cells around its cell.  The three x-neighbours of a (q1, q2)
// pair are consecutive keys, so one lower-bound search and a walk over at most three entries of `keys` give one
// contiguous range: 9 searches, not 27.  fn(i) returns true to stop the walk.
// A point is admitted with a cell coordinate in [-1, 2^21] on every axis: a query of the search may lie one cell outside
// the source's box.  That is a superset of [0, 2^21), the cells themselves, and every element of the DBSCAN passes has a
// cell by construction, so those passes admit what they always did.  The radius test is the caller's.
template <typename Fn>
__device__ __forceinline__ void for_candidates(const CellIndex &ix, const double (&x)[3], Fn fn)
{
    int64_t q[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // the cell is tested on the double, before any conversion (NaN and the infinities fail the test)
        const double f = cell_coord(x[a], ix.lo[a], ix.cell);
        ok = ok && f >= -1.0 && f <= (double)kCellAxis;
        q[a] = ok ? (int64_t)f : 0;
    }
    if (!ok) return;
    const int64_t x_lo = q[0] > 0 ? q[0] - 1 : 0, x_hi = q[0] + 1 < kCellAxis ? q[0] + 1 : kCellAxis - 1;
    for (int d2 = -1; d2 <= 1; ++d2) {
        const int64_t a2 = q[2] + d2;
        if (a2 < 0 || a2 >= kCellAxis) continue;                    // the axis itself: the key must not wrap
        for (int d1 = -1; d1 <= 1; ++d1) {
            const int64_t a1 = q[1] + d1;
            if (a1 < 0 || a1 >= kCellAxis) continue;
            const int64_t base = (a1 << kCellBits) + (a2 << (2 * kCellBits)), want = base + x_lo, last = base + x_hi;
            const int64_t a = keys_lower_bound(ix.keys, ix.n_voxels, want);
            int64_t b = a;
            while (b < ix.n_voxels && b < a + 3 && ix.keys[b] <= last) ++b;
            if (b == a) continue;
            int64_t i = ix.offs[a], end = ix.offs[b];
            i = i > 0 ? i : 0, end = end < ix.n_source ? end : ix.n_source;      // a bad offs entry reads nothing outside
            for (; i < end; ++i)
                if (fn(i)) return;
        }
    }
}

// The index arguments of an entry point, checked and gathered.  Without a cell (n_voxels == 0) no pointer is asked for:
// the walk finds no key and follows none.
inline int cell_index(const char *what, const double *cloud, const int64_t *keys, const int32_t *offs, const int32_t *order,
                      int64_t n_voxels, int64_t n_source, const double *lo_host, double cell, CellIndex &ix)
{
    ix = CellIndex{cloud, keys, offs, order, n_voxels, n_source, {0.0, 0.0, 0.0}, cell};
    if (n_voxels == 0) return BFF_OK;
    BFF_REQUIRE(cloud && keys && offs && order && lo_host, "%s: null pointer (the index: src or cloud, keys, offs, order, lo_host)",
                what);
    for (int a = 0; a < 3; ++a) {
        ix.lo[a] = lo_host[a];
        BFF_REQUIRE(std::isfinite(ix.lo[a]), "%s: lo_host: the grid's minimum is not finite", what);
    }
    return BFF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The forest over the elements of a [K][vw] bit array (the split's occupied (row, cell) pairs, the clustering's
// (row, point) pairs), numbered in (row, bit) order; uf_find and uf_union: rows.h.

// the element of bit v of row k; the bit is set.  prefix[k][w] = set bits of row k below word w, elem_offs[k] = set bits
// of the rows before k
__device__ __forceinline__ int element_of(const uint64_t *__restrict__ bits, const int32_t *__restrict__ prefix,
                                          const int32_t *__restrict__ elem_offs, int64_t vw, int k, int64_t v)
{
    const int64_t i = (int64_t)k * vw + (v >> 6);
    return elem_offs[k] + prefix[i] + popc64(bits[i] & ((1ull << (v & 63)) - 1));
}

// The kernels are spatial.hip's; density.hip launches them through these.
void elements_prefix(const uint64_t *bits, int32_t n_rows, int64_t vw, int32_t *prefix, int32_t *row_total, hipStream_t st);
void forest_init(int32_t *parent, int32_t n_elems, hipStream_t st);         // every element its own root
void forest_flatten(int32_t *parent, int32_t n_elems, hipStream_t st);      // after the unions: every element at its root

}  // namespace bff
