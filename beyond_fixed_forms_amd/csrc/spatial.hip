// 3-D instances split into spatially connected parts (include/bff_hip.h: bff_voxel_*, bff_split_*).
// An instance is a bit row over the cloud; here its points are binned into the cells of a voxel grid, cells that touch
// (26-adjacency) are joined by a lock-free union-find, and every component becomes a bit row of its own.
// What nearest.hip and density.hip share with this unit is in cells.h: the cell of a point, the search over `keys`, the
// element index; the forest's prefix, init and flatten kernels are defined here and launched by density.hip as well.
//
// Data layout in HBM
//   points   f64 [N][stride >= 3]   the cloud in the caller's point order (x, y, z first)
//   box      u64 [6]                min x, y, z and max x, y, z over the finite points as order-preserving integers
//   key      i64 [N]                q0 + (q1 << 21) + (q2 << 42) of the point's cell, kVoxNoKey for a non-finite point
//   keys     i64 [V]                the distinct keys, ascending; a cell's rank is its position here
//   vox      i32 [N]                the rank of the point's cell, -1 for a non-finite point (read coalesced: lane = point)
//   nbr      i32 [V][13]            ranks of the 13 forward neighbours, -1 = empty or outside the grid
//   rows     u64 [K][nw]            the instances; bits at positions >= N are ignored
//   occ      u64 [K][vw]            vw = ceil(V / 64): bit v of row k = row k holds a point of cell v
//   prefix   i32 [K][vw]            set bits of occ[k] below word w;  elem_offs i32 [K + 1]: set bits of the rows before k
//   parent   i32 [T]                the forest over the T occupied (row, cell) pairs ("elements", numbered in (k, v) order:
//                                   e = elem_offs[k] + prefix[k][v >> 6] + popcount(occ[k][v >> 6] below bit v))
//   count    i32 [T]                points of the component whose root (= smallest element = anchor) is e
//   table    i32 [T]                root element -> output row, or -1
//   out      u64 [R][nw]            the parts
// No [K][V] or [K][N] integer array exists: what is per (row, cell) is a bit, what is per element is indexed by e.
#include "cells.h"

namespace bff {

constexpr int64_t kVoxNoKey = 0x7fffffffffffffffll;               // sorts after every key (keys are < 2^63)
constexpr int kVoxNbr = 13;

// doubles as unsigned integers of the same order (NaN aside, which is never encoded)
__device__ __forceinline__ uint64_t order_bits(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// one thread per point, 4 waves per block; a wave reduces its finite points and makes six atomics at most
__global__ __launch_bounds__(256) void voxel_bounds_kernel(const double *__restrict__ points, int64_t n, int64_t stride,
                                                            unsigned long long *__restrict__ box)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
    if (p < n) {
        const double x = points[p * stride], y = points[p * stride + 1], z = points[p * stride + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            lo[0] = hi[0] = order_bits(x);
            lo[1] = hi[1] = order_bits(y);
            lo[2] = hi[2] = order_bits(z);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t l = __shfl_xor(lo[a], d), h = __shfl_xor(hi[a], d);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    if (lane_id() == 0 && lo[0] != ~0ull) {                         // a wave without a finite point offers nothing
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(box + a, (unsigned long long)lo[a]);
            atomicMax(box + 3 + a, (unsigned long long)hi[a]);
        }
    }
}

struct VoxelFrame { double lo[3]; double cell; };

// the key of every point's cell (cells.h: cell_coord)
__global__ __launch_bounds__(256) void voxel_keys_kernel(const double *__restrict__ points, int64_t n, int64_t stride,
                                                          VoxelFrame fr, int64_t *__restrict__ key)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x[3] = {points[p * stride], points[p * stride + 1], points[p * stride + 2]};
    int64_t k = kVoxNoKey;
    if (isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2])) {
        k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double q = cell_coord(x[a], fr.lo[a], fr.cell);
            // 0 <= q < 2^21 for a box that holds the point (checked by the entry point); anything else has no cell
            if (!(q >= 0.0 && q < (double)kCellAxis)) { k = kVoxNoKey; break; }
            k += (int64_t)q << (kCellBits * a);
        }
    }
    key[p] = k;
}

// sorted keys -> 1 where a new cell starts
__global__ __launch_bounds__(256) void voxel_heads_kernel(const int64_t *__restrict__ sorted, int64_t n, int32_t *__restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = sorted[i];
    head[i] = (k != kVoxNoKey && (i == 0 || sorted[i - 1] != k)) ? 1 : 0;
}

// heads_incl: the inclusive prefix sum of head.  Position i of the sorted list holds point order[i].
__global__ __launch_bounds__(256) void voxel_ranks_kernel(const int64_t *__restrict__ sorted, const int32_t *__restrict__ order,
                                                           const int64_t *__restrict__ heads_incl, int64_t n, int64_t n_voxels,
                                                           int32_t *__restrict__ vox, int64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = sorted[i], p = order[i], r = heads_incl[i] - 1;
    if ((uint64_t)p >= (uint64_t)n) return;                         // a bad order entry writes nothing
    const bool cell = k != kVoxNoKey && r >= 0 && r < n_voxels;
    vox[p] = cell ? (int32_t)r : -1;
    if (cell && (i == 0 || sorted[i - 1] != k)) keys[r] = k;
}

// forward neighbour j of a cell: the offsets (d2, d1, d0) > (0, 0, 0) in lexicographic order
__device__ __forceinline__ void forward_offset(int j, int &d2, int &d1, int &d0)
{
    if (j == 0) { d2 = 0, d1 = 0, d0 = 1; return; }
    if (j < 4) { d2 = 0, d1 = 1, d0 = j - 2; return; }
    d2 = 1, d1 = (j - 4) / 3 - 1, d0 = (j - 4) % 3 - 1;
}

// one thread per (cell, neighbour): the axis test, then a binary search over the ascending keys
__global__ __launch_bounds__(256) void voxel_neighbours_kernel(const int64_t *__restrict__ keys, int64_t n_voxels,
                                                                int32_t *__restrict__ nbr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_voxels * kVoxNbr) return;
    const int64_t v = t / kVoxNbr;
    const int j = (int)(t % kVoxNbr);
    const int64_t k = keys[v];
    int d[3];
    forward_offset(j, d[2], d[1], d[0]);
    int64_t want = 0;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int64_t q = ((k >> (kCellBits * a)) & (kCellAxis - 1)) + d[a];
        inside = inside && q >= 0 && q < kCellAxis;                 // the axis itself: the key must not wrap
        want += q << (kCellBits * a);
    }
    int32_t found = -1;
    if (inside) {
        const int64_t a = keys_lower_bound(keys, n_voxels, want);
        if (a < n_voxels && keys[a] == want) found = (int32_t)a;
    }
    nbr[t] = found;
}

// ---------------------------------------------------------------------------------------------------------------------
// The row passes (occupancy, count, emit) share one shape: one wave per 64-bit word of a row, lane = point.
struct RowWord {
    int k;                                                         // the row
    int64_t w;                                                     // the word
    bool set;                                                      // this lane's point is in the row and has a cell
    int32_t v;                                                     // its cell
};

// wave-uniform false: no such word, or a zero word
__device__ __forceinline__ bool row_word(const uint64_t *__restrict__ rows, int n_rows, int64_t nw, int64_t n_points,
                                         const int32_t *__restrict__ vox, int64_t n_voxels, RowWord &rw)
{
    const int64_t g = (int64_t)blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);
    if (g >= (int64_t)n_rows * nw) return false;
    rw.k = (int)(g / nw);
    rw.w = g % nw;
    const uint64_t word = rows[g];
    if (word == 0) return false;
    const int64_t p = rw.w * kWave + lane_id();
    rw.set = false, rw.v = -1;
    if (p < n_points && ((word >> lane_id()) & 1)) {               // bits at positions >= N are ignored
        rw.v = vox[p];
        rw.set = rw.v >= 0 && rw.v < n_voxels;
    }
    return true;
}

__global__ __launch_bounds__(256) void split_occupancy_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                               int64_t n_points, const int32_t *__restrict__ vox,
                                                               int64_t n_voxels, int64_t vw, unsigned long long *__restrict__ occ)
{
    RowWord rw;
    if (!row_word(rows, n_rows, nw, n_points, vox, n_voxels, rw)) return;
    // neighbours in the cloud often share a cell: a lane whose left neighbour offers the same bit stays silent
    const int32_t left = __shfl_up(rw.set ? rw.v : -1, 1);
    if (rw.set && !(lane_id() > 0 && left == rw.v))
        atomicOr(occ + (int64_t)rw.k * vw + (rw.v >> 6), 1ull << (rw.v & 63));      // result unused: returnless
}

// one wave per row of a [K][vw] bit array: the exclusive prefix of the words' popcounts, 64 words a step with the carry
// in a register
__global__ __launch_bounds__(kWave) void elements_prefix_kernel(const uint64_t *__restrict__ occ, int n_rows, int64_t vw,
                                                              int32_t *__restrict__ prefix, int32_t *__restrict__ row_total)
{
    const int k = blockIdx.x, lane = lane_id();
    if (k >= n_rows) return;
    int carry = 0;
    for (int64_t w0 = 0; w0 < vw; w0 += kWave) {
        const int64_t w = w0 + lane;
        const int c = w < vw ? popc64(occ[(int64_t)k * vw + w]) : 0;
        int incl = c;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
        if (w < vw) prefix[(int64_t)k * vw + w] = carry + incl - c;
        carry += __shfl(incl, kWave - 1);
    }
    if (lane == 0) row_total[k] = carry;
}

__global__ __launch_bounds__(256) void forest_init_kernel(int32_t *__restrict__ parent, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = i;
}

// one thread per occ word: every set bit against its 13 forward neighbours in the same row
__global__ __launch_bounds__(256) void split_union_kernel(const uint64_t *__restrict__ occ, const int32_t *__restrict__ prefix,
                                                           const int32_t *__restrict__ elem_offs, int n_rows, int64_t vw,
                                                           int64_t n_voxels, const int32_t *__restrict__ nbr, int n_elems,
                                                           int32_t *__restrict__ parent)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)n_rows * vw) return;
    const int k = (int)(g / vw);
    const int64_t w = g % vw;
    const uint64_t word = occ[g];
    if (word == 0) return;
    const int e0 = elem_offs[k] + prefix[g];
    uint64_t rest = word;
    int below = 0;
    while (rest) {
        const int b = __ffsll((unsigned long long)rest) - 1;
        rest &= rest - 1;
        const int64_t v = w * 64 + b;
        const int e = e0 + below++;
        if (v >= n_voxels || (unsigned)e >= (unsigned)n_elems) return;      // occ past the grid: not this call's
        for (int j = 0; j < kVoxNbr; ++j) {
            const int32_t u = nbr[v * kVoxNbr + j];
            if (u < 0 || u >= n_voxels) continue;
            if (!((occ[(int64_t)k * vw + (u >> 6)] >> (u & 63)) & 1)) continue;
            const int e2 = element_of(occ, prefix, elem_offs, vw, k, u);
            if ((unsigned)e2 < (unsigned)n_elems) uf_union(parent, e, e2);
        }
    }
}

// After the unions (a kernel boundary): every element points at its root.  The walk only reads -- uf_find's path halving
// would let another thread's late store of a grandparent land on top of this thread's root -- so the only stores of this
// kernel are roots, and every parent[] a walk meets is still an ancestor.
__global__ __launch_bounds__(256) void forest_flatten_kernel(int32_t *__restrict__ parent, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x = i, p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (x != i) __hip_atomic_store(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// calls fn(value, lanes) once per distinct value among the wave's active lanes, on the lowest lane that holds it
template <typename Fn>
__device__ __forceinline__ void per_distinct(bool active, int value, Fn fn)
{
    uint64_t todo = __ballot(active);
    while (todo) {                                                  // wave-uniform
        const int src = __ffsll((unsigned long long)todo) - 1;
        const int lead = __shfl(value, src);
        const uint64_t same = __ballot(active && value == lead);
        if (lane_id() == src) fn(lead, same);
        todo &= ~same;
    }
}

// the root of the lane's point, or -1
__device__ __forceinline__ int root_of(const RowWord &rw, const uint64_t *__restrict__ occ, const int32_t *__restrict__ prefix,
                                       const int32_t *__restrict__ elem_offs, int64_t vw, const int32_t *__restrict__ parent,
                                       int n_elems)
{
    if (!rw.set || !((occ[(int64_t)rw.k * vw + (rw.v >> 6)] >> (rw.v & 63)) & 1)) return -1;
    const int e = element_of(occ, prefix, elem_offs, vw, rw.k, rw.v);
    if ((unsigned)e >= (unsigned)n_elems) return -1;
    const int r = parent[e];
    return (unsigned)r < (unsigned)n_elems ? r : -1;
}

__global__ __launch_bounds__(256) void split_count_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                           int64_t n_points, const int32_t *__restrict__ vox, int64_t n_voxels,
                                                           const uint64_t *__restrict__ occ, const int32_t *__restrict__ prefix,
                                                           const int32_t *__restrict__ elem_offs, int64_t vw,
                                                           const int32_t *__restrict__ parent, int n_elems,
                                                           int32_t *__restrict__ count)
{
    RowWord rw;
    if (!row_word(rows, n_rows, nw, n_points, vox, n_voxels, rw)) return;
    const int r = root_of(rw, occ, prefix, elem_offs, vw, parent, n_elems);
    per_distinct(r >= 0, r, [&](int root, uint64_t lanes) { atomicAdd(count + root, popc64(lanes)); });
}

// roots with at least min_points points -> kept[1 + slot] = (root, points), kept[0] = (how many, 0).  The slots depend
// on the run; the host orders the list.
__global__ __launch_bounds__(256) void split_compact_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ count,
                                                             int n_elems, int min_points, int32_t *__restrict__ kept)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n_elems && parent[i] == i && count[i] >= min_points;
    const uint64_t votes = __ballot(keep);
    if (votes == 0) return;
    int base = 0;
    if (lane_id() == __ffsll((unsigned long long)votes) - 1) base = atomicAdd(kept, popc64(votes));
    base = __shfl(base, __ffsll((unsigned long long)votes) - 1);
    if (keep) {
        const int slot = base + popc64(votes & ((1ull << lane_id()) - 1));
        if (slot < n_elems) {                                       // at most one entry per element
            kept[2 * (int64_t)(1 + slot)] = i;
            kept[2 * (int64_t)(1 + slot) + 1] = count[i];
        }
    }
}

// word w of an output row belongs to one parent row, and that row's word w to one wave: plain stores into cleared rows
__global__ __launch_bounds__(256) void split_emit_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                          int64_t n_points, const int32_t *__restrict__ vox, int64_t n_voxels,
                                                          const uint64_t *__restrict__ occ, const int32_t *__restrict__ prefix,
                                                          const int32_t *__restrict__ elem_offs, int64_t vw,
                                                          const int32_t *__restrict__ parent, int n_elems,
                                                          const int32_t *__restrict__ table, int n_out, uint64_t *__restrict__ out)
{
    RowWord rw;
    if (!row_word(rows, n_rows, nw, n_points, vox, n_voxels, rw)) return;
    const int r = root_of(rw, occ, prefix, elem_offs, vw, parent, n_elems);
    const int o = r >= 0 ? table[r] : -1;
    per_distinct(o >= 0 && o < n_out, o, [&](int row, uint64_t lanes) { out[(int64_t)row * nw + rw.w] = lanes; });
}

// the checks the row passes share
static int split_check(const char *what, int32_t n_rows, int64_t nw, int64_t n_points, int64_t n_voxels)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0 && n_points >= 0 && n_voxels >= 0, "%s: bad sizes", what);
    BFF_REQUIRE(nw >= ceil_div(n_points, 64), "%s: rows of %lld words for %lld points", what, (long long)nw, (long long)n_points);
    BFF_LIMIT(n_points < (1ll << 31) && n_voxels < (1ll << 31), "%s: at most 2^31 - 1 points and cells", what);
    // every element is a set bit of occ: its index stays below 2^31
    BFF_LIMIT((int64_t)n_rows * ceil_div(n_voxels, 64) * 64 < (1ll << 31), "%s: rows x cells = %lld x %lld, at most 2^31 - 1 bits",
              what, (long long)n_rows, (long long)n_voxels);
    BFF_LIMIT(ceil_div((int64_t)n_rows * nw, 256 / kWave) < (1ll << 31), "%s: too many row words for one launch", what);
    return BFF_OK;
}

static unsigned row_word_blocks(int32_t n_rows, int64_t nw) { return (unsigned)ceil_div((int64_t)n_rows * nw, 256 / kWave); }

void elements_prefix(const uint64_t *bits, int32_t n_rows, int64_t vw, int32_t *prefix, int32_t *row_total, hipStream_t st)
{
    elements_prefix_kernel<<<(unsigned)n_rows, kWave, 0, st>>>(bits, n_rows, vw, prefix, row_total);
}

void forest_init(int32_t *parent, int32_t n_elems, hipStream_t st)
{
    forest_init_kernel<<<(unsigned)ceil_div(n_elems, 256), 256, 0, st>>>(parent, n_elems);
}

void forest_flatten(int32_t *parent, int32_t n_elems, hipStream_t st)
{
    forest_flatten_kernel<<<(unsigned)ceil_div(n_elems, 256), 256, 0, st>>>(parent, n_elems);
}

}  // namespace bff

using namespace bff;

extern "C" int bff_voxel_bounds(const double *points, int64_t n_points, int64_t stride, uint64_t *box, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && stride >= 3, "bff_voxel_bounds: bad sizes");
    BFF_LIMIT(n_points < (1ll << 31), "bff_voxel_bounds: at most 2^31 - 1 points");
    if (n_points == 0 && !box) return BFF_OK;
    BFF_REQUIRE(box && (points || n_points == 0), "bff_voxel_bounds: null pointer");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(box, 0xff, 3 * sizeof(uint64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(box + 3, 0, 3 * sizeof(uint64_t), st);
    if (e != hipSuccess) return fail((int)e, "bff_voxel_bounds: memset: %s", hipGetErrorString(e));
    if (n_points == 0) return BFF_OK;
    voxel_bounds_kernel<<<(unsigned)ceil_div(n_points, 256), 256, 0, st>>>(points, n_points, stride,
                                                                           reinterpret_cast<unsigned long long *>(box));
    return launched("bff_voxel_bounds");
}

extern "C" int bff_voxel_keys(const double *points, int64_t n_points, int64_t stride, const double *lo_host,
                              const double *hi_host, double cell, int64_t *key, void *stream)
{
    BFF_REQUIRE(cell > 0.0 && std::isfinite(cell), "bff_voxel_keys: cell must be finite and > 0");      // fails on NaN
    BFF_REQUIRE(n_points >= 0 && stride >= 3, "bff_voxel_keys: bad sizes");
    BFF_LIMIT(n_points < (1ll << 31), "bff_voxel_keys: at most 2^31 - 1 points");
    if (n_points == 0) return BFF_OK;
    BFF_REQUIRE(lo_host && hi_host, "bff_voxel_keys: null pointer (the box)");
    VoxelFrame fr;
    fr.cell = cell;
    for (int a = 0; a < 3; ++a) {
        BFF_REQUIRE(std::isfinite(lo_host[a]) && std::isfinite(hi_host[a]) && lo_host[a] <= hi_host[a],
                    "bff_voxel_keys: the box must be finite and ordered");
        // subtraction, division and floor are monotonic: no point of the box has a larger q than its far corner
        const double q = cell_coord(hi_host[a], lo_host[a], cell);
        BFF_LIMIT(q < (double)kCellAxis, "bff_voxel_keys: %g cells on axis %d, at most 2^21 (a larger cell is needed)", q, a);
        fr.lo[a] = lo_host[a];
    }
    BFF_REQUIRE(points && key, "bff_voxel_keys: null pointer");
    voxel_keys_kernel<<<(unsigned)ceil_div(n_points, 256), 256, 0, as_stream(stream)>>>(points, n_points, stride, fr, key);
    return launched("bff_voxel_keys");
}

extern "C" int bff_voxel_heads(const int64_t *sorted_keys, int64_t n_points, int32_t *head, void *stream)
{
    BFF_REQUIRE(n_points >= 0, "bff_voxel_heads: bad sizes");
    BFF_LIMIT(n_points < (1ll << 31), "bff_voxel_heads: at most 2^31 - 1 points");
    if (n_points == 0) return BFF_OK;
    BFF_REQUIRE(sorted_keys && head, "bff_voxel_heads: null pointer");
    voxel_heads_kernel<<<(unsigned)ceil_div(n_points, 256), 256, 0, as_stream(stream)>>>(sorted_keys, n_points, head);
    return launched("bff_voxel_heads");
}

extern "C" int bff_voxel_ranks(const int64_t *sorted_keys, const int32_t *order, const int64_t *heads_incl, int64_t n_points,
                               int64_t n_voxels, int32_t *vox, int64_t *keys, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && n_voxels >= 0 && n_voxels <= n_points, "bff_voxel_ranks: bad sizes");
    BFF_LIMIT(n_points < (1ll << 31), "bff_voxel_ranks: at most 2^31 - 1 points");
    if (n_points == 0) return BFF_OK;
    BFF_REQUIRE(sorted_keys && order && heads_incl && vox && (keys || n_voxels == 0), "bff_voxel_ranks: null pointer");
    voxel_ranks_kernel<<<(unsigned)ceil_div(n_points, 256), 256, 0, as_stream(stream)>>>(sorted_keys, order, heads_incl, n_points,
                                                                                         n_voxels, vox, keys);
    return launched("bff_voxel_ranks");
}

extern "C" int bff_voxel_neighbours(const int64_t *keys, int64_t n_voxels, int32_t *nbr, void *stream)
{
    BFF_REQUIRE(n_voxels >= 0, "bff_voxel_neighbours: bad sizes");
    BFF_LIMIT(n_voxels < (1ll << 31), "bff_voxel_neighbours: at most 2^31 - 1 cells");
    if (n_voxels == 0) return BFF_OK;
    BFF_REQUIRE(keys && nbr, "bff_voxel_neighbours: null pointer");
    voxel_neighbours_kernel<<<(unsigned)ceil_div(n_voxels * kVoxNbr, 256), 256, 0, as_stream(stream)>>>(keys, n_voxels, nbr);
    return launched("bff_voxel_neighbours");
}

extern "C" int bff_split_occupancy(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *vox,
                                   int64_t n_voxels, uint64_t *occ, int32_t *prefix, int32_t *row_total, void *stream)
{
    int rc = split_check("bff_split_occupancy", n_rows, nw, n_points, n_voxels);
    if (rc != BFF_OK) return rc;
    if (n_rows == 0 || n_voxels == 0) return BFF_OK;
    BFF_REQUIRE(occ && prefix && row_total && (n_points == 0 || (rows && vox)), "bff_split_occupancy: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t vw = ceil_div(n_voxels, 64);
    hipError_t e = hipMemsetAsync(occ, 0, sizeof(uint64_t) * (size_t)n_rows * (size_t)vw, st);
    if (e != hipSuccess) return fail((int)e, "bff_split_occupancy: memset: %s", hipGetErrorString(e));
    if (n_points > 0) {
        split_occupancy_kernel<<<row_word_blocks(n_rows, nw), 256, 0, st>>>(rows, n_rows, nw, n_points, vox, n_voxels, vw,
                                                                            reinterpret_cast<unsigned long long *>(occ));
        rc = launched("bff_split_occupancy");
        if (rc != BFF_OK) return rc;
    }
    elements_prefix(occ, n_rows, vw, prefix, row_total, st);
    return launched("bff_split_occupancy");
}

extern "C" int bff_split_union(const uint64_t *occ, const int32_t *prefix, const int32_t *elem_offs, int32_t n_rows,
                               int64_t n_voxels, const int32_t *nbr, int32_t n_elems, int32_t *parent, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && n_voxels >= 0 && n_elems >= 0, "bff_split_union: bad sizes");
    BFF_LIMIT(n_voxels < (1ll << 31) && (int64_t)n_rows * ceil_div(n_voxels, 64) * 64 < (1ll << 31),
              "bff_split_union: rows x cells beyond 2^31 - 1 bits");
    if (n_rows == 0 || n_voxels == 0 || n_elems == 0) return BFF_OK;
    BFF_REQUIRE(occ && prefix && elem_offs && nbr && parent, "bff_split_union: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t vw = ceil_div(n_voxels, 64);
    forest_init(parent, n_elems, st);
    split_union_kernel<<<(unsigned)ceil_div((int64_t)n_rows * vw, 256), 256, 0, st>>>(occ, prefix, elem_offs, n_rows, vw, n_voxels,
                                                                                      nbr, n_elems, parent);
    forest_flatten(parent, n_elems, st);
    return launched("bff_split_union");
}

extern "C" int bff_split_count(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *vox,
                               int64_t n_voxels, const uint64_t *occ, const int32_t *prefix, const int32_t *elem_offs,
                               const int32_t *parent, int32_t n_elems, int32_t min_points, int32_t *count, int32_t *kept,
                               void *stream)
{
    int rc = split_check("bff_split_count", n_rows, nw, n_points, n_voxels);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(n_elems >= 0 && min_points >= 1, "bff_split_count: bad sizes (min_points >= 1)");
    if (n_rows == 0 || n_voxels == 0 || n_elems == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(rows && vox && occ && prefix && elem_offs && parent && count && kept, "bff_split_count: null pointer");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)n_elems, st);
    if (e == hipSuccess) e = hipMemsetAsync(kept, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return fail((int)e, "bff_split_count: memset: %s", hipGetErrorString(e));
    split_count_kernel<<<row_word_blocks(n_rows, nw), 256, 0, st>>>(rows, n_rows, nw, n_points, vox, n_voxels, occ, prefix,
                                                                    elem_offs, ceil_div(n_voxels, 64), parent, n_elems, count);
    split_compact_kernel<<<(unsigned)ceil_div(n_elems, 256), 256, 0, st>>>(parent, count, n_elems, min_points, kept);
    return launched("bff_split_count");
}

extern "C" int bff_split_emit(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *vox,
                              int64_t n_voxels, const uint64_t *occ, const int32_t *prefix, const int32_t *elem_offs,
                              const int32_t *parent, int32_t n_elems, const int32_t *table, int32_t n_out, uint64_t *out,
                              void *stream)
{
    int rc = split_check("bff_split_emit", n_rows, nw, n_points, n_voxels);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(n_elems >= 0 && n_out >= 0, "bff_split_emit: bad sizes");
    if (n_out == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(out, "bff_split_emit: null pointer");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t) * (size_t)n_out * (size_t)nw, st);
    if (e != hipSuccess) return fail((int)e, "bff_split_emit: memset: %s", hipGetErrorString(e));
    if (n_rows == 0 || n_voxels == 0 || n_elems == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(rows && vox && occ && prefix && elem_offs && parent && table, "bff_split_emit: null pointer");
    split_emit_kernel<<<row_word_blocks(n_rows, nw), 256, 0, st>>>(rows, n_rows, nw, n_points, vox, n_voxels, occ, prefix,
                                                                   elem_offs, ceil_div(n_voxels, 64), parent, n_elems, table, n_out,
                                                                   out);
    return launched("bff_split_emit");
}
