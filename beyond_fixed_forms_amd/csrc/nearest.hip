// 3-D instances lifted from a subsampled cloud to the full cloud (include/bff_hip.h: bff_nn_search, bff_rows_to_columns,
// bff_lift_bits).  A nearest-neighbour search on the voxel grid of section 7g, and a many-row bit
// gather that takes "no source" for an answer.  The walk over a query's 27 cells is cells.h's, shared with density.hip.
//
// Data layout in HBM
//   src      f64 [M'][3]            the source points that have a cell, gathered into (cell, point index) order: the
//                                   candidates of a cell are contiguous
//   order    i32 [M']               the source index of every gathered point;  offs i32 [V + 1]: cell v is [offs[v], offs[v + 1])
//   keys     i64 [V]                the distinct cell keys q0 + (q1 << 21) + (q2 << 42), ascending (L2 resident: 8 V bytes)
//   queries  f64 [N][stride >= 3]   the query points (x, y, z first)
//   nn       i32 [N]                the nearest source within r, -1 = none;  d2 f64 [N]: its squared distance, +inf = none
//   rows_in  u64 [K][nw_in]         bit rows over the M source points; bits at positions >= M are ignored
//   cols     u64 [M][kw]            kw = ceil(K / 64): bit k of cols[s] = bit s of row k (the rows transposed)
//   rows_out u64 [K][ceil(N / 64)]  bit p of row k = bit nn[p] of input row k, 0 where nn[p] is not in [0, M)
// No atomics, no LDS: every output word has one writer and every result is the same on every run.
#include "cells.h"

namespace bff {

constexpr int kLiftWaves = 4;                                      // waves per block of the transpose and the gather

// One lane per query: the nearest of its candidates (cells.h: for_candidates) within the radius.
__global__ __launch_bounds__(256) void nn_search_kernel(CellIndex ix, double r2, const double *__restrict__ queries, int64_t n,
                                                         int64_t stride, int32_t *__restrict__ nn, double *__restrict__ d2_out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x[3] = {queries[p * stride], queries[p * stride + 1], queries[p * stride + 2]};
    double best = INFINITY;
    int32_t best_s = -1;
    for_candidates(ix, x, [&](int64_t i) {
        const double dx = x[0] - ix.cloud[i * 3], dy = x[1] - ix.cloud[i * 3 + 1], dz = x[2] - ix.cloud[i * 3 + 2];
        const double d = (dx * dx + dy * dy) + dz * dz;              // every operation rounded: -ffp-contract=off
        if (d <= r2) {
            const int32_t s = ix.order[i];
            // the nine ranges are not in index order: the tie goes to the smallest index explicitly
            if (d < best || (d == best && (best_s < 0 || s < best_s))) best = d, best_s = s;
        }
        return false;
    });
    nn[p] = best_s;
    if (d2_out) d2_out[p] = best;
}

// One wave per 64 x 64 bit block: lane l reads word wb of row kb * 64 + l, 64 ballots turn the block, lane j writes
// word kb of source point wb * 64 + j.
__global__ __launch_bounds__(kLiftWaves * kWave) void rows_to_columns_kernel(const uint64_t *__restrict__ rows, int64_t n_rows,
                                                                              int64_t nw_in, int64_t n_source, int64_t kw,
                                                                              int64_t n_blocks, uint64_t *__restrict__ cols)
{
    const int64_t g = (int64_t)blockIdx.x * kLiftWaves + (threadIdx.x >> 6);
    if (g >= n_blocks) return;                                      // wave-uniform
    const int64_t wb = g / kw, kb = g % kw;
    const int lane = lane_id();
    const int64_t k = kb * 64 + lane;
    const uint64_t word = k < n_rows ? rows[k * nw_in + wb] : 0;    // wb < ceil(M / 64) <= nw_in
    uint64_t mine = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
        const uint64_t col = __ballot((word >> j) & 1);
        if (lane == j) mine = col;
    }
    const int64_t s = wb * 64 + lane;
    if (s < n_source) cols[s * kw + kb] = mine;                     // bits at positions >= M are ignored: never written
}

// One wave per 64 consecutive targets: every lane follows its own nn into the column words, row k's output word is one
// ballot of bit k, and lane j stores the word of row kb * 64 + j.
__global__ __launch_bounds__(kLiftWaves * kWave) void lift_bits_kernel(const uint64_t *__restrict__ cols, int64_t n_source,
                                                                        int64_t n_rows, int64_t kw,
                                                                        const int32_t *__restrict__ nn, int64_t n_target,
                                                                        int64_t nw_out, uint64_t *__restrict__ out)
{
    const int64_t w = (int64_t)blockIdx.x * kLiftWaves + (threadIdx.x >> 6);
    if (w >= nw_out) return;                                        // wave-uniform
    const int lane = lane_id();
    const int64_t p = w * 64 + lane;
    const int64_t s = p < n_target ? (int64_t)nn[p] : -1;
    const bool has = s >= 0 && s < n_source;                        // -1 and anything out of range: never followed
    for (int64_t kb = 0; kb < kw; ++kb) {
        const uint64_t col = has ? cols[s * kw + kb] : 0;
        const int64_t left = n_rows - kb * 64;
        const int here = left < 64 ? (int)left : 64;                // wave-uniform
        uint64_t mine = 0;
        for (int j = 0; j < here; ++j) {
            const uint64_t word = __ballot((col >> j) & 1);
            if (lane == j) mine = word;
        }
        if (lane < here) out[(kb * 64 + lane) * nw_out + w] = mine;
    }
}

}  // namespace bff

using namespace bff;

extern "C" int bff_nn_search(const double *src, const int64_t *keys, const int32_t *offs, const int32_t *order,
                             int64_t n_voxels, int64_t n_source, const double *lo_host, double cell, double radius,
                             const double *queries, int64_t n_queries, int64_t stride, int32_t *nn, double *d2,
                             void *stream)
{
    BFF_REQUIRE(n_voxels >= 0 && n_source >= 0 && n_queries >= 0, "bff_nn_search: bad sizes (n_voxels, n_source, n_queries)");
    BFF_REQUIRE(stride >= 3, "bff_nn_search: stride: at least 3 doubles per query");
    BFF_REQUIRE(cell > 0.0 && std::isfinite(cell), "bff_nn_search: cell must be a finite number > 0");
    BFF_REQUIRE(radius > 0.0 && std::isfinite(radius), "bff_nn_search: radius must be a finite number > 0");
    BFF_REQUIRE(n_voxels <= n_source, "bff_nn_search: n_voxels: %lld cells for %lld source points", (long long)n_voxels,
                (long long)n_source);
    BFF_LIMIT(n_queries < (1ll << 31) && n_source < (1ll << 31) && n_voxels < (1ll << 31),
              "bff_nn_search: n_queries, n_source, n_voxels: at most 2^31 - 1 each");
    if (n_queries == 0) return BFF_OK;
    BFF_REQUIRE(queries, "bff_nn_search: null pointer (queries)");
    BFF_REQUIRE(nn, "bff_nn_search: null pointer (nn)");
    CellIndex ix;
    const int rc = cell_index("bff_nn_search", src, keys, offs, order, n_voxels, n_source, lo_host, cell, ix);
    if (rc != BFF_OK) return rc;
    nn_search_kernel<<<(unsigned)ceil_div(n_queries, 256), 256, 0, as_stream(stream)>>>(ix, radius * radius, queries, n_queries,
                                                                                       stride, nn, d2);
    return launched("bff_nn_search");
}

static int lift_sizes(const char *what, int64_t n_rows, int64_t n_source)
{
    BFF_REQUIRE(n_rows >= 0 && n_source >= 0, "%s: bad sizes (n_rows, n_source)", what);
    BFF_LIMIT(n_source < (1ll << 31), "%s: n_source: at most 2^31 - 1 points", what);
    BFF_LIMIT(n_source * ceil_div(n_rows, 64) < (1ll << 31), "%s: n_source x ceil(n_rows / 64) = %lld x %lld, at most 2^31 - 1 words",
              what, (long long)n_source, (long long)ceil_div(n_rows, 64));
    return BFF_OK;
}

extern "C" int bff_rows_to_columns(const uint64_t *rows_in, int32_t n_rows, int64_t nw_in, int64_t n_source, uint64_t *cols,
                                   void *stream)
{
    BFF_REQUIRE(nw_in >= 0, "bff_rows_to_columns: bad sizes (nw_in)");
    int rc = lift_sizes("bff_rows_to_columns", n_rows, n_source);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(nw_in >= ceil_div(n_source, 64), "bff_rows_to_columns: nw_in: rows of %lld words for %lld points", (long long)nw_in,
                (long long)n_source);
    if (n_rows == 0 || n_source == 0) return BFF_OK;
    BFF_REQUIRE(rows_in, "bff_rows_to_columns: null pointer (rows_in)");
    BFF_REQUIRE(cols, "bff_rows_to_columns: null pointer (cols)");
    const int64_t kw = ceil_div(n_rows, 64), n_blocks = ceil_div(n_source, 64) * kw;      // <= M * kw < 2^31
    rows_to_columns_kernel<<<(unsigned)ceil_div(n_blocks, kLiftWaves), kLiftWaves * kWave, 0, as_stream(stream)>>>(
        rows_in, n_rows, nw_in, n_source, kw, n_blocks, cols);
    return launched("bff_rows_to_columns");
}

extern "C" int bff_lift_bits(const uint64_t *cols, int64_t n_source, int32_t n_rows, const int32_t *nn, int64_t n_target,
                             uint64_t *rows_out, void *stream)
{
    BFF_REQUIRE(n_target >= 0, "bff_lift_bits: bad sizes (n_target)");
    int rc = lift_sizes("bff_lift_bits", n_rows, n_source);
    if (rc != BFF_OK) return rc;
    BFF_LIMIT(n_target < (1ll << 31), "bff_lift_bits: n_target: at most 2^31 - 1 points");
    const int64_t nw_out = ceil_div(n_target, 64);
    BFF_LIMIT((int64_t)n_rows * nw_out < (1ll << 31), "bff_lift_bits: n_rows x ceil(n_target / 64) = %lld x %lld, at most 2^31 - 1 words",
              (long long)n_rows, (long long)nw_out);
    if (n_rows == 0 || n_target == 0) return BFF_OK;
    BFF_REQUIRE(rows_out, "bff_lift_bits: null pointer (rows_out)");
    BFF_REQUIRE(nn, "bff_lift_bits: null pointer (nn)");
    BFF_REQUIRE(n_source == 0 || cols, "bff_lift_bits: null pointer (cols)");
    lift_bits_kernel<<<(unsigned)ceil_div(nw_out, kLiftWaves), kLiftWaves * kWave, 0, as_stream(stream)>>>(
        cols, n_source, n_rows, ceil_div(n_rows, 64), nn, n_target, nw_out, rows_out);
    return launched("bff_lift_bits");
}
