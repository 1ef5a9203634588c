// 3-D instances snapped to superpoints (include/bff_hip.h: bff_spp_*).  An instance is a bit row
// over the cloud; a superpoint that holds enough of a row's points goes to the row whole.  The work follows the set
// bits of the rows in the caller's point order: nothing is permuted into superpoint order.
//
// Data layout in HBM
//   rows     u64 [K][nw]            the instances; bits at positions >= N are ignored
//   seg      i32 [N]                the superpoint of every point, -1 = none (read coalesced: lane = point)
//   count    i32 [K][S]             points of row k in superpoint s (read coalesced: lane = superpoint)
//   need     i32 [S]                points a row must hold of superpoint s to take it
//   owner    i32 [S]                "exclusive" mode: the one row that takes superpoint s, -1 = none
//   order    i32 [N']               the points with a superpoint, by (superpoint, point); offs i32 [S + 1] into it
//   out      u64 [K][nw]            rows & free on entry, the snapped rows on return
// Integer atomics only (add, or): every result is the same on every run.
#include "rows.h"

namespace bff {

constexpr int kSppWaves = 4;                                       // waves per block of the count and fill kernels

// One wave per 64 consecutive words of a row: the lanes read a word each, the wave takes the non-zero ones one at a
// time with lane = bit, so a zero word costs nothing beyond its share of that one read.
__global__ __launch_bounds__(kSppWaves * kWave) void spp_count_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                                       int64_t n_points, int64_t groups_per_row,
                                                                       const int32_t *__restrict__ seg, int64_t n_segments,
                                                                       int32_t *__restrict__ count)
{
    const int64_t g = (int64_t)blockIdx.x * kSppWaves + (threadIdx.x >> 6);
    if (g >= (int64_t)n_rows * groups_per_row) return;             // wave-uniform
    const int k = (int)(g / groups_per_row), lane = lane_id();
    const int64_t w0 = (g % groups_per_row) * kWave;
    const int64_t w = w0 + lane;
    const uint64_t mine = w * 64 < n_points ? rows[(int64_t)k * nw + w] : 0;       // w * 64 < N implies w < nw
    uint64_t todo = __ballot(mine != 0);
    int32_t *row_count = count + (int64_t)k * n_segments;
    while (todo) {                                                  // wave-uniform
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t word = __shfl(mine, src);
        const int64_t p = (w0 + src) * 64 + lane;
        // one atomic per set lane: merging the lanes of a word that share a superpoint first was measured and took
        // 1.8 times as long on generator rows
        if (p < n_points && ((word >> lane) & 1)) {                 // bits at positions >= N are ignored
            const int32_t s = seg[p];
            if (s >= 0 && s < n_segments) atomicAdd(row_count + s, 1);          // result unused: returnless
        }
    }
}

// one thread per superpoint walks the rows: the largest count that reaches need, the first row that holds it
__global__ __launch_bounds__(256) void spp_owner_kernel(const int32_t *__restrict__ count, int n_rows, int64_t n_segments,
                                                         const int32_t *__restrict__ need, int32_t *__restrict__ owner)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_segments) return;
    const int32_t least = need[s] > 1 ? need[s] : 1;
    int32_t best = -1, held = least - 1;
    for (int k = 0; k < n_rows; ++k) {
        const int32_t c = count[(int64_t)k * n_segments + s];
        if (c > held) held = c, best = k;
    }
    owner[s] = best;
}

// One wave per 64 consecutive superpoints of a row: the lanes decide a superpoint each, the wave takes the chosen ones
// one at a time and strides over that superpoint's points, so a floor of many thousands of points is spread over 64 lanes.
__global__ __launch_bounds__(kSppWaves * kWave) void spp_fill_kernel(const int32_t *__restrict__ count, int n_rows,
                                                                      int64_t n_segments, int64_t groups_per_row,
                                                                      const int32_t *__restrict__ need,
                                                                      const int32_t *__restrict__ owner,
                                                                      const int32_t *__restrict__ order,
                                                                      const int32_t *__restrict__ offs,
                                                                      unsigned long long *__restrict__ out, int64_t nw)
{
    const int64_t g = (int64_t)blockIdx.x * kSppWaves + (threadIdx.x >> 6);
    if (g >= (int64_t)n_rows * groups_per_row) return;             // wave-uniform
    const int k = (int)(g / groups_per_row), lane = lane_id();
    const int64_t s = (g % groups_per_row) * kWave + lane;
    bool take = false;
    int32_t first = 0, last = 0;
    if (s < n_segments) {
        if (owner) {
            take = owner[s] == k;
        } else {
            const int32_t least = need[s] > 1 ? need[s] : 1;
            take = count[(int64_t)k * n_segments + s] >= least;
        }
        if (take) first = offs[s], last = offs[s + 1];
    }
    uint64_t todo = __ballot(take && first >= 0);
    unsigned long long *row = out + (int64_t)k * nw;
    const uint64_t bits = (uint64_t)nw * 64;
    while (todo) {                                                  // wave-uniform
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t a = __shfl(first, src), b = __shfl(last, src);
        for (int64_t i = a + lane; i < b; i += kWave) {
            const int32_t p = order[i];
            if ((uint64_t)(int64_t)p < bits) atomicOr(row + (p >> 6), 1ull << (p & 63));      // result unused: returnless
        }
    }
}

static int spp_sizes(const char *what, int32_t n_rows, int64_t n_segments)
{
    BFF_REQUIRE(n_rows >= 0 && n_segments >= 0, "%s: bad sizes (n_rows, n_segments)", what);
    BFF_LIMIT(n_segments < (1ll << 31), "%s: n_segments: at most 2^31 - 1 superpoints", what);
    BFF_LIMIT((int64_t)n_rows * n_segments < (1ll << 31), "%s: n_rows x n_segments = %lld x %lld, at most 2^31 - 1 counts", what,
              (long long)n_rows, (long long)n_segments);
    return BFF_OK;
}

}  // namespace bff

using namespace bff;

extern "C" int bff_spp_count(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *seg,
                             int64_t n_segments, int32_t *count, void *stream)
{
    BFF_REQUIRE(nw >= 0 && n_points >= 0, "bff_spp_count: bad sizes (nw, n_points)");
    int rc = spp_sizes("bff_spp_count", n_rows, n_segments);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(nw >= ceil_div(n_points, 64), "bff_spp_count: nw: rows of %lld words for %lld points", (long long)nw,
                (long long)n_points);
    BFF_LIMIT(n_points < (1ll << 31), "bff_spp_count: n_points: at most 2^31 - 1 points");
    if (n_rows == 0 || n_segments == 0) return BFF_OK;
    BFF_REQUIRE(count, "bff_spp_count: null pointer (count)");
    BFF_REQUIRE(n_points == 0 || rows, "bff_spp_count: null pointer (rows)");
    BFF_REQUIRE(n_points == 0 || seg, "bff_spp_count: null pointer (seg)");
    const int64_t groups = ceil_div(ceil_div(n_points, 64), kWave);
    BFF_LIMIT(ceil_div((int64_t)n_rows * groups, kSppWaves) < (1ll << 31), "bff_spp_count: too many row words for one launch");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)n_rows * (size_t)n_segments, st);
    if (e != hipSuccess) return fail((int)e, "bff_spp_count: memset: %s", hipGetErrorString(e));
    if (n_points == 0) return BFF_OK;
    spp_count_kernel<<<(unsigned)ceil_div((int64_t)n_rows * groups, kSppWaves), kSppWaves * kWave, 0, st>>>(
        rows, n_rows, nw, n_points, groups, seg, n_segments, count);
    return launched("bff_spp_count");
}

extern "C" int bff_spp_owner(const int32_t *count, int32_t n_rows, int64_t n_segments, const int32_t *need, int32_t *owner,
                             void *stream)
{
    int rc = spp_sizes("bff_spp_owner", n_rows, n_segments);
    if (rc != BFF_OK) return rc;
    if (n_segments == 0) return BFF_OK;
    BFF_REQUIRE(owner, "bff_spp_owner: null pointer (owner)");
    BFF_REQUIRE(n_rows == 0 || count, "bff_spp_owner: null pointer (count)");
    BFF_REQUIRE(need, "bff_spp_owner: null pointer (need)");
    spp_owner_kernel<<<(unsigned)ceil_div(n_segments, 256), 256, 0, as_stream(stream)>>>(count, n_rows, n_segments, need, owner);
    return launched("bff_spp_owner");
}

extern "C" int bff_spp_fill(const int32_t *count, int32_t n_rows, int64_t n_segments, const int32_t *need, const int32_t *owner,
                            const int32_t *order, const int32_t *offs, uint64_t *out, int64_t nw, void *stream)
{
    BFF_REQUIRE(nw >= 0, "bff_spp_fill: bad sizes (nw)");
    int rc = spp_sizes("bff_spp_fill", n_rows, n_segments);
    if (rc != BFF_OK) return rc;
    if (n_rows == 0 || n_segments == 0 || nw == 0) return BFF_OK;
    BFF_REQUIRE(out, "bff_spp_fill: null pointer (out)");
    BFF_REQUIRE(owner || (count && need), "bff_spp_fill: null pointer (count and need, or owner)");
    BFF_REQUIRE(order && offs, "bff_spp_fill: null pointer (order, offs)");
    const int64_t groups = ceil_div(n_segments, kWave);
    spp_fill_kernel<<<(unsigned)ceil_div((int64_t)n_rows * groups, kSppWaves), kSppWaves * kWave, 0, as_stream(stream)>>>(
        count, n_rows, n_segments, groups, need, owner, order, offs, reinterpret_cast<unsigned long long *>(out), nw);
    return launched("bff_spp_fill");
}
