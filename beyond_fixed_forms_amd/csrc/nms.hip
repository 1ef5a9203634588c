// 3-D mask NMS over ranked bit rows (include/bff_hip.h: bff_nms_pairs, bff_nms_greedy).
#include "common.h"

namespace bff {

constexpr int kNmsMax = 4096;      // rows: bff_resolve_overlaps_max_rows(); the removed set is one word per lane of one wave
constexpr int kNmsAhead = 16;      // rows of sup in one register ring: a row is requested 16 to 32 ranks before its turn

// ---- which rank hits which ----------------------------------------------------------------------------------------
// One wave per word of sup: lane l tests the pair (rank r, rank s = 64 sw + l), the ballot is the word and lane 0 stores
// it -- no atomics.  A word that lies wholly at or below the diagonal is zero without a load.  Both overlap values are
// one float32 division of exactly converted integers (areas < 2^23, so the union is < 2^24), and the test is the
// reference's keep-test `v < thres` negated, in float32.
__global__ __launch_bounds__(256) void nms_pairs_kernel(const int32_t *__restrict__ inter, const int32_t *__restrict__ area,
                                                        const int32_t *__restrict__ order, const int32_t *__restrict__ cls,
                                                        int k, int criterion, float thres, uint64_t *__restrict__ sup)
{
    const int w = (k + kWave - 1) / kWave, lane = lane_id();
    const int64_t word = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);           // wave-uniform
    if (word >= (int64_t)k * w) return;
    const int r = (int)(word / w), sw = (int)(word % w);
    uint64_t bits = 0;
    if (sw * kWave + kWave - 1 > r) {
        const int s = sw * kWave + lane;
        bool hit = false;
        if (s > r && s < k) {
            const int i = order[r], j = order[s];
            if ((unsigned)i < (unsigned)k && (unsigned)j < (unsigned)k) {        // an order that is no permutation hits nothing
                const int both = inter[(int64_t)i * k + j], ai = area[i], aj = area[j];
                const float den = criterion == BFF_NMS_IOU ? (float)(ai + aj - both) : (float)min(ai, aj);
                const float v = (float)both / den;
                hit = !(v < thres) && (!cls || cls[i] == cls[j]);
            }
        }
        bits = __ballot(hit);
    }
    if (lane == 0) sup[word] = bits;
}

// ---- the greedy chain ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t read_lane_u64(uint64_t v, int l)             // l wave-uniform: two v_readlane
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// One wave; lane l owns word l of `removed` (k <= 4096 = 64 words) and of the keep bits.  In rank order: rank r is kept iff
// its bit of `removed` is clear, and a kept rank ORs its row of sup into `removed`.  The decision is serial in r, the rows of
// sup are not: two register rings of kNmsAhead rows take turns, and the loads that refill one are issued before the ranks
// of the other are decided, so a row is requested kNmsAhead to 2 kNmsAhead ranks before its turn and nothing is copied
// (row indices past the end are clamped: every load is unconditional and in bounds).  The bit of rank r is read from lane
// r >> 6 with a wave-uniform lane index; the branch on it is scalar.
__device__ __forceinline__ void nms_load_rows(uint64_t (&ring)[kNmsAhead], const uint64_t *__restrict__ col, int r0, int k, int w)
{
#pragma unroll
    for (int q = 0; q < kNmsAhead; ++q) ring[q] = col[(int64_t)min(r0 + q, k - 1) * w];
}

__device__ __forceinline__ void nms_decide_rows(const uint64_t (&ring)[kNmsAhead], int r0, int k, bool mine, int lane,
                                                uint64_t &removed, uint64_t &kept)
{
#pragma unroll
    for (int q = 0; q < kNmsAhead; ++q) {
        const int r = r0 + q;                                                     // wave-uniform
        if (r < k) {
            const bool gone = (read_lane_u64(removed, r >> 6) >> (r & 63)) & 1;
            if (!gone) {
                removed |= mine ? ring[q] : 0;
                if (lane == (r >> 6)) kept |= 1ull << (r & 63);
            }
        }
    }
}

__global__ __launch_bounds__(kWave) void nms_greedy_kernel(const uint64_t *__restrict__ sup, int k,
                                                           uint64_t *__restrict__ keep_bits, int32_t *__restrict__ n_kept)
{
    const int lane = threadIdx.x, w = (k + kWave - 1) / kWave;
    const bool mine = lane < w;
    const uint64_t *col = sup + (mine ? lane : 0);
    uint64_t removed = 0, kept = 0;
    uint64_t even[kNmsAhead], odd[kNmsAhead];
    nms_load_rows(even, col, 0, k, w);
    for (int r0 = 0; r0 < k; r0 += 2 * kNmsAhead) {
        nms_load_rows(odd, col, r0 + kNmsAhead, k, w);
        nms_decide_rows(even, r0, k, mine, lane, removed, kept);
        nms_load_rows(even, col, r0 + 2 * kNmsAhead, k, w);
        nms_decide_rows(odd, r0 + kNmsAhead, k, mine, lane, removed, kept);
    }
    if (mine) keep_bits[lane] = kept;
    int n = popc64(kept);
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) n += __shfl_down(n, d);
    if (lane == 0) *n_kept = n;
}

// by[s] = the smallest kept rank that hits s, -1 for a kept s.  One wave per 64 ranks s (word sw of every row of sup).
// Per 64 ranks r (wq = 0 .. sw), lane l loads row 64 wq + l's word sw if that rank is kept, the next block's word already
// in flight; then one ballot per rank s that still waits for its keeper: the lowest lane with bit s set is the
// smallest r of the block, and blocks come in ascending order.  A removed rank has a kept rank that hits it by
// construction, so the walk ends early; kept ranks cost nothing.
__global__ __launch_bounds__(kWave) void nms_by_kernel(const uint64_t *__restrict__ sup, int k,
                                                       const uint64_t *__restrict__ keep_bits, int32_t *__restrict__ by)
{
    const int sw = blockIdx.x, lane = threadIdx.x, w = (k + kWave - 1) / kWave;
    const int left = k - sw * kWave;
    const uint64_t valid = left >= kWave ? ~0ull : (1ull << left) - 1;
    uint64_t pending = ~read_lane_u64(keep_bits[sw], 0) & valid;                  // wave-uniform: one bit per removed s
    int found = -1;
    auto fetch = [&](int wq) -> uint64_t {
        const int r = wq * kWave + lane;
        const bool on = wq <= sw && r < k && ((keep_bits[wq] >> lane) & 1);
        return on ? sup[(int64_t)r * w + sw] : 0;
    };
    uint64_t t = fetch(0);
    for (int wq = 0; wq <= sw && pending; ++wq) {
        const uint64_t t_next = fetch(wq + 1);
        for (uint64_t it = pending; it; it &= it - 1) {
            const int sb = __builtin_ctzll(it);
            const uint64_t b = __ballot((t >> sb) & 1);
            if (b) {
                if (lane == sb) found = wq * kWave + __builtin_ctzll(b);
                pending &= ~(1ull << sb);
            }
        }
        t = t_next;
    }
    if (lane < left) by[sw * kWave + lane] = found;
}

}  // namespace bff

using namespace bff;

extern "C" int bff_nms_pairs(const int32_t *inter, const int32_t *area, const int32_t *order, const int32_t *cls, int32_t k,
                             int32_t criterion, float thres, uint64_t *sup, void *stream)
{
    BFF_REQUIRE(k >= 0, "bff_nms_pairs: bad size");
    BFF_REQUIRE(criterion == BFF_NMS_IOU || criterion == BFF_NMS_CONTAINMENT, "bff_nms_pairs: unknown criterion %d", criterion);
    BFF_REQUIRE(thres == thres, "bff_nms_pairs: the threshold is NaN");
    BFF_LIMIT(k <= kNmsMax, "bff_nms_pairs: %d rows, more than %d", k, kNmsMax);
    if (k == 0) return BFF_OK;
    BFF_REQUIRE(inter && area && order && sup, "bff_nms_pairs: null pointer");
    const int64_t words = (int64_t)k * ceil_div(k, kWave);
    nms_pairs_kernel<<<(unsigned)ceil_div(words, 4), 256, 0, as_stream(stream)>>>(inter, area, order, cls, k, criterion, thres, sup);
    return launched("bff_nms_pairs");
}

extern "C" int bff_nms_greedy(const uint64_t *sup, int32_t k, uint64_t *keep_bits, int32_t *by, int32_t *n_kept, void *stream)
{
    BFF_REQUIRE(k >= 0, "bff_nms_greedy: bad size");
    BFF_LIMIT(k <= kNmsMax, "bff_nms_greedy: %d rows, more than %d", k, kNmsMax);
    if (k == 0) return BFF_OK;
    BFF_REQUIRE(sup && keep_bits && by && n_kept, "bff_nms_greedy: null pointer");
    nms_greedy_kernel<<<1, kWave, 0, as_stream(stream)>>>(sup, k, keep_bits, n_kept);
    nms_by_kernel<<<(unsigned)ceil_div(k, kWave), kWave, 0, as_stream(stream)>>>(sup, k, keep_bits, by);
    return launched("bff_nms_greedy");
}
