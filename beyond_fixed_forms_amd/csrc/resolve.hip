// Overlap resolution (include/bff_hip.h: a16): the ordered pair list of solve_overlapping and its one-pass closed form.
#include "common.h"

namespace bff {

// ---- row programs -----------------------------------------------------------------------------
// Sequential overlap decisions of solve_overlapping (P:285-299) on the device: inter is the K x K
// intersection matrix of the aggregated rows BEFORE any edit (P:289-292), size[i] the number of raw masks
// merged into row i; pairs are visited in the reference's order (i ascending, j > i ascending) and the
// and-not operations appended to `ops` ([0] = count, then (opcode, dst, src) triples).
constexpr int kOvlRows = 8192;   // rows whose pair counts fit the block's LDS; beyond that one thread walks the pairs

// One block: (1) wave w counts, for its rows i = w, w + 16, ..., the rows j > i with inter[i][j] > 0 (ballots over 64
// columns at a time), (2) a block-wide exclusive scan turns the counts into list offsets -- the reference visits the
// pairs in (i ascending, j ascending) order and that IS the order of (offset of i, rank of j within i), (3) the waves
// walk their rows again and write the triples.  The order of the list is the semantics (P:285-299); building it is
// embarrassingly parallel.
__global__ __launch_bounds__(1024) void overlap_ops_kernel(const int32_t *__restrict__ inter,
                                                            const int32_t *__restrict__ size, int k,
                                                            int32_t *__restrict__ ops)
{
    __shared__ int s_cnt[kOvlRows];
    __shared__ int s_wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k > kOvlRows) {                            // not a realistic size: the plain ordered loop
        if (tid) return;
        int n = 0;
        for (int i = 0; i < k; ++i)
            for (int j = i + 1; j < k; ++j)
                if (inter[(int64_t)i * k + j] > 0) {
                    const bool i_wins = size[i] > size[j];            // ties: i loses (P:296-299)
                    ops[1 + 3 * n] = 0; ops[2 + 3 * n] = i_wins ? j : i; ops[3 + 3 * n] = i_wins ? i : j;
                    ++n;
                }
        ops[0] = n;
        return;
    }
    for (int i = wave; i < k; i += 16) {
        int c = 0;
        for (int j0 = (i + 1) & ~63; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            c += __popcll(__ballot(j > i && j < k && inter[(int64_t)i * k + j] > 0));
        }
        if (lane == 0) s_cnt[i] = c;
    }
    __syncthreads();
    // exclusive scan of s_cnt[0..k) in place: thread t owns a contiguous run of ceil(k / 1024) rows
    const int per = (k + 1023) / 1024, lo = tid * per, hi = min(k, lo + per);
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += s_cnt[i];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int base = incl - mine;
    for (int q = 0; q < wave; ++q) base += s_wsum[q];
    if (tid == 1023) ops[0] = base + mine;
    for (int i = lo; i < hi; ++i) { const int c = s_cnt[i]; s_cnt[i] = base; base += c; }
    __syncthreads();
    for (int i = wave; i < k; i += 16) {
        int at = s_cnt[i];
        const int size_i = size[i];
        for (int j0 = (i + 1) & ~63; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            const bool on = j > i && j < k && inter[(int64_t)i * k + j] > 0;
            const uint64_t bal = __ballot(on);
            if (on) {
                const int n = at + __popcll(bal & ((1ull << lane) - 1));
                const bool i_wins = size_i > size[j];                 // ties: i loses (P:296-299)
                ops[1 + 3 * n] = 0;
                ops[2 + 3 * n] = i_wins ? j : i;
                ops[3 + 3 * n] = i_wins ? i : j;
            }
            at += __popcll(bal);
        }
    }
}

// solve_overlapping (P:277-301) + the point filter (P:595) + both popcounts (P:592, 596) in ONE pass, for any number
// of rows.
//
// The reference lists the pairs (i < j) that share a point BEFORE any edit and visits them in (i, j) order: the row
// merged from more raw masks keeps the current overlap, the other loses it, ties go to j (P:285-299).  Seen from ONE
// point p this is a walk over S = the rows that hold p at the start (every pair inside S shares p, so every one of
// them is on the list; rows outside S neither change at p nor change others there).  A row's bit is only ever
// cleared, and a pair with a cleared bit changes nothing, so the walk is a champion scan over S in index order: the
// first row stays until it meets a row of at least its size, which then takes its place, and so on.  Champion sizes
// never decrease and a later equal size replaces the champion, hence
//     p ends up in exactly one row of S: the one with the largest size, and among those the LARGEST index.
// With the rows ordered by that priority (size descending, index descending) the whole loop is one exclusive prefix
// OR: row r keeps  r & ~(OR of the rows ranked before it).  No pair list, no intersections, no order dependence
// between words.  (tests: against the literal ordered replay, bff_overlap_ops + bff_apply_row_ops, and the oracle.)
//
// One block = 64 word columns x 16 waves; wave s owns the ranks [s L, (s+1) L), L = ceil(k / 16): it loads its rows'
// words (independent loads, all in flight), ORs them, the 16 segment sums meet in LDS, and every row is finished with
// the OR of the segments before its own plus its own exclusive prefix.  Rows that do not change are not written.
constexpr int kResWaves = 16;
constexpr int kResolveMax = 4096;          // rows: the ranks are found by counting, k^2 / 1024 comparisons per thread

__device__ __forceinline__ uint32_t wave_sum_to_lane63(uint32_t v)
{
#define BFF_DPP_ADD(ctrl, rows) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xF, false)
    BFF_DPP_ADD(0x111, 0xF);    // row_shr:1
    BFF_DPP_ADD(0x112, 0xF);    // row_shr:2
    BFF_DPP_ADD(0x114, 0xF);    // row_shr:4
    BFF_DPP_ADD(0x118, 0xF);    // row_shr:8
    BFF_DPP_ADD(0x142, 0xA);    // row_bcast:15 -> rows 1 and 3
    BFF_DPP_ADD(0x143, 0xC);    // row_bcast:31 -> rows 2 and 3
#undef BFF_DPP_ADD
    return v;                   // lane 63 holds the sum of all 64 lanes
}

// one finished row: write it if it changed, add its popcounts before / after (<= 4096 each per wave: two 16-bit fields)
__device__ __forceinline__ void resolve_emit(uint64_t *__restrict__ dst, uint64_t v, uint64_t out, bool in, int row,
                                             int32_t *__restrict__ before, int32_t *__restrict__ after, int lane)
{
    if (in && out != v) *dst = out;
    const uint32_t pc = wave_sum_to_lane63(((uint32_t)popc64(v) << 16) | (uint32_t)popc64(out));
    if (lane == kWave - 1) {
        if (pc >> 16) atomicAdd(before + row, (int)(pc >> 16));
        if (pc & 0xffffu) atomicAdd(after + row, (int)(pc & 0xffffu));
    }
}

template <int kMaxL>
__device__ __forceinline__ void resolve_segment_in_registers(uint64_t *__restrict__ rows, int64_t nw, int64_t w, bool in,
                                                             int r0, int r1, const int *s_order, uint64_t (*s_seg)[kWave],
                                                             uint64_t kp, int32_t *__restrict__ before,
                                                             int32_t *__restrict__ after, int lane, int wave)
{
    uint64_t v[kMaxL];
#pragma unroll
    for (int q = 0; q < kMaxL; ++q)                                  // r0 + q < r1 is wave-uniform
        v[q] = (r0 + q < r1 && in) ? rows[(int64_t)s_order[r0 + q] * nw + w] : 0;
    uint64_t tot = 0;
#pragma unroll
    for (int q = 0; q < kMaxL; ++q) tot |= v[q];
    s_seg[wave][lane] = tot;
    __syncthreads();
    uint64_t claimed = 0;
    for (int s = 0; s < wave; ++s) claimed |= s_seg[s][lane];
#pragma unroll
    for (int q = 0; q < kMaxL; ++q)
        if (r0 + q < r1) {
            const int row = s_order[r0 + q];
            resolve_emit(rows + (int64_t)row * nw + w, v[q], v[q] & ~claimed & kp, in, row, before, after, lane);
            claimed |= v[q];
        }
}

__global__ __launch_bounds__(1024) void resolve_priority_kernel(uint64_t *__restrict__ rows, int64_t nw, int k,
                                                                 const int32_t *__restrict__ size,
                                                                 const uint64_t *__restrict__ keep,
                                                                 int32_t *__restrict__ before, int32_t *__restrict__ after,
                                                                 const int32_t *__restrict__ k_dev)
{
    // k_dev != NULL: the row count lives on the device (groups formed there); k is then the capacity the launch
    // was sized for and a count beyond it leaves the rows alone (the host sees the count and takes the general path)
    if (k_dev) {
        const int kd = *k_dev;
        if (kd <= 0 || kd > k) return;
        k = kd;
    }
    extern __shared__ int s_res[];                                  // [k] sizes, then [k] rows by priority
    int *s_size = s_res, *s_order = s_res + k;
    __shared__ uint64_t s_seg[kResWaves][kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    for (int r = tid; r < k; r += 1024) s_size[r] = size[r];
    __syncthreads();
    for (int r = tid; r < k; r += 1024) {
        const int sr = s_size[r];
        int rank = 0;                                                // rows that take their points before row r does
#pragma unroll 8
        for (int q = 0; q < k; ++q) {
            const int sq = s_size[q];
            rank += (sq > sr || (sq == sr && q > r)) ? 1 : 0;
        }
        s_order[rank] = r;
    }
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * kWave + lane;
    const bool in = w < nw;
    const uint64_t kp = keep ? (in ? keep[w] : 0) : ~0ull;
    const int len = (k + kResWaves - 1) / kResWaves;                 // block-uniform
    const int r0 = min(k, wave * len), r1 = min(k, r0 + len);
    if (len <= 2) {
        resolve_segment_in_registers<2>(rows, nw, w, in, r0, r1, s_order, s_seg, kp, before, after, lane, wave);
    } else if (len <= 8) {
        resolve_segment_in_registers<8>(rows, nw, w, in, r0, r1, s_order, s_seg, kp, before, after, lane, wave);
    } else if (len <= 32) {
        resolve_segment_in_registers<32>(rows, nw, w, in, r0, r1, s_order, s_seg, kp, before, after, lane, wave);
    } else {
        // more than 512 rows: two passes over the segment (the second one finds its words in the cache)
        uint64_t tot = 0;
#pragma unroll 8
        for (int r = r0; r < r1; ++r) tot |= in ? rows[(int64_t)s_order[r] * nw + w] : 0;
        s_seg[wave][lane] = tot;
        __syncthreads();
        uint64_t claimed = 0;
        for (int s = 0; s < wave; ++s) claimed |= s_seg[s][lane];
        for (int r = r0; r < r1; ++r) {
            const int row = s_order[r];
            uint64_t *dst = rows + (int64_t)row * nw + w;
            const uint64_t v = in ? *dst : 0;
            resolve_emit(dst, v, v & ~claimed & kp, in, row, before, after, lane);
            claimed |= v;
        }
    }
}

}  // namespace bff

using namespace bff;

extern "C" int bff_overlap_ops(const int32_t *inter, const int32_t *size, int32_t k, int32_t *ops, void *stream)
{
    BFF_REQUIRE(k >= 0, "bff_overlap_ops: bad size");
    BFF_REQUIRE(ops && (k == 0 || (inter && size)), "bff_overlap_ops: null pointer");
    overlap_ops_kernel<<<1, 1024, 0, as_stream(stream)>>>(inter, size, k, ops);
    return launched("bff_overlap_ops");
}

static int launch_resolve(uint64_t *rows, int k, int64_t nw, const int32_t *size, const uint64_t *keep, int32_t *before,
                          int32_t *after, const int32_t *k_dev, hipStream_t st, const char *what)
{
    hipError_t e = zero_async(before, sizeof(int32_t) * (size_t)k, st);
    if (e == hipSuccess) e = zero_async(after, sizeof(int32_t) * (size_t)k, st);
    if (e != hipSuccess) return fail((int)e, "%s: memset: %s", what, hipGetErrorString(e));
    resolve_priority_kernel<<<(unsigned)ceil_div(nw > 0 ? nw : 1, kWave), 1024, sizeof(int) * 2 * (size_t)k, st>>>(
        rows, nw, k, size, keep, before, after, k_dev);
    return launched(what);
}

extern "C" int bff_resolve_overlaps(uint64_t *rows, int32_t k, int64_t nw, const int32_t *size, const uint64_t *keep,
                                    int32_t *before, int32_t *after, void *stream)
{
    BFF_REQUIRE(k >= 0 && nw >= 0, "bff_resolve_overlaps: bad sizes");
    BFF_LIMIT(k <= kResolveMax, "bff_resolve_overlaps: more than %d rows (use bff_overlap_ops + bff_apply_row_ops)", kResolveMax);
    if (k == 0) return BFF_OK;
    BFF_REQUIRE(rows && size && before && after, "bff_resolve_overlaps: null pointer");
    return launch_resolve(rows, k, nw, size, keep, before, after, nullptr, as_stream(stream), "bff_resolve_overlaps");
}

extern "C" int bff_resolve_overlaps_dev(uint64_t *rows, int32_t k_cap, int64_t nw, const int32_t *size, const uint64_t *keep,
                                        int32_t *before, int32_t *after, const int32_t *k_dev, void *stream)
{
    BFF_REQUIRE(k_cap > 0 && nw >= 0, "bff_resolve_overlaps_dev: bad sizes");
    BFF_LIMIT(k_cap <= kResolveMax, "bff_resolve_overlaps_dev: capacity beyond %d rows", kResolveMax);
    BFF_REQUIRE(rows && size && before && after && k_dev, "bff_resolve_overlaps_dev: null pointer");
    return launch_resolve(rows, k_cap, nw, size, keep, before, after, k_dev, as_stream(stream), "bff_resolve_overlaps_dev");
}

extern "C" int bff_resolve_overlaps_max_rows(void) { return kResolveMax; }
