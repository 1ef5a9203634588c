// The run-major cached sweep (bff_project_views_runs) and the pixel-sorted companion of the visibility table it walks
// (bff_visibility_sorted).
#include <algorithm>
#include <cstdlib>

#include <hip/hip_ext.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "sweep.h"

namespace bff {

// ---------------------------------------------------------------------------------------------
// Pixel-sorted companion of the visibility table (bff_visibility_sorted): the visible pairs of every slot ordered by
// (flat pixel, point), so that a run [start, end) of a 2-D mask covers one contiguous range of the slot's list.
//   spix      [pairs]            flat pixel v * W + u
//   spt       [pairs]            point index
//   rowstart  [n_slots][H + 1]   absolute position of the slot's first pair with pixel >= y * W; entry H = the slot's end
// Built by a stable radix sort of the pairs (they arrive in (slot, point) order) on the key slot * H * W + pixel.

// step 1: keys and points of the pairs; one wave per (slot, word), as vis_pixels_kernel
__global__ __launch_bounds__(kBlock) void vis_sort_keys_kernel(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ off,
                                                               const uint32_t *__restrict__ pix, int64_t stride, int64_t n_pairs,
                                                               int W, uint32_t hw, uint32_t *__restrict__ keys,
                                                               uint32_t *__restrict__ pts)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int slot = blockIdx.y;
    if (w >= stride) return;
    const uint64_t m = mask[slot * stride + w];
    if (!((m >> lane) & 1)) return;
    const int64_t at = (int64_t)off[slot * stride + w] + __popcll(m & ((1ull << lane) - 1));
    if (at >= n_pairs) return;
    const uint32_t p = pix[at];
    keys[at] = (uint32_t)slot * hw + (p >> 16) * (uint32_t)W + (p & 0xffffu);
    pts[at] = (uint32_t)(w * kWave + lane);
}

// step 3: the sorted keys without their slot
__global__ __launch_bounds__(kBlock) void vis_sorted_pixels_kernel(const uint32_t *__restrict__ keys, int64_t n_pairs, uint32_t hw,
                                                                   uint32_t *__restrict__ spix)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_pairs) spix[i] = keys[i] % hw;
}

// step 4: one thread per (slot, image row): lower bound of the row's first pixel inside the slot's part of the list
__global__ __launch_bounds__(kBlock) void vis_rowstart_kernel(const uint32_t *__restrict__ spix, const uint32_t *__restrict__ off,
                                                              int64_t stride, int64_t n_pairs, int n_slots, int H, int W,
                                                              uint32_t *__restrict__ rowstart)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)n_slots * (H + 1)) return;
    const int s = (int)(t / (H + 1)), y = (int)(t - (int64_t)s * (H + 1));
    int64_t lo = min((int64_t)off[s * stride], n_pairs);
    int64_t hi = s + 1 < n_slots ? min((int64_t)off[(s + 1) * stride], n_pairs) : n_pairs;
    const uint32_t target = (uint32_t)y * (uint32_t)W;          // y == H: behind every pixel
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (spix[mid] < target) lo = mid + 1; else hi = mid;
    }
    rowstart[t] = (uint32_t)lo;
}

// ---------------------------------------------------------------------------------------------
// Run-major cached sweep (bff_project_views_runs).  The point-major kVis sweep asks, per visible (point, frame) pair, which
// masks of the frame cover the pixel; here every run of every mask asks which visible pairs of its frame's slot it covers:
// with the slot's pairs sorted by flat pixel that is one contiguous range of the list, found by a lower bound inside the
// image row of the run's first pixel and one inside the row of its last.  One workgroup owns one instance row = mask m of
// frame f: it ORs the covered points into a bitmap of the row in LDS (LDS atomics), then stores the bitmap's non-zero 32-B
// sectors and the row's chunk flags with plain stores -- nobody else writes the row or its flag words.
constexpr int kRunsDeal = 4;                     // pairs a lane has in flight when the wave deals its runs' pairs out

__global__ __launch_bounds__(kBlock) void sweep_runs_fill_kernel(
    int n_frames, const int32_t *__restrict__ depth_index, int H, int W,
    const uint32_t *__restrict__ spix, const uint32_t *__restrict__ spt, const uint32_t *__restrict__ rowstart,
    const int32_t *__restrict__ run_start, const int32_t *__restrict__ run_end, const int32_t *__restrict__ mask_run_offs,
    const int32_t *__restrict__ view_mask_offs, const int32_t *__restrict__ frame_mask,
    const int32_t *__restrict__ frame_rowbase, const int32_t *__restrict__ frame_nmask,
    uint64_t *__restrict__ rows, int64_t nw, int n_chunks, uint64_t *__restrict__ chunk_mask, int mw)
{
    extern __shared__ uint64_t s_row[];                    // n_chunks * kCW words: the row, padded to whole chunks
    const int f = blockIdx.x, m = blockIdx.y;
    const int mi = frame_mask[f];
    if (mi < 0 || m >= frame_nmask[f]) return;             // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)frame_rowbase[f] + m;
    for (int i = tid; i < n_chunks * kCW; i += kBlock) s_row[i] = 0;
    __syncthreads();

    const int g = view_mask_offs[mi] + m;
    const int r0 = mask_run_offs[g], r1 = mask_run_offs[g + 1];
    const uint32_t *rs = rowstart + (int64_t)depth_index[f] * (H + 1);
    const int hw = H * W;
    uint32_t *bits = reinterpret_cast<uint32_t *>(s_row);  // little endian: bit n & 31 of 32-bit word n >> 5
    // A wave takes 64 consecutive runs (consecutive image rows of the mask, as a rule): lane l finds the list range
    // [lo, hi) its run covers -- two lower bounds, each inside one image row's segment; a run that crosses a row end needs
    // nothing special, the list is sorted by flat pixel.  The wave then deals the covered pairs of all 64 runs evenly
    // to its lanes: pair k belongs to the first lane whose inclusive count prefix exceeds k (a search over the wave by
    // shuffles), so neighbouring lanes read neighbouring entries of vis_spt whatever the runs' lengths are.
    for (int rb = r0 + wave * kWave; rb < r1; rb += kBlock) {          // wave-uniform
        const int r = rb + lane;
        uint32_t lo = 0, cnt = 0;
        if (r < r1) {
            const int start = max(run_start[r], 0), end = min(run_end[r], hw);
            if (start < end) {
                // first pair at or behind `start` in the row of the run's first pixel, first pair at or behind `end` in the
                // row of its last: two lower bounds, searched in step so that their loads travel together
                const int y = start / W, ye = (end - 1) / W;
                uint32_t lo1 = rs[y], hi1 = rs[y + 1], lo2 = rs[ye], hi2 = rs[ye + 1];
                while (lo1 < hi1 || lo2 < hi2) {
                    const bool go1 = lo1 < hi1, go2 = lo2 < hi2;
                    const uint32_t mid1 = lo1 + ((hi1 - lo1) >> 1), mid2 = lo2 + ((hi2 - lo2) >> 1);
                    const uint32_t v1 = go1 ? spix[mid1] : 0u, v2 = go2 ? spix[mid2] : 0u;
                    if (go1) { if (v1 < (uint32_t)start) lo1 = mid1 + 1; else hi1 = mid1; }
                    if (go2) { if (v2 < (uint32_t)end) lo2 = mid2 + 1; else hi2 = mid2; }
                }
                lo = lo1;
                cnt = lo2 - lo1;                           // start < end: the second bound is not before the first
            }
        }
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const uint32_t total = __shfl(incl, kWave - 1);
        const uint32_t base = lo - (incl - cnt);           // pair k of the wave, owned by this lane, is entry base + k
        for (uint32_t k0 = 0; k0 < total; k0 += kRunsDeal * kWave) {       // wave-uniform
            uint32_t at[kRunsDeal], pt[kRunsDeal];
#pragma unroll
            for (int j = 0; j < kRunsDeal; ++j) {
                const uint32_t k = k0 + j * kWave + lane;
                int owner = 0;                             // lanes whose prefix is <= k; every lane takes part in the shuffles
#pragma unroll
                for (int step = kWave / 2; step; step >>= 1)
                    if (__shfl(incl, owner + step - 1) <= k) owner += step;
                at[j] = __shfl(base, owner & (kWave - 1)) + k;
            }
#pragma unroll
            for (int j = 0; j < kRunsDeal; ++j) pt[j] = k0 + j * kWave + lane < total ? spt[at[j]] : 0u;
#pragma unroll
            for (int j = 0; j < kRunsDeal; ++j)
                if (k0 + j * kWave + lane < total) atomicOr(bits + (pt[j] >> 5), 1u << (pt[j] & 31));
        }
    }
    __syncthreads();

    // flush: thread -> chunk (kCW words = two 32-B sectors); a wave's 64 chunks are one word of the row's chunk flags
    for (int c0 = wave * kWave; c0 < n_chunks; c0 += kBlock) {         // wave-uniform
        const int c = c0 + lane;
        uint64_t v[kCW] = {};
        if (c < n_chunks) {
#pragma unroll
            for (int q = 0; q < kCW; ++q) v[q] = s_row[c * kCW + q];
        }
        bool any = false;
#pragma unroll
        for (int h = 0; h < kCW; h += kPPT) {
            uint64_t o = 0;
#pragma unroll
            for (int q = 0; q < kPPT; ++q) o |= v[h + q];
            if (o) {
                any = true;
#pragma unroll
                for (int q = 0; q < kPPT; ++q) {
                    const int64_t w = (int64_t)c * kCW + h + q;
                    if (w < nw) rows[row * nw + w] = v[h + q];         // nw need not be a multiple of 4
                }
            }
        }
        const uint64_t flags = __ballot(any);
        if (lane == 0 && flags) chunk_mask[row * mw + (c0 >> 6)] |= flags;
    }
}

// masked_count += column sums of the rows: every row belongs to one (frame, mask), so the number of masks that cover a point
// over all frames is the number of rows with the point's bit.  One workgroup owns one 512-point chunk: its threads list
// the rows whose flag for the chunk is set in LDS (the order of the list does not matter to a sum), then every wave takes
// listed rows, lane l counting the points 8 l .. 8 l + 7 of the chunk in registers.
constexpr int kCountBlock = 1024;
constexpr int kCountBatch = 4;                   // loads a thread has in flight, in both phases
constexpr int kCountList = 4096;                 // rows listed per round

__global__ __launch_bounds__(kCountBlock) void sweep_runs_count_kernel(const uint64_t *__restrict__ rows, int64_t n_rows, int64_t nw,
                                                                       const uint64_t *__restrict__ chunk_mask, int mw,
                                                                       int64_t n_points, int32_t *__restrict__ masked_count)
{
    __shared__ int s_cnt[kCW * kWave];
    __shared__ int s_list[kCountList];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x;
    static_assert(kCountList == kCountBatch * kCountBlock, "a round lists what one batch of flag loads covers");
    for (int i = tid; i < kCW * kWave; i += kCountBlock) s_cnt[i] = 0;
    int cnt[8] = {};
    const int64_t word = (int64_t)c * kCW + (lane >> 3);
    const int shift = 8 * (lane & 7);
    const uint64_t *flag = chunk_mask + (c >> 6);
    for (int64_t r0 = 0; r0 < n_rows; r0 += kCountList) {             // block-uniform
        if (tid == 0) s_n = 0;
        __syncthreads();
        bool set[kCountBatch];
#pragma unroll
        for (int k = 0; k < kCountBatch; ++k) {
            const int64_t r = r0 + k * kCountBlock + tid;
            set[k] = r < n_rows && ((flag[r * mw] >> (c & 63)) & 1);
        }
#pragma unroll
        for (int k = 0; k < kCountBatch; ++k)
            if (set[k]) s_list[atomicAdd(&s_n, 1)] = k * kCountBlock + tid;
        __syncthreads();
        const int n = s_n;
        for (int i0 = wave * kCountBatch; i0 < n; i0 += (kCountBlock / kWave) * kCountBatch) {      // wave-uniform
            uint64_t v[kCountBatch];
#pragma unroll
            for (int k = 0; k < kCountBatch; ++k)
                v[k] = (i0 + k < n && word < nw) ? rows[(r0 + s_list[i0 + k]) * nw + word] : 0;
#pragma unroll
            for (int k = 0; k < kCountBatch; ++k) {
                const uint32_t b = (uint32_t)(v[k] >> shift) & 0xffu;
#pragma unroll
                for (int q = 0; q < 8; ++q) cnt[q] += (b >> q) & 1;
            }
        }
        __syncthreads();                                              // the list is rewritten by the next round
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (cnt[q]) atomicAdd(&s_cnt[8 * lane + q], cnt[q]);
    __syncthreads();
    for (int i = tid; i < kCW * kWave; i += kCountBlock) {
        const int64_t n = (int64_t)c * kCW * kWave + i;
        if (n < n_points && s_cnt[i]) masked_count[n] += s_cnt[i];        // the chunk's points are this workgroup's alone
    }
}

// viewed_count += the table's bit of the point in every frame with flag bit 0.  A wave owns one word of points; lane l
// fetches the words of the frames f0 + l, f0 + 64 + l, ... (the gathers of kViewedBatch x 64 frames in flight), then the
// non-zero words go round the wave one by one.
constexpr int kViewedBatch = 4;

__global__ __launch_bounds__(kBlock) void sweep_runs_viewed_kernel(int n_frames, const int32_t *__restrict__ depth_index,
                                                                   const int32_t *__restrict__ frame_flags,
                                                                   const uint64_t *__restrict__ vis_mask, int64_t stride,
                                                                   int64_t nw, int64_t n_points, int32_t *__restrict__ viewed_count)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (w >= nw) return;                                   // wave-uniform
    int cnt = 0;
    for (int f0 = 0; f0 < n_frames; f0 += kViewedBatch * kWave) {      // the gathers of kViewedBatch x 64 frames in flight
        uint64_t m[kViewedBatch];
        int32_t slot[kViewedBatch], flags[kViewedBatch];
#pragma unroll
        for (int k = 0; k < kViewedBatch; ++k) {
            const int f = f0 + k * kWave + lane;
            slot[k] = f < n_frames ? depth_index[f] : 0;
            flags[k] = f < n_frames ? frame_flags[f] : 0;
        }
#pragma unroll
        for (int k = 0; k < kViewedBatch; ++k) m[k] = (flags[k] & 1) ? vis_mask[(int64_t)slot[k] * stride + w] : 0;
#pragma unroll
        for (int k = 0; k < kViewedBatch; ++k) {
            uint64_t live = __ballot(m[k] != 0);
            while (live) {
                const int l = __ffsll((unsigned long long)live) - 1;
                live &= live - 1;
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)m[k], l);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(m[k] >> 32), l);
                cnt += (int)(((((uint64_t)hi << 32) | lo) >> lane) & 1);
            }
        }
    }
    const int64_t n = w * kWave + lane;
    if (n < n_points && cnt) viewed_count[n] += cnt;
}

}  // namespace bff

using namespace bff;

// The run-major form keeps one instance row in LDS: 8 bytes per 64 points, padded to whole chunks.
constexpr int64_t kRunsLdsMax = 64 * 1024;       // two workgroups per CU at worst; n_points <= 524 288

static int64_t runs_row_bytes(int64_t n_points)
{
    return (int64_t)sizeof(uint64_t) * kCW * ceil_div(ceil_div(n_points, (int64_t)kWave), (int64_t)kCW);
}

extern "C" int32_t bff_sweep_runs_ok(int64_t n_points)
{
    // both read per call: BFF_SWEEP_RUNS=0 keeps the point-major form, BFF_SWEEP_RUNS_LDS_BYTES lowers the bound
    const char *on = getenv("BFF_SWEEP_RUNS"), *cap = getenv("BFF_SWEEP_RUNS_LDS_BYTES");
    if (on && on[0] == '0' && on[1] == 0) return 0;
    int64_t bound = kRunsLdsMax;
    if (cap && *cap) bound = std::min<int64_t>(bound, std::max<int64_t>(0, atoll(cap)));
    return n_points > 0 && runs_row_bytes(n_points) <= bound;
}

extern "C" int bff_project_views_runs(int64_t n_points, int32_t n_frames, const int32_t *depth_index, int32_t height,
                                      int32_t width, const uint64_t *vis_mask, const uint32_t *vis_spix,
                                      const uint32_t *vis_spt, const uint32_t *vis_rowstart, const int32_t *run_start,
                                      const int32_t *run_end, const int32_t *mask_run_offs, const int32_t *view_mask_offs,
                                      int32_t word_bits, const int32_t *frame_mask, const int32_t *frame_rowbase,
                                      const int32_t *frame_nmask, const int32_t *frame_flags, uint64_t *rows, int64_t n_rows,
                                      int64_t nw, uint64_t *chunk_mask, int32_t *masked_count, int32_t *viewed_count,
                                      void *stream)
{
    if (n_points <= 0 || n_frames <= 0) return BFF_OK;
    BFF_REQUIRE(height > 0 && width > 0, "bff_project_views_runs: bad image size");
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "bff_project_views_runs: image larger than 2^31 pixels");
    BFF_REQUIRE(vis_mask && vis_spix && vis_spt && vis_rowstart, "bff_project_views_runs: null table");
    BFF_REQUIRE(word_bits == 32 || word_bits == 64, "bff_project_views_runs: word_bits must be 32 or 64");
    BFF_REQUIRE(depth_index && frame_mask && frame_rowbase && frame_nmask && frame_flags && run_start && run_end &&
                mask_run_offs && view_mask_offs && rows && chunk_mask && n_rows >= 0, "bff_project_views_runs: null pointer");
    BFF_REQUIRE(nw == ceil_div(n_points, 64), "bff_project_views_runs: nw must be ceil(n_points/64)");
    const int64_t row_bytes = runs_row_bytes(n_points);
    BFF_LIMIT(row_bytes <= kRunsLdsMax, "bff_project_views_runs: an instance row exceeds 64 KB of LDS (bff_sweep_runs_ok)");
    hipStream_t st = as_stream(stream);
    const int n_chunks = (int)ceil_div(nw, kCW), mw = (int)ceil_div(n_chunks, 64);
    hipEvent_t ev0, ev1;                                        // start rides on the first launch, stop on the last
    take_sweep_events(&ev0, &ev1);
    const bool count = masked_count != nullptr && n_rows > 0, viewed = viewed_count != nullptr;
    hipExtLaunchKernelGGL(sweep_runs_fill_kernel, dim3((unsigned)n_frames, (unsigned)word_bits), dim3(kBlock),
        (unsigned)row_bytes, st, ev0, (count || viewed) ? nullptr : ev1, 0,
        n_frames, depth_index, height, width, vis_spix, vis_spt, vis_rowstart, run_start, run_end, mask_run_offs,
        view_mask_offs, frame_mask, frame_rowbase, frame_nmask, rows, nw, n_chunks, chunk_mask, mw);
    if (count)
        hipExtLaunchKernelGGL(sweep_runs_count_kernel, dim3((unsigned)n_chunks), dim3(kCountBlock), 0, st,
            nullptr, viewed ? nullptr : ev1, 0, rows, n_rows, nw, chunk_mask, mw, n_points, masked_count);
    if (viewed)
        hipExtLaunchKernelGGL(sweep_runs_viewed_kernel, dim3((unsigned)ceil_div(nw, kBlock / kWave)), dim3(kBlock), 0, st,
            nullptr, ev1, 0, n_frames, depth_index, frame_flags, vis_mask, bff_visibility_words(n_points), nw, n_points,
            viewed_count);
    return launched("bff_project_views_runs");
}

extern "C" int bff_visibility_sorted_bytes(int32_t n_slots, int32_t height, int64_t n_pixels, int64_t *bytes)
{
    BFF_REQUIRE(n_slots >= 0 && height >= 0 && n_pixels >= 0 && bytes, "bff_visibility_sorted_bytes: bad arguments");
    bytes[0] = (int64_t)sizeof(uint32_t) * n_pixels;
    bytes[1] = (int64_t)sizeof(uint32_t) * n_pixels;
    bytes[2] = (int64_t)sizeof(uint32_t) * n_slots * ((int64_t)height + 1);
    return BFF_OK;
}

extern "C" int bff_visibility_sorted(const uint64_t *vis_mask, const uint32_t *vis_off, const uint32_t *vis_pix,
                                     int64_t n_pixels, int64_t n_points, int32_t n_slots, int32_t height, int32_t width,
                                     uint32_t *vis_spix, uint32_t *vis_spt, uint32_t *vis_rowstart, void *temp,
                                     size_t *temp_bytes, void *stream)
{
    BFF_REQUIRE(n_pixels >= 0 && n_points >= 0 && n_slots >= 0 && temp_bytes, "bff_visibility_sorted: bad sizes");
    BFF_REQUIRE(height > 0 && width > 0, "bff_visibility_sorted: bad image size");
    BFF_LIMIT(height < (1 << 15) && width < (1 << 15), "bff_visibility_sorted: image too large for packed pixels");
    BFF_LIMIT(n_slots <= 65535, "bff_visibility_sorted: too many depth slots");
    BFF_LIMIT(n_pixels < (1ll << 32), "bff_visibility_sorted: more than 2^32 visible pairs");
    const int64_t hw = (int64_t)height * width, span = hw * std::max(n_slots, 1);
    BFF_LIMIT(span <= (1ll << 32), "bff_visibility_sorted: slots x pixels exceed the 32-bit sort key");
    hipStream_t st = as_stream(stream);
    unsigned key_bits = 1;
    while (key_bits < 32 && (1ll << key_bits) < span) ++key_bits;
    const size_t part = ((size_t)n_pixels * sizeof(uint32_t) + 255) & ~(size_t)255;    // keys, points, sorted keys
    size_t need = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n_pixels, 0, key_bits, st);
    if (e != hipSuccess) return fail((int)e, "bff_visibility_sorted: %s", hipGetErrorString(e));
    if (!temp) { *temp_bytes = 3 * part + need; return BFF_OK; }
    BFF_REQUIRE(*temp_bytes >= 3 * part + need, "bff_visibility_sorted: temp storage too small");
    if (n_slots == 0 || n_points == 0) return BFF_OK;
    BFF_REQUIRE(vis_mask && vis_off && vis_rowstart && (n_pixels == 0 || (vis_pix && vis_spix && vis_spt)),
                "bff_visibility_sorted: null pointer");
    const int64_t stride = bff_visibility_words(n_points);
    if (n_pixels > 0) {
        uint32_t *keys = reinterpret_cast<uint32_t *>(temp);
        uint32_t *pts = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(temp) + part);
        uint32_t *sorted = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(temp) + 2 * part);
        dim3 grid((unsigned)ceil_div(stride, kBlock / kWave), (unsigned)n_slots);
        vis_sort_keys_kernel<<<grid, kBlock, 0, st>>>(vis_mask, vis_off, vis_pix, stride, n_pixels, width, (uint32_t)hw, keys, pts);
        // a radix sort is stable: pairs of one pixel keep their (ascending) point order
        e = rocprim::radix_sort_pairs(reinterpret_cast<char *>(temp) + 3 * part, need, (const uint32_t *)keys, sorted,
                                      (const uint32_t *)pts, vis_spt, (size_t)n_pixels, 0, key_bits, st);
        if (e != hipSuccess) return fail((int)e, "bff_visibility_sorted: %s", hipGetErrorString(e));
        vis_sorted_pixels_kernel<<<(unsigned)ceil_div(n_pixels, kBlock), kBlock, 0, st>>>(sorted, n_pixels, (uint32_t)hw, vis_spix);
    }
    vis_rowstart_kernel<<<(unsigned)ceil_div((int64_t)n_slots * (height + 1), kBlock), kBlock, 0, st>>>(
        vis_spix, vis_off, stride, n_pixels, n_slots, height, width, vis_rowstart);
    return launched("bff_visibility_sorted");
}
