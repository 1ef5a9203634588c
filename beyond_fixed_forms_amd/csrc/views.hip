// The best views of 3-D instances, read off the visibility table (include/bff_hip.h: bff_instance_views,
// bff_select_views).
#include <cmath>

#include "common.h"

namespace bff {

constexpr int kViewBlock = 256;                      // 4 waves
constexpr int kViewWaves = kViewBlock / kWave;
constexpr int kViewTile = 16;                        // slots of one workgroup: 4 per wave, one after the other
constexpr int kViewLdsWords = 2048;                  // non-zero words of one instance kept in LDS: 24 KB (131 072 points)

// ---- visible points and pixel boxes per (instance, slot) -----------------------------------------------------------
// One workgroup per (instance k, tile of kViewTile slots).  The instance's non-zero words are compacted once, in word
// order, into LDS as (word index, bits): the cloud is Morton-sorted, so an instance fills a short span of its row and the
// slots of the tile then walk only that.  The compaction is a ballot scan (no atomics, not even in LDS); a row with more
// than kViewLdsWords non-zero words is walked in global memory instead, zero words included.  One wave per slot: lane l takes
// entry l, l + 64, ... and, where the instance and the slot share bits, walks them: the pair of bit b of word w lies at
// vis_off[f][w] + popcount(vis_mask[f][w] below b).  Count, minima and maxima stay in registers; a butterfly over the wave
// ends in one store of the five integers by lane 0, sentinels included (an empty pair keeps the initial values).
__global__ __launch_bounds__(kViewBlock) void instance_views_kernel(
    const uint64_t *__restrict__ rows, int64_t nw, const uint64_t *__restrict__ vis_mask, const uint32_t *__restrict__ vis_off,
    const uint32_t *__restrict__ vis_pix, int n_slots, int64_t stride, int64_t n_pixels, int height, int width,
    int32_t *__restrict__ visible, int32_t *__restrict__ box)
{
    __shared__ uint64_t s_bits[kViewLdsWords];
    __shared__ uint32_t s_word[kViewLdsWords];
    __shared__ int s_wave[kViewWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t k = blockIdx.x;
    const uint64_t *row = rows + k * nw;

    int total = 0;                                                 // block-uniform: non-zero words so far
    for (int64_t base = 0; base < nw; base += kViewBlock) {
        const int64_t w = base + tid;
        const uint64_t b = w < nw ? row[w] : 0;
        const uint64_t bal = __ballot(b != 0);
        if (lane == 0) s_wave[wave] = popc64(bal);
        __syncthreads();
        int before = 0, piece = 0;
#pragma unroll
        for (int q = 0; q < kViewWaves; ++q) {
            const int t = s_wave[q];
            before += q < wave ? t : 0;
            piece += t;
        }
        const int at = total + before + popc64(bal & ((1ull << lane) - 1));
        if (b != 0 && at < kViewLdsWords) {
            s_bits[at] = b;
            s_word[at] = (uint32_t)w;
        }
        total += piece;
        __syncthreads();                                           // s_wave is rewritten by the next piece
        if (total > kViewLdsWords) break;                          // block-uniform: the row is walked in global memory
    }
    const bool in_lds = total <= kViewLdsWords;                    // block-uniform
    const int64_t n_entries = in_lds ? total : nw;

    const int f0 = blockIdx.y * kViewTile;
    const int f1 = min(n_slots, f0 + kViewTile);
    for (int f = f0 + wave; f < f1; f += kViewWaves) {             // wave-uniform
        const uint64_t *fmask = vis_mask + (int64_t)f * stride;
        const uint32_t *foff = vis_off + (int64_t)f * stride;
        int cnt = 0, u0 = width, v0 = height, u1 = -1, v1 = -1;
        for (int64_t i = lane; i < n_entries; i += kWave) {
            const int64_t w = in_lds ? (int64_t)s_word[i] : i;
            const uint64_t bits = in_lds ? s_bits[i] : row[i];
            const uint64_t m = fmask[w];                           // w < nw <= stride
            uint64_t h = bits & m;
            if (h == 0) continue;
            const int64_t at0 = foff[w];
            cnt += popc64(h);
            for (; h; h &= h - 1) {
                const int b = __builtin_ctzll(h);
                const int64_t at = at0 + popc64(m & ((1ull << b) - 1));
                if (at < n_pixels) {                               // a table whose offsets overrun its pixels: no read
                    const uint32_t p = vis_pix[at];
                    const int u = (int)(p & 0xffffu), v = (int)(p >> 16);
                    u0 = min(u0, u);
                    v0 = min(v0, v);
                    u1 = max(u1, u);
                    v1 = max(v1, v);
                }
            }
        }
#pragma unroll
        for (int d = kWave / 2; d; d >>= 1) {
            cnt += __shfl_xor(cnt, d);
            u0 = min(u0, __shfl_xor(u0, d));
            v0 = min(v0, __shfl_xor(v0, d));
            u1 = max(u1, __shfl_xor(u1, d));
            v1 = max(v1, __shfl_xor(v1, d));
        }
        if (lane == 0) {
            const int64_t o = k * n_slots + f;
            visible[o] = cnt;
            reinterpret_cast<int4 *>(box)[o] = make_int4(u0, v0, u1, v1);
        }
    }
}

// ---- top views and their crops --------------------------------------------------------------------------------------
// One wave per instance.  A slot's key is count << 32 | ~position, so that a larger key is more points or, at equal
// points, the earlier slot; keys are distinct.  Round t takes the largest key below the one round t - 1 took (lane l scans
// slots l, l + 64, ...; a butterfly of 64-bit maxima) -- nothing is marked and nothing is kept between rounds but that key.
// Lane t keeps round t's key and, after the last round, writes its view and the crops of its box at every level.
__device__ __forceinline__ int crop_expand(int extent, double expand, int level)
{
    // (int)floor((double)extent * expand) * level; the product is cut at 2^15, past every image side (bff_hip.h), before
    // the conversion, so that no expand overflows an int
    return (int)fmin(floor((double)extent * expand), 32768.0) * level;
}

__global__ __launch_bounds__(kViewBlock) void select_views_kernel(
    const int32_t *__restrict__ visible, const int32_t *__restrict__ box, int n_rows, int n_slots, int height, int width,
    int top_k, int min_points, int levels, double expand, int32_t *__restrict__ top, int32_t *__restrict__ top_visible,
    int32_t *__restrict__ crops)
{
    const int lane = lane_id();
    const int64_t k = (int64_t)blockIdx.x * kViewWaves + (threadIdx.x >> 6);      // wave-uniform
    if (k >= n_rows) return;
    const int32_t *vis = visible + k * n_slots;
    const int need = max(1, min_points);
    uint64_t prev = ~0ull, mine = 0;
    for (int t = 0; t < top_k; ++t) {
        uint64_t best = 0;
        if (prev != 0) {                                           // wave-uniform: no candidate was left a round ago
            for (int f = lane; f < n_slots; f += kWave) {
                const int c = vis[f];
                const uint64_t key = ((uint64_t)(uint32_t)c << 32) | (uint32_t)~(uint32_t)f;
                if (c >= need && key < prev && key > best) best = key;
            }
#pragma unroll
            for (int d = kWave / 2; d; d >>= 1) {
                const uint64_t o = __shfl_xor(best, d);
                best = o > best ? o : best;
            }
        }
        if (lane == t) mine = best;
        prev = best;
    }
    if (lane >= top_k) return;
    const int f = mine ? (int)~(uint32_t)mine : -1;
    top[k * top_k + lane] = f;
    top_visible[k * top_k + lane] = (int32_t)(mine >> 32);
    int4 b = make_int4(width, height, -1, -1);
    if (f >= 0) b = reinterpret_cast<const int4 *>(box)[k * n_slots + f];
    int4 *out = reinterpret_cast<int4 *>(crops) + (k * top_k + lane) * levels;
    for (int l = 0; l < levels; ++l) {
        int4 c = b;
        if (f >= 0) {
            const int ex = crop_expand(b.z - b.x, expand, l), ey = crop_expand(b.w - b.y, expand, l);
            c = make_int4(max(0, b.x - ex), max(0, b.y - ey), min(width - 1, b.z + ex), min(height - 1, b.w + ey));
        }
        out[l] = c;
    }
}

}  // namespace bff

using namespace bff;

extern "C" int32_t bff_instance_views_lds_words(void) { return kViewLdsWords; }

static int views_limits(const char *who, int32_t n_rows, int32_t n_slots, int32_t height, int32_t width)
{
    BFF_REQUIRE(n_rows >= 0 && n_slots >= 0, "%s: bad sizes", who);
    BFF_REQUIRE(height > 0 && width > 0, "%s: bad image size", who);
    BFF_LIMIT(n_slots <= 65535, "%s: %d slots, more than 65535", who, n_slots);
    BFF_LIMIT(height < (1 << 15) && width < (1 << 15), "%s: image too large for packed pixels", who);
    BFF_LIMIT((int64_t)n_rows * n_slots * 4 < (1ll << 31), "%s: %d instances x %d slots x 4 reaches 2^31", who, n_rows, n_slots);
    return BFF_OK;
}

extern "C" int bff_instance_views(const uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *vis_mask,
                                  const uint32_t *vis_off, const uint32_t *vis_pix, int32_t n_slots, int64_t stride,
                                  int64_t n_pixels, int32_t height, int32_t width, int32_t *visible, int32_t *box, void *stream)
{
    const int rc = views_limits("bff_instance_views", n_rows, n_slots, height, width);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(nw >= 0 && stride >= nw && n_pixels >= 0, "bff_instance_views: bad sizes (stride must hold the rows' words)");
    BFF_LIMIT(nw < (1ll << 32), "bff_instance_views: rows of 2^32 words");
    if (n_rows == 0 || n_slots == 0) return BFF_OK;
    BFF_REQUIRE(visible && box && (nw == 0 || (rows && vis_mask && vis_off)) && (n_pixels == 0 || vis_pix),
                "bff_instance_views: null pointer");
    BFF_REQUIRE((reinterpret_cast<uintptr_t>(box) & 15) == 0, "bff_instance_views: box is not 16-byte aligned");
    dim3 grid((unsigned)n_rows, (unsigned)ceil_div(n_slots, kViewTile));
    instance_views_kernel<<<grid, kViewBlock, 0, as_stream(stream)>>>(rows, nw, vis_mask, vis_off, vis_pix, n_slots, stride,
                                                                     n_pixels, height, width, visible, box);
    return launched("bff_instance_views");
}

extern "C" int bff_select_views(const int32_t *visible, const int32_t *box, int32_t n_rows, int32_t n_slots, int32_t height,
                                int32_t width, int32_t top_k, int32_t min_points, int32_t levels, double expand, int32_t *top,
                                int32_t *top_visible, int32_t *crops, void *stream)
{
    const int rc = views_limits("bff_select_views", n_rows, n_slots, height, width);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(std::isfinite(expand) && expand >= 0.0, "bff_select_views: expand must be finite and >= 0");
    BFF_LIMIT(top_k >= 1 && top_k <= 64, "bff_select_views: top_k %d outside 1 .. 64", top_k);
    BFF_LIMIT(levels >= 1 && levels <= 8, "bff_select_views: %d crop levels outside 1 .. 8", levels);
    if (n_rows == 0 || n_slots == 0) return BFF_OK;
    BFF_REQUIRE(visible && box && top && top_visible && crops, "bff_select_views: null pointer");
    BFF_REQUIRE(((reinterpret_cast<uintptr_t>(box) | reinterpret_cast<uintptr_t>(crops)) & 15) == 0,
                "bff_select_views: box or crops is not 16-byte aligned");
    select_views_kernel<<<(unsigned)ceil_div(n_rows, kViewWaves), kViewBlock, 0, as_stream(stream)>>>(
        visible, box, n_rows, n_slots, height, width, top_k, min_points, levels, expand, top, top_visible, crops);
    return launched("bff_select_views");
}
