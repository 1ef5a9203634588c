// Row directory of the 2-D masks: per mask a bounding box and one 32-bit entry per image row of the box, built from the
// run tables alone (formats: mask_rows.h).  The sweep's look-up mode asks it at the pixels visible points project to,
// instead of decoding every mask view into a dense image first.  Three launches, no host round trip:
//   boxes    one wave per mask: column range over its runs, row range from its first and last run, height
//   offsets  one block: exclusive scan of the heights (in place, word 2 of the mask table)
//   entries  one thread per (mask, row of its box): two searches in the mask's run list
// Every output word is a function of the run tables only (no atomics, no order dependence): deterministic.
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "mask_rows.h"

namespace bff {

__global__ __launch_bounds__(256) void mask_boxes_kernel(const int32_t *__restrict__ run_start,
                                                         const int32_t *__restrict__ run_end,
                                                         const int32_t *__restrict__ mask_run_offs, int n_masks, int W,
                                                         uint4 *__restrict__ tab)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g > n_masks) return;                                   // wave-uniform; g == n_masks: the closing entry
    const int lo = mask_run_offs[g];
    const int hi = g < n_masks ? mask_run_offs[g + 1] : lo;
    uint32_t c0 = 0xffffu, c1 = 0;
    for (int i = lo + lane; i < hi; i += 64) {
        const uint32_t s = (uint32_t)run_start[i], e = (uint32_t)run_end[i] - 1;
        const uint32_t rs = s / (uint32_t)W, re = e / (uint32_t)W;
        const bool one_row = rs == re;                         // a run that crosses a row end touches columns 0 and W - 1
        c0 = min(c0, one_row ? s - rs * W : 0u);
        c1 = max(c1, one_row ? e - re * W : (uint32_t)W - 1);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        c0 = min(c0, (uint32_t)__shfl_xor((int)c0, d));
        c1 = max(c1, (uint32_t)__shfl_xor((int)c1, d));
    }
    if (lane == 0) {
        if (hi > lo) {
            const uint32_t r0 = (uint32_t)run_start[lo] / (uint32_t)W, r1 = ((uint32_t)run_end[hi - 1] - 1) / (uint32_t)W;
            tab[g] = make_uint4(c0 | (r0 << 16), c1 | (r1 << 16), r1 - r0 + 1, (uint32_t)lo);
        } else {
            tab[g] = make_uint4(0xffffffffu, 0u, 0u, (uint32_t)lo);
        }
    }
}

// exclusive scan of word 2 (the heights) of the n entries of the mask table, in place: thread t owns entries
// [t * per, (t + 1) * per)
__global__ __launch_bounds__(1024) void mask_dir_offsets_kernel(uint4 *__restrict__ tab, int n, int per)
{
    __shared__ uint32_t wave_sum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i0 = min(t * per, n), i1 = min(i0 + per, n);
    constexpr int kChunk = 16;                                 // loads of a chunk are all in flight together
    uint32_t sum = 0;
    for (int c = i0; c < i1; c += kChunk) {
        uint32_t h[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) h[k] = c + k < i1 ? tab[c + k].z : 0u;
#pragma unroll
        for (int k = 0; k < kChunk; ++k) sum += h[k];
    }
    uint32_t inc = sum;                                        // inclusive scan over the wave, then over the 16 waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t at = inc - sum;
    for (int w = 0; w < wave; ++w) at += wave_sum[w];
    for (int c = i0; c < i1; c += kChunk) {
        uint32_t h[kChunk];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) h[k] = c + k < i1 ? tab[c + k].z : 0u;
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            if (c + k < i1) tab[c + k].z = at;
            at += h[k];
        }
    }
}

__global__ __launch_bounds__(256) void mask_dir_entries_kernel(const int32_t *__restrict__ run_start,
                                                               const int32_t *__restrict__ run_end, int W,
                                                               const uint4 *__restrict__ tab, uint32_t *__restrict__ dir)
{
    const int64_t g = blockIdx.x;
    const uint4 t = tab[g];
    if (t.x == 0xffffffffu) return;                            // no runs: no rows
    const int r0 = (int)(t.x >> 16), r1 = (int)(t.y >> 16);
    const int r = r0 + (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (r > r1) return;
    const int lo = (int)t.w, hi = (int)tab[g + 1].w;
    const int row0 = r * W, row1 = row0 + W;                   // H * W < 2^31 (checked by the entry point)
    // first run that ends behind the row's first pixel.  A mask is mostly one run per row: then it is run r - r0
    int a = lo + (r - r0), b = hi;
    if (!(a < hi && run_end[a] > row0 && (a == lo || run_end[a - 1] <= row0))) {
        a = lo;
        while (a < b) {
            const int mid = a + ((b - a) >> 1);
            if (run_end[mid] > row0) b = mid; else a = mid + 1;
        }
    }
    // first run at or behind a that starts behind the row: mostly a or a + 1, else searched
    b = a;
    if (b < hi && run_start[b] < row1) {
        ++b;
        if (b < hi && run_start[b] < row1) {
            int e = hi;
            ++b;
            while (b < e) {
                const int mid = b + ((e - b) >> 1);
                if (run_start[mid] >= row1) e = mid; else b = mid + 1;
            }
        }
    }
    const uint32_t count = (uint32_t)(b - a);
    uint32_t entry = 0;
    if (count == 1) {
        const int cs = max(run_start[a], row0) - row0, ce = min(run_end[a], row1) - row0;
        entry = (uint32_t)cs | ((uint32_t)ce << 15);
    } else if (count > 1) {
        uint32_t first = (uint32_t)(a - lo), c = min(count, kRowCountSat);
        if (first > kRowFirstMask) { first = 0; c = kRowCountSat; }
        entry = kRowFlag | (c << kRowCountShift) | first;
    }
    dir[(size_t)t.z + (size_t)(r - r0)] = entry;
}

}  // namespace bff

using namespace bff;

// BFF_MASK_LOOKUP=rows|dense, read once
static bool lookup_rows_on()
{
    static const bool on = [] { const char *e = getenv("BFF_MASK_LOOKUP"); return !e || strcmp(e, "dense") != 0; }();
    return on;
}

extern "C" int32_t bff_mask_lookup_rows(int32_t height, int32_t width, int64_t n_masks)
{
    // the sweep keeps the resize's tap table (12 bytes per image row and column) and the frames' mask tables in 64 KB of LDS
    return lookup_rows_on() && height > 0 && width > 0 && width < (1 << 15) && height < (1 << 15) &&
           12 * ((int64_t)height + width) + 16 + 16 * kRowsFrames * kRowsMaskSlots + 8192 <= 64 * 1024 &&
           n_masks * (int64_t)height < (1ll << 32) && (int64_t)height * width < (1ll << 31);
}

extern "C" int bff_mask_row_directory(const int32_t *run_start, const int32_t *run_end, const int32_t *mask_run_offs,
                                      int32_t n_masks, int32_t height, int32_t width, uint32_t *mask_tab,
                                      uint32_t *mask_dir, void *stream)
{
    BFF_REQUIRE(n_masks >= 0 && height > 0 && width > 0, "bff_mask_row_directory: bad sizes");
    BFF_LIMIT(width < (1 << 15) && height < (1 << 15), "bff_mask_row_directory: image too large for packed entries");
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "bff_mask_row_directory: image larger than 2^31 pixels");
    BFF_LIMIT((int64_t)n_masks * height < (1ll << 32), "bff_mask_row_directory: directory larger than 2^32 entries");
    BFF_REQUIRE(mask_run_offs && mask_tab && (mask_dir || n_masks == 0), "bff_mask_row_directory: null pointer");   // run arrays may be empty (NULL)
    hipStream_t st = as_stream(stream);
    uint4 *tab = reinterpret_cast<uint4 *>(mask_tab);
    mask_boxes_kernel<<<(unsigned)ceil_div((int64_t)n_masks + 1, 4), 256, 0, st>>>(run_start, run_end, mask_run_offs, n_masks,
                                                                                  width, tab);
    mask_dir_offsets_kernel<<<1, 1024, 0, st>>>(tab, n_masks + 1, (int)ceil_div((int64_t)n_masks + 1, 1024));
    if (n_masks > 0)
        mask_dir_entries_kernel<<<dim3((unsigned)n_masks, (unsigned)ceil_div(height, 256)), 256, 0, st>>>(run_start, run_end,
                                                                                                         width, tab, mask_dir);
    return launched("bff_mask_row_directory");
}
