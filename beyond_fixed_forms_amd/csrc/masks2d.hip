// Dense 2-D masks -> bit planes + run tables (include/bff_hip.h: a1b).
//
// The producer in front of the path (SEG:276-305) holds a frame's masks as a dense (M,1,H,W) bool tensor on the
// device; the reference turns it into RLE one mask at a time with a nonzero + a host copy each (RLE:10-32).  Here the
// dense bytes are read ONCE, by the count pass, which leaves 1/8 of them behind as bit planes and the number of runs of
// every mask; the run pass ranks the run starts and ends of the bit planes and writes the int32 [start, end) tables
// that bff_rle_to_maskbits reads.  The host's only part is the scan of the counts in between (one device cumsum).
//
// Bound: the count pass is a pure HBM stream (one byte in, 1/64 word out per pixel, a dozen integer ops per 16
// pixels); the run pass reads the bit planes (mostly from L2) and is bound by the latency of its block scans.
#include <algorithm>

#include "common.h"

namespace bff {

constexpr int kM2Threads = 256;
constexpr int kM2WavePixels = 16 * kWave;                       // a wave reads 1024 contiguous bytes per step
constexpr int kM2Steps = 2;                                     // steps per wave
constexpr int kM2Tile = kM2Steps * (kM2Threads / kWave) * kM2WavePixels;     // pixels per block (8192)
constexpr unsigned kM2MaxGridY = 65535;

struct __attribute__((packed)) bytes16 { uint32_t v[4]; };      // alignment 1: a mask's base is g * n_pixels

// 4 bytes -> 4 bits (bit k = byte k != 0).  The high bit of every byte of `nz` says "byte non-zero" (the 7-bit add
// cannot carry into the next byte); the multiply moves bit 8k to bit 24 + k, all partial products land on distinct
// bits, so there are no carries.
__device__ __forceinline__ uint32_t nonzero_nibble(uint32_t x)
{
    const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return (((nz >> 7) * 0x01020408u) >> 24) & 0xfu;
}

// grid (pixel tiles, masks).  Lane l of a wave takes pixels [16 l, 16 l + 16) of the wave's 1024-pixel stretch, four
// lanes make one 64-bit word (shuffles inside the quad), the quad's first lane owns it.
__global__ __launch_bounds__(kM2Threads) void masks2d_count_kernel(const uint8_t *__restrict__ masks, int64_t n_pixels,
                                                                    int64_t nw, int mask0, uint64_t *__restrict__ bits,
                                                                    int32_t *__restrict__ n_runs)
{
    __shared__ int part[kM2Threads / kWave];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int g = mask0 + blockIdx.y;
    const uint8_t *mask = masks + (int64_t)g * n_pixels;
    uint64_t *row = bits + (int64_t)g * nw;
    const int64_t tile0 = (int64_t)blockIdx.x * kM2Tile;
    uint32_t got[kM2Steps];
    uint32_t before[kM2Steps];
#pragma unroll
    for (int s = 0; s < kM2Steps; ++s) {                        // every load of the block is issued before any is used
        const int64_t w0 = tile0 + (int64_t)(s * (kM2Threads / kWave) + wave) * kM2WavePixels;   // the wave's stretch
        const int64_t p0 = w0 + 16 * lane;
        uint32_t b16 = 0;
        if (p0 + 16 <= n_pixels) {
            bytes16 v;
            __builtin_memcpy(&v, mask + p0, 16);
            b16 = nonzero_nibble(v.v[0]) | (nonzero_nibble(v.v[1]) << 4) | (nonzero_nibble(v.v[2]) << 8) |
                  (nonzero_nibble(v.v[3]) << 12);
        } else {                                                // the mask's last, partial 16 pixels: byte by byte
            for (int k = 0; k < 16; ++k)
                if (p0 + k < n_pixels && mask[p0 + k]) b16 |= 1u << k;
        }
        got[s] = b16;
        // the pixel before the stretch comes from memory, not from another wave or block
        before[s] = (lane == 0 && w0 > 0 && w0 < n_pixels) ? (mask[w0 - 1] != 0) : 0u;
    }
    int c = 0;
#pragma unroll
    for (int s = 0; s < kM2Steps; ++s) {
        const int64_t w0 = tile0 + (int64_t)(s * (kM2Threads / kWave) + wave) * kM2WavePixels;
        uint32_t h = got[s] << (16 * (lane & 1));
        h |= (uint32_t)__shfl_xor((int)h, 1);                   // 32 pixels of the lane pair
        const uint32_t o = (uint32_t)__shfl_xor((int)h, 2);     // the other pair's
        const uint64_t cur = (lane & 2) ? (((uint64_t)h << 32) | o) : (((uint64_t)o << 32) | h);
        const uint32_t top = (uint32_t)(cur >> 63);
        uint32_t prev = (uint32_t)__shfl_up((int)top, 4);       // last pixel of the word before
        const uint32_t first = (uint32_t)__shfl((int)before[s], 0);
        if (lane < 4) prev = first;
        const uint64_t starts = cur & ~((cur << 1) | prev);
        const int64_t w = (w0 >> 6) + (lane >> 2);
        if ((lane & 3) == 0 && w < nw) {
            row[w] = cur;
            c += popc64(starts);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int q = 0; q < kM2Threads / kWave; ++q) t += part[q];
        if (t) atomicAdd(n_runs + g, t);                        // exact, order independent
    }
}

// grid (segments, masks): a block ranks the edges of words [seg * seg_words, (seg + 1) * seg_words) of its mask -- the
// last segment includes the virtual word nw.  The ranks of its first start and first end are the edges of the words
// before the segment, which the block counts itself (the planes are 1/8 of the dense bytes and sit in L2).  Starts and
// ends are ranked independently: the k-th end closes the k-th start.
__global__ __launch_bounds__(kM2Threads) void masks2d_runs_kernel(const uint64_t *__restrict__ bits, int64_t nw,
                                                                   int64_t seg_words, int mask0,
                                                                   const int32_t *__restrict__ run_offs,
                                                                   int32_t *__restrict__ run_start,
                                                                   int32_t *__restrict__ run_end)
{
    __shared__ int wsum[kM2Threads / kWave];
    __shared__ int psum[2][kM2Threads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = mask0 + blockIdx.y;
    const uint64_t *row = bits + (int64_t)g * nw;
    const int64_t w_begin = (int64_t)blockIdx.x * seg_words;
    const int64_t w_end = min(w_begin + seg_words, nw + 1);     // exclusive; nw + 1: the virtual word
    const int64_t lo = run_offs[g];
    const int n_mine = run_offs[g + 1] - run_offs[g];           // nothing is written past the mask's own slots
    int ps = 0, pe = 0;
    for (int64_t w = tid; w < w_begin; w += kM2Threads) {
        uint64_t st, en;
        rle_word_edges(row, w, nw, st, en);
        ps += popc64(st);
        pe += popc64(en);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { ps += __shfl_xor(ps, d); pe += __shfl_xor(pe, d); }
    if (lane == 0) { psum[0][wave] = ps; psum[1][wave] = pe; }
    __syncthreads();
    int base_st = 0, base_en = 0;
#pragma unroll
    for (int q = 0; q < kM2Threads / kWave; ++q) { base_st += psum[0][q]; base_en += psum[1][q]; }
    for (int64_t w0 = w_begin; w0 < w_end; w0 += kM2Threads) {
        const int64_t w = w0 + tid;
        uint64_t st = 0, en = 0;
        if (w < w_end) rle_word_edges(row, w, nw, st, en);
        const int packed = popc64(st) | (popc64(en) << 16);     // <= 32 starts / ends per word, 256 words: no carry
        int incl = packed;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int excl = incl - packed, total = 0;
#pragma unroll
        for (int q = 0; q < kM2Threads / kWave; ++q) { if (q < wave) excl += wsum[q]; total += wsum[q]; }
        int rs = base_st + (excl & 0xFFFF), re = base_en + (excl >> 16);
        while (st) {
            const int b = __ffsll((unsigned long long)st) - 1;
            st &= st - 1;
            if (rs < n_mine) run_start[lo + rs] = (int32_t)(w * 64 + b);
            ++rs;
        }
        while (en) {
            const int b = __ffsll((unsigned long long)en) - 1;
            en &= en - 1;
            if (re < n_mine) run_end[lo + re] = (int32_t)(w * 64 + b);
            ++re;
        }
        base_st += total & 0xFFFF;
        base_en += total >> 16;
        __syncthreads();
    }
}

}  // namespace bff

using namespace bff;

extern "C" int32_t bff_masks2d_tile_pixels(void) { return kM2Tile; }

extern "C" int bff_masks2d_count(const uint8_t *masks, int32_t n_masks, int64_t n_pixels, uint64_t *bits, int32_t *n_runs,
                                 void *stream)
{
    BFF_REQUIRE(n_masks >= 0 && n_pixels >= 0, "bff_masks2d_count: bad sizes");
    BFF_LIMIT(n_pixels < (1ll << 31), "bff_masks2d_count: n_pixels = %lld, at most 2^31 - 1", (long long)n_pixels);
    if (n_masks == 0) return BFF_OK;
    BFF_REQUIRE(n_runs, "bff_masks2d_count: null pointer");
    hipError_t e = hipMemsetAsync(n_runs, 0, sizeof(int32_t) * (size_t)n_masks, as_stream(stream));
    if (e != hipSuccess) return fail((int)e, "bff_masks2d_count: memset: %s", hipGetErrorString(e));
    if (n_pixels == 0) return BFF_OK;
    BFF_REQUIRE(masks && bits, "bff_masks2d_count: null pointer");
    const int64_t nw = ceil_div(n_pixels, 64);
    for (int64_t m0 = 0; m0 < n_masks; m0 += kM2MaxGridY) {
        dim3 grid((unsigned)ceil_div(n_pixels, kM2Tile), (unsigned)std::min<int64_t>(kM2MaxGridY, n_masks - m0));
        masks2d_count_kernel<<<grid, kM2Threads, 0, as_stream(stream)>>>(masks, n_pixels, nw, (int)m0, bits, n_runs);
    }
    return launched("bff_masks2d_count");
}

extern "C" int bff_masks2d_runs(const uint64_t *bits, int32_t n_masks, int64_t n_pixels, const int32_t *run_offs,
                                int32_t *run_start, int32_t *run_end, void *stream)
{
    BFF_REQUIRE(n_masks >= 0 && n_pixels >= 0, "bff_masks2d_runs: bad sizes");
    BFF_LIMIT(n_pixels < (1ll << 31), "bff_masks2d_runs: n_pixels = %lld, at most 2^31 - 1", (long long)n_pixels);
    if (n_masks == 0 || n_pixels == 0) return BFF_OK;
    BFF_REQUIRE(bits && run_offs, "bff_masks2d_runs: null pointer");     // the run tables are empty (NULL) when no mask has a run
    const int64_t nw = ceil_div(n_pixels, 64);
    // segments of 2048 words (8 scan steps); at most 64 per mask, since every block also counts the words before its own
    int64_t seg_words = 8 * kM2Threads;
    if (ceil_div(nw + 1, seg_words) > 64) seg_words = ceil_div(ceil_div(nw + 1, 64), kM2Threads) * kM2Threads;
    for (int64_t m0 = 0; m0 < n_masks; m0 += kM2MaxGridY) {
        dim3 grid((unsigned)ceil_div(nw + 1, seg_words), (unsigned)std::min<int64_t>(kM2MaxGridY, n_masks - m0));
        masks2d_runs_kernel<<<grid, kM2Threads, 0, as_stream(stream)>>>(bits, nw, seg_words, (int)m0, run_offs, run_start,
                                                                       run_end);
    }
    return launched("bff_masks2d_runs");
}
