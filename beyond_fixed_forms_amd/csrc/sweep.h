// What the sweep kernels share (project.hip, visibility.hip, diag.hip; the block shape also sweep_runs.hip): the block
// shape, how a depth frame is read at a pixel -- the one statement of the depth read -- and the depth test.  The storage of
// the frames and the tap table are depth.hip's.
#pragma once

#include "geom.h"
#include "mask_rows.h"

namespace bff {

// 256 threads = 4 waves own 1024 consecutive points (16 row words = one 128-B line per row); wave w owns the 4 consecutive
// words 4w..4w+3 of that line (its 32-B sector), 4 points per thread kept in registers across the frames of a frame tile
constexpr int kBlock = 256;
constexpr int kPPT = 4;                          // points per thread
constexpr int kWordsPerBlock = (kBlock / kWave) * kPPT;   // 16 row words per block
constexpr int kPtsPerBlock = kWordsPerBlock * kWave;       // 1024

// Depth kept as the PNGs store it (P:431-436): uint16 millimetres at the sensor's resolution.  The sweep then evaluates
// `astype(f32) / 1000` and the two 2-tap passes of the bilinear resize to (H, W) PER POINT, at the pixel the point
// projects to, with exactly the float32 operations of depth_resize_kernel (depth.hip) / io.resize_bilinear_f32 -- the
// (H, W) float image (8x the bytes of the source) is never built.  hs == H and ws == W: the resize is the identity.
struct RawDepth {
    const uint32_t *taps;       // device table of the resize, 3 words per destination column then per destination row:
                                //   column u: (texel offset of its left tap inside a source row, of its right tap, fraction bits)
                                //   row v:    (texel offset of its upper source row, of its lower one, fraction bits)
                                // a tap's texel = row offset + column offset; offsets follow the frames' layout (row-major,
                                // or 8 x 8-texel tiles: ((y >> 3) * tw + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)); fractions and
                                // tap indices as io._axis_taps (sensor_taps_kernel, depth.hip)
    int n_taps;                 // W + H
    int texel_f32;              // frames hold float32 metres (`astype(f32) / 1000` done once per texel at ingestion) instead of
                                // the uint16 millimetres themselves
    int64_t frame_stride;       // texels per frame (padded to whole tiles when tiled)
    float scale;                // 1000
};

// The per-scene visibility table (bff_visibility_table): what the sweep's geometry and depth test answer per (depth slot,
// point), kept from call to call -- the answer depends on the cloud, the poses, the depth frames and the threshold only.
//   mask  [n_slots][stride]  bit l of word w: point 64 w + l passes the sweep's test in the slot's frame
//   off   [n_slots][stride]  exclusive prefix of the words' popcounts in (slot, word) order
//   pix   the visible pairs' pixels, u | v << 16, pair (slot, w, l) at off[slot][w] + popcount(mask & lanes below l)
// stride = bff_visibility_words(n_points): the words of whole sweep blocks, so that every wave of a sweep finds its four.
struct VisTable {
    const uint64_t *mask;
    const uint32_t *off;
    const uint32_t *pix;
    int64_t stride;
};

// Host side of a raw-depth launch (depth.hip): `r` from the frames' layout (0 uint16 row-major frames as stored, 1 uint16
// in 8 x 8 tiles, 2 float32 metres in 8 x 8 tiles) and sizes, its tap table built on first use.  lds_bytes (null: the
// caller reads the table in place): the bytes a block's copy of the table takes, refused with lds_msg beyond 48 KB.
int raw_depth_launch(int32_t depth_h, int32_t depth_w, int32_t height, int32_t width, int32_t layout, hipStream_t st,
                     RawDepth *r, size_t *lds_bytes = nullptr, const char *lds_msg = nullptr);

// bff_profile_next_sweep's events (project.hip), taken by the next sweep dispatch of this host thread: both null afterwards
void take_sweep_events(hipEvent_t *start, hipEvent_t *stop);

__device__ __forceinline__ void lds_phase_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The block's copy of RawDepth::taps in LDS: two LDS reads per axis replace ~25 instructions per point.  16 bytes per
// load (the table is padded to whole uint4), a thread's loads independent of each other: the fill costs a block one
// memory latency (word by word it was ~27 dependent round trips: +330 us on config 4's 73 k blocks).  Ends in a barrier.
__device__ __forceinline__ void fill_lds_taps(uint32_t *s_taps, const RawDepth &raw)
{
    const int n_vec = (3 * raw.n_taps + 3) / 4;
    const uint4 *src = reinterpret_cast<const uint4 *>(raw.taps);
    uint4 *dst = reinterpret_cast<uint4 *>(s_taps);
    for (int i = (int)threadIdx.x; i < n_vec; i += kBlock) dst[i] = src[i];
    __syncthreads();
}

// the frame in slot `slot` of a raw-depth array
__device__ __forceinline__ const char *raw_frame(const void *depth, int64_t slot, const RawDepth &r)
{
    return reinterpret_cast<const char *>(depth) + slot * r.frame_stride * (r.texel_f32 ? 4 : 2);
}

// one source texel in metres: float32 frames hold it, uint16 frames hold millimetres (P:432-435: astype(f32) / 1000)
__device__ __forceinline__ float sensor_texel(const void *frame, uint32_t t, const RawDepth &r)
{
    return r.texel_f32 ? reinterpret_cast<const float *>(frame)[t]
                       : __fdiv_rn((float)reinterpret_cast<const uint16_t *>(frame)[t], r.scale);
}

// the four source texels of pixel (u, v) -- two distinct ones when the sizes agree -- and the resize's two fractions
struct PixelTaps {
    uint32_t t00, t01, t10, t11;                 // texel offsets inside the frame: upper left, upper right, lower left, lower right
    float a, b;                                  // fraction along x, along y
};
struct PixelTexels { float s00, s01, s10, s11, a, b; };

__device__ __forceinline__ PixelTaps pixel_taps(const uint32_t *taps, int W, int u, int v)
{
    const uint32_t *tx = taps + 3 * u, *ty = taps + 3 * (W + v);
    const uint32_t c0 = tx[0], c1 = tx[1], r0 = ty[0], r1 = ty[1];
    return {r0 + c0, r0 + c1, r1 + c0, r1 + c1, __uint_as_float(tx[2]), __uint_as_float(ty[2])};
}

// the gathers of one pixel: nothing here waits for a load, so a caller that fetches several pixels before it looks at any
// has all their texels in flight together
__device__ __forceinline__ PixelTexels fetch_texels(const uint32_t *s_taps, int W, int u, int v, const void *frame, const RawDepth &r)
{
    const PixelTaps p = pixel_taps(s_taps, W, u, v);
    return {sensor_texel(frame, p.t00, r), sensor_texel(frame, p.t01, r), sensor_texel(frame, p.t10, r),
            sensor_texel(frame, p.t11, r), p.a, p.b};
}

// the resized depth value at one pixel from its four source texels: the horizontal 2-tap pass on both rows, then the
// vertical one (io.resize_bilinear_f32's float32 operation order)
__device__ __forceinline__ float bilinear_depth(float s00, float s01, float s10, float s11, float a, float b)
{
    const float one_a = __fsub_rn(1.0f, a), one_b = __fsub_rn(1.0f, b);
    const float r0 = __fadd_rn(__fmul_rn(s00, one_a), __fmul_rn(s01, a));
    const float r1 = __fadd_rn(__fmul_rn(s10, one_a), __fmul_rn(s11, a));
    return __fadd_rn(__fmul_rn(r0, one_b), __fmul_rn(r1, b));
}
__device__ __forceinline__ float bilinear_depth(const PixelTexels &t) { return bilinear_depth(t.s00, t.s01, t.s10, t.s11, t.a, t.b); }

// the depth test: the frame has a measurement at the pixel and the point's camera z is within thresh of it
__device__ __forceinline__ bool depth_visible(double cz, float d, double thresh)
{
    return (d != 0.0f) && (fabs(cz - (double)d) < thresh);
}

}  // namespace bff
