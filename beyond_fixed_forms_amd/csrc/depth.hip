// How a depth frame is stored and read: raw 16-bit depth -> float32 (H, W) images
// (bff_depth_from_u16), or kept at the sensor's resolution -- row-major or in 8 x 8 tiles (bff_depth_tile_u16) -- and
// resized per point by the sweep through a tap table (sweep.h: RawDepth).
#include <map>
#include <mutex>
#include <tuple>

#include "sweep.h"

namespace bff {

// io._axis_taps for one destination index: f = (float)((d + 0.5) * scale - 0.5) (float64 products and differences, each
// rounded once; no contraction), i0 = floor(f), a = f - i0 in float32; x axis: border columns are copied (a = 0), y axis:
// the fraction is kept and the two row indices are clamped.
template <bool kX>
__device__ __forceinline__ void axis_tap(int d, double scale, int n_src, int &i0, int &i1, float &a)
{
    const float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    const float fl = floorf(f);
    int s = (int)fl;
    a = __fsub_rn(f, fl);
    if (kX) {
        if (s < 0) { s = 0; a = 0.0f; }
        else if (s >= n_src - 1) { s = n_src - 1; a = 0.0f; }
        i0 = s;
        i1 = min(s + 1, n_src - 1);
    } else {
        i1 = min(max(s + 1, 0), n_src - 1);
        i0 = min(max(s, 0), n_src - 1);
    }
}

// the table RawDepth::taps points to, for source frames of hs x ws texels resized to H x W (tiled != 0: tile layout)
__global__ void sensor_taps_kernel(int hs, int ws, int H, int W, int tiled, double sx, double sy, uint32_t *__restrict__ table)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W + H) return;
    const int tw = (ws + 7) / 8;
    int i0, i1;
    float a;
    uint32_t p0, p1;
    if (i < W) {
        axis_tap<true>(i, sx, ws, i0, i1, a);
        p0 = tiled ? (uint32_t)((i0 >> 3) * 64 + (i0 & 7)) : (uint32_t)i0;
        p1 = tiled ? (uint32_t)((i1 >> 3) * 64 + (i1 & 7)) : (uint32_t)i1;
    } else {
        axis_tap<false>(i - W, sy, hs, i0, i1, a);
        p0 = tiled ? (uint32_t)((i0 >> 3) * tw * 64 + (i0 & 7) * 8) : (uint32_t)(i0 * ws);
        p1 = tiled ? (uint32_t)((i1 >> 3) * tw * 64 + (i1 & 7) * 8) : (uint32_t)(i1 * ws);
    }
    table[3 * i] = p0;
    table[3 * i + 1] = p1;
    table[3 * i + 2] = __float_as_uint(a);
}

// uint16 frames [n][hs][ws] -> 8 x 8-texel tiles, [n][ceil(hs/8)][ceil(ws/8)][8][8] (padding texels 0): the 64 points of a
// wave project onto a compact patch of a frame, and the four taps of a point are neighbours in BOTH directions -- in
// tiles they touch a fraction of the 128-byte lines that row-major frames make them touch.  out_f32: the tiles hold
// float32 metres, `astype(float32) / 1000` of P:432-435 done here once per texel instead of four times per (point, frame).
template <typename OutT>
__global__ void depth_tile_kernel(const uint16_t *__restrict__ src, int hs, int ws, int th, int tw, OutT *__restrict__ dst, float scale)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // one destination texel
    const int64_t per_frame = (int64_t)th * tw * 64;
    if (t >= per_frame) return;
    const int f = blockIdx.y;
    const int tile = (int)(t >> 6), in = (int)(t & 63);
    const int y = (tile / tw) * 8 + (in >> 3), x = (tile % tw) * 8 + (in & 7);
    const uint16_t v = (y < hs && x < ws) ? src[((int64_t)f * hs + y) * ws + x] : (uint16_t)0;
    if constexpr (sizeof(OutT) == 4) dst[(int64_t)f * per_frame + t] = __fdiv_rn((float)v, scale);
    else dst[(int64_t)f * per_frame + t] = v;
}

// Depth ingestion: raw 16-bit depth (millimetres, source resolution) -> float32 metres at (H, W): `png.astype(f32) / 1000`
// followed by the 2-tap horizontal then vertical passes of a bilinear resize with half-pixel centres and
// edge clamp (reference P:432-436 does this with cv2.imread + cv2.resize; restated on the host in
// io.resize_bilinear_f32, to which this kernel is bit-identical: same float32 operation order, tap tables
// computed by the host in float64).  One thread per output pixel; the 4 source texels are L2-resident.
__global__ void depth_resize_kernel(const uint16_t *__restrict__ src, int hs, int ws, int n_frames,
                                    const int32_t *__restrict__ x0, const int32_t *__restrict__ x1,
                                    const float *__restrict__ ax, const int32_t *__restrict__ y0,
                                    const int32_t *__restrict__ y1, const float *__restrict__ ay, int H, int W,
                                    float scale, float *__restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= W) return;
    const uint16_t *img = src + (int64_t)f * hs * ws;
    const int xa = x0[x], xb = x1[x], ya = y0[y], yb = y1[y];
    auto texel = [&](int yy, int xx) { return __fdiv_rn((float)img[(int64_t)yy * ws + xx], scale); };
    dst[((int64_t)f * H + y) * W + x] = bilinear_depth(texel(ya, xa), texel(ya, xb), texel(yb, xa), texel(yb, xb), ax[x], ay[y]);
}

__global__ void depth_scale_kernel(const uint16_t *__restrict__ src, int64_t n, float scale, float *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = __fdiv_rn((float)src[i], scale);
}

}  // namespace bff

using namespace bff;

extern "C" int64_t bff_depth_tiled_texels(int32_t h_src, int32_t w_src)
{
    return (int64_t)((h_src + 7) / 8) * ((w_src + 7) / 8) * 64;
}

extern "C" int bff_depth_tile_u16(const uint16_t *src, int32_t n_frames, int32_t h_src, int32_t w_src, void *dst,
                                  int32_t out_f32, void *stream)
{
    BFF_REQUIRE(n_frames >= 0 && h_src > 0 && w_src > 0, "bff_depth_tile_u16: bad sizes");
    if (n_frames == 0) return BFF_OK;
    BFF_REQUIRE(src && dst, "bff_depth_tile_u16: null pointer");
    BFF_LIMIT(n_frames <= 65535, "bff_depth_tile_u16: too many frames");
    const int th = (h_src + 7) / 8, tw = (w_src + 7) / 8;
    dim3 grid((unsigned)ceil_div((int64_t)th * tw * 64, 256), (unsigned)n_frames);
    if (out_f32)
        depth_tile_kernel<float><<<grid, 256, 0, as_stream(stream)>>>(src, h_src, w_src, th, tw, (float *)dst, 1000.0f);
    else
        depth_tile_kernel<uint16_t><<<grid, 256, 0, as_stream(stream)>>>(src, h_src, w_src, th, tw, (uint16_t *)dst, 1000.0f);
    return launched("bff_depth_tile_u16");
}

// The resize's tap table for one combination of sizes and layout lives on the device for the rest of the process (a few
// tens of KB each, a handful of combinations): built on first use, synchronously, so that every later call on any stream
// finds it complete.
static int sensor_taps(int hs, int ws, int H, int W, int tiled, hipStream_t st, const uint32_t **out)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int, int, int>, uint32_t *> cache;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail((int)e, "bff_project_views_u16: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(dev, hs, ws, H, W, tiled);
    auto it = cache.find(key);
    if (it == cache.end()) {
        uint32_t *table = nullptr;
        e = hipMalloc(reinterpret_cast<void **>(&table), sizeof(uint32_t) * (3 * (size_t)(W + H) + 4));     // read as whole uint4
        if (e != hipSuccess) return fail((int)e, "bff_project_views_u16: tap table: %s", hipGetErrorString(e));
        const double sx = 1.0 / ((double)W / (double)ws), sy = 1.0 / ((double)H / (double)hs);     // io._axis_taps: 1 / (n_dst / n_src)
        sensor_taps_kernel<<<(unsigned)ceil_div(W + H, 256), 256, 0, st>>>(hs, ws, H, W, tiled, sx, sy, table);
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(table); return fail((int)e, "bff_project_views_u16: tap table: %s", hipGetErrorString(e)); }
        it = cache.emplace(key, table).first;
    }
    *out = it->second;
    return BFF_OK;
}

int bff::raw_depth_launch(int32_t depth_h, int32_t depth_w, int32_t height, int32_t width, int32_t layout, hipStream_t st,
                          RawDepth *r, size_t *lds_bytes, const char *lds_msg)
{
    BFF_REQUIRE(layout >= 0 && layout <= 2 && depth_h > 0 && depth_w > 0, "bff_project_views_u16: bad depth layout / size");
    const int tiled = layout != 0;
    r->n_taps = width + height;
    r->texel_f32 = layout == 2;
    r->frame_stride = tiled ? bff_depth_tiled_texels(depth_h, depth_w) : (int64_t)depth_h * depth_w;
    r->scale = 1000.0f;                                                 // depth_scale, hard-coded at P:346
    BFF_LIMIT(r->frame_stride < (1ll << 31), "bff_project_views_u16: depth frame too large");
    if (lds_bytes) {
        *lds_bytes = sizeof(uint32_t) * ((3 * (size_t)r->n_taps + 3) / 4 * 4);
        BFF_LIMIT(*lds_bytes <= 48 * 1024, "%s", lds_msg);
    }
    return sensor_taps(depth_h, depth_w, height, width, tiled, st, &r->taps);
}

extern "C" int bff_depth_from_u16(const uint16_t *src, int32_t n_frames, int32_t h_src, int32_t w_src,
                                  const int32_t *x0, const int32_t *x1, const float *ax,
                                  const int32_t *y0, const int32_t *y1, const float *ay,
                                  int32_t height, int32_t width, float depth_scale, float *dst, void *stream)
{
    BFF_REQUIRE(n_frames >= 0 && h_src > 0 && w_src > 0 && height > 0 && width > 0 && depth_scale > 0,
                "bff_depth_from_u16: bad sizes");
    if (n_frames == 0) return BFF_OK;
    BFF_REQUIRE(src && dst, "bff_depth_from_u16: null pointer");
    if (h_src == height && w_src == width) {       // cv2.resize to the same size is the identity
        const int64_t n = (int64_t)n_frames * height * width;
        depth_scale_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, as_stream(stream)>>>(src, n, depth_scale, dst);
        return launched("bff_depth_from_u16");
    }
    BFF_REQUIRE(x0 && x1 && ax && y0 && y1 && ay, "bff_depth_from_u16: tap tables required when resizing");
    BFF_LIMIT(height <= 65535 && n_frames <= 65535, "bff_depth_from_u16: grid limits");
    dim3 grid((unsigned)ceil_div(width, 256), (unsigned)height, (unsigned)n_frames);
    depth_resize_kernel<<<grid, 256, 0, as_stream(stream)>>>(src, h_src, w_src, n_frames, x0, x1, ax, y0, y1, ay, height,
                                                             width, depth_scale, dst);
    return launched("bff_depth_from_u16");
}
