// Depth frames rendered from the cloud (include/bff_hip.h: bff_render_depth_u16): a point z-buffer for scenes that come
// without sensor depth.  Every point is projected into every frame with the sweep's geometry (geom.h); a point in front
// of the camera whose pixel is in bounds splats its depth in millimetres into the texel of the (depth_h, depth_w) frame
// its pixel falls into, and a texel keeps the minimum.
//
// Data layout in HBM
//   xyz      f64 [3][n_pad]                    the sorted cloud of the sweep (a wave reads 3 x 512 B contiguous)
//   scratch  u32 [n_frames][depth_h * depth_w] all ones = empty; unsigned min by returnless vector atomics (executed at the
//                                              L2 / memory side: no read-modify-write traffic in the CUs)
//   out      u16 [n_frames][depth_h][depth_w]  millimetres, 0 = no depth: what bff_depth_tile_u16, bff_depth_from_u16 and
//                                              bff_project_views_u16 (layout 0) take
// Kernel shape: viewed_count_kernel's (project.hip): 256 threads own 1024 consecutive points, 4 per thread in registers
// across the frames of the block's frame tile, poses wave-uniform, the tile culled against tile_bounds in groups of 8
// frames.  A minimum of integers does not depend on the order of its operands: the frames are the same bytes on every run.
#include "geom.h"

namespace bff {

constexpr int kRdBlock = 256;
constexpr int kRdPPT = 4;                                          // points per thread
constexpr int kRdWordsPerBlock = (kRdBlock / kWave) * kRdPPT;      // 16 x 64 points
constexpr int kRdPtsPerBlock = kRdWordsPerBlock * kWave;           // 1024
constexpr int kRdCullGroup = 8;                                    // frames one culling pass decides
constexpr uint32_t kRdEmpty = 0xffffffffu;

__global__ __launch_bounds__(kRdBlock) void render_depth_kernel(
    const double *__restrict__ xyz, int64_t n_points, int64_t n_pad, const double *__restrict__ inv_pose, CameraK K,
    int n_frames, int frames_per_block, int H, int W, int dh, int dw, uint32_t *__restrict__ scratch,
    const double *__restrict__ tile_bounds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t word0 = (int64_t)blockIdx.x * kRdWordsPerBlock + (int64_t)wave * kRdPPT;     // the wave's first 64 points
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    const int64_t plane = (int64_t)dh * dw;
    const double dW = (double)W, dH = (double)H;

    double px[kRdPPT], py[kRdPPT], pz[kRdPPT];
    bool valid[kRdPPT];
#pragma unroll
    for (int j = 0; j < kRdPPT; ++j) {
        const int64_t n = (word0 + j) * kWave + lane;
        valid[j] = n < n_points;                                   // padding lanes never splat (they read point 0)
        const int64_t m = valid[j] ? n : 0;
        px[j] = xyz[m];
        py[j] = xyz[n_pad + m];
        pz[j] = xyz[2 * n_pad + m];
    }

    for (int g0 = f0; g0 < f1; g0 += kRdCullGroup) {
        const int g1 = min(f1, g0 + kRdCullGroup);
        uint64_t culled = 0;
        if (tile_bounds && word0 * kWave < n_points)               // wave-uniform; one box per tile that holds points
            culled = cull_frames(tile_bounds + 6 * (word0 / kRdPPT), inv_pose, K, g0, g1, lane, dW, dH);
        for (int f = g0; f < g1; ++f) {
            if ((culled >> (8 * (f - g0))) & 1) continue;          // wave-uniform
            const double *P = inv_pose + 16 * (int64_t)f;
            uint32_t *img = scratch + (int64_t)f * plane;
            int texel[kRdPPT];
            uint32_t mm[kRdPPT];
#pragma unroll
            for (int j = 0; j < kRdPPT; ++j) {
                double cz, u, v;
                camera_pixel(P, K, px[j], py[j], pz[j], cz, u, v);
                // millimetres, half to even; a surface the camera sees lies in front of it (NaN fails cz > 0)
                const double m = rint(__dmul_rn(cz, 1000.0));
                const bool splat = valid[j] && pixel_in_bounds(u, v, dW, dH) && (cz > 0.0) && (m >= 1.0) && (m <= 65535.0);
                // u < W and v < H, so tx < dw and ty < dh; W * dw and H * dh < 2^31 (checked by the entry point)
                texel[j] = splat ? (int)(((unsigned)(int)v * (unsigned)dh) / (unsigned)H) * dw +
                                   (int)(((unsigned)(int)u * (unsigned)dw) / (unsigned)W) : -1;
                mm[j] = splat ? (uint32_t)m : kRdEmpty;
            }
#pragma unroll
            for (int j = 0; j < kRdPPT; ++j)
                if (texel[j] >= 0) atomicMin(img + texel[j], mm[j]);                   // result unused: returnless
        }
    }
}

// scratch -> uint16 frames: all ones (no point splatted) becomes 0, the reference's "no depth"; four texels per thread
// when both pointers allow 16-byte loads / 8-byte stores
__global__ __launch_bounds__(256) void render_depth_narrow_kernel(const uint32_t *__restrict__ scratch, int64_t total,
                                                                   int vec_ok, uint16_t *__restrict__ out)
{
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    if (vec_ok && i + 4 <= total) {
        const uint4 s = *reinterpret_cast<const uint4 *>(scratch + i);
        ushort4 o;
        o.x = s.x == kRdEmpty ? 0 : (uint16_t)s.x;
        o.y = s.y == kRdEmpty ? 0 : (uint16_t)s.y;
        o.z = s.z == kRdEmpty ? 0 : (uint16_t)s.z;
        o.w = s.w == kRdEmpty ? 0 : (uint16_t)s.w;
        *reinterpret_cast<ushort4 *>(out + i) = o;
        return;
    }
    for (int64_t k = i; k < total && k < i + 4; ++k) {
        const uint32_t s = scratch[k];
        out[k] = s == kRdEmpty ? 0 : (uint16_t)s;
    }
}

}  // namespace bff

using namespace bff;

extern "C" int bff_render_depth_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                                    const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width,
                                    int32_t depth_h, int32_t depth_w, int32_t frames_per_block, uint32_t *scratch_u32,
                                    uint16_t *out_u16, const double *tile_bounds, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && n_pad >= n_points && n_frames >= 0 && frames_per_block >= 0, "bff_render_depth_u16: bad sizes");
    BFF_REQUIRE(height > 0 && width > 0 && depth_h > 0 && depth_w > 0, "bff_render_depth_u16: bad image size");
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "bff_render_depth_u16: image larger than 2^31 pixels");
    BFF_LIMIT((int64_t)depth_h * depth_w < (1ll << 31), "bff_render_depth_u16: depth frame larger than 2^31 texels");
    BFF_LIMIT((int64_t)height * depth_h < (1ll << 31) && (int64_t)width * depth_w < (1ll << 31),
              "bff_render_depth_u16: pixel x texel products beyond 2^31 (height * depth_h, width * depth_w)");
    BFF_LIMIT(n_frames <= 65535, "bff_render_depth_u16: too many frames");
    const int64_t gx = ceil_div(n_points, kRdPtsPerBlock);
    const int64_t n_narrow = ceil_div(ceil_div((int64_t)n_frames * depth_h * depth_w, 4), 256);
    BFF_LIMIT(gx < (1ll << 31) && n_narrow < (1ll << 31), "bff_render_depth_u16: too many points / texels for one launch");
    if (n_frames == 0) return BFF_OK;
    BFF_REQUIRE(out_u16, "bff_render_depth_u16: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t total = (int64_t)n_frames * depth_h * depth_w;
    if (n_points == 0) {                                             // nothing splats: every texel is "no depth"
        hipError_t e = hipMemsetAsync(out_u16, 0, sizeof(uint16_t) * (size_t)total, st);
        if (e != hipSuccess) return fail((int)e, "bff_render_depth_u16: memset: %s", hipGetErrorString(e));
        return BFF_OK;
    }
    BFF_REQUIRE(xyz && inv_pose && cam_intr_host && scratch_u32, "bff_render_depth_u16: null pointer");
    hipError_t e = hipMemsetAsync(scratch_u32, 0xff, sizeof(uint32_t) * (size_t)total, st);
    if (e != hipSuccess) return fail((int)e, "bff_render_depth_u16: memset: %s", hipGetErrorString(e));
    CameraK K;
    for (int i = 0; i < 9; ++i) K.k[i] = cam_intr_host[i];
    // the culling table's tiles are the sweep's (bff_point_tile_bounds): they must be this kernel's waves
    BFF_REQUIRE(!tile_bounds || bff_point_tile_size() == kRdPPT * kWave, "bff_render_depth_u16: tile_bounds holds tiles of %d "
                "points, the renderer's waves own %d", bff_point_tile_size(), kRdPPT * kWave);
    int fpb = frames_per_block;
    if (fpb == 0) {                                                  // >= ~4096 blocks in flight, tiles of up to 8 frames
        fpb = (int)((int64_t)n_frames * gx / 4096);
        fpb = fpb < 1 ? 1 : (fpb > kRdCullGroup ? kRdCullGroup : fpb);
    }
    dim3 grid((unsigned)gx, (unsigned)ceil_div(n_frames, fpb));
    render_depth_kernel<<<grid, kRdBlock, 0, st>>>(xyz, n_points, n_pad, inv_pose, K, n_frames, fpb, height, width, depth_h,
                                                   depth_w, scratch_u32, tile_bounds);
    int rc = launched("bff_render_depth_u16");
    if (rc != BFF_OK) return rc;
    const int vec_ok = (reinterpret_cast<uintptr_t>(scratch_u32) % 16 == 0) && (reinterpret_cast<uintptr_t>(out_u16) % 8 == 0);
    render_depth_narrow_kernel<<<(unsigned)n_narrow, 256, 0, st>>>(scratch_u32, total, vec_ok, out_u16);
    return launched("bff_render_depth_u16");
}
