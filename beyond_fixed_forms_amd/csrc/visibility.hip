// The sweep's visibility answer without masks: the detection-ratio pass (bff_count_viewed, a15) and the per-scene
// visibility table built from it (bff_visibility_table), which the cached sweeps (project.hip, sweep_runs.hip) read.
#include <atomic>

#include "sweep.h"

namespace bff {

// The detection-ratio sweep alone (P:538-567): viewed_count[n] += visible(n, f) for every frame of the list.  Per (point,
// frame) exactly the arithmetic of project_views_kernel -- both call camera_pixel / pixel_in_bounds (geom.h) and the depth
// read and test of sweep.h -- so the counts are the ones the fused sweep adds under frame flag bit 0.  Same block
// shape (1024 points, 4 per thread in registers, frames tiled over blockIdx.y); without masks there are no gathers of
// mask words, no ballot transposition and no row stores, so a block takes a longer frame tile (fewer atomics per point):
// the tile is culled against tile_bounds in groups of 8 frames, the fused sweep's exact test.
constexpr int kCullGroup = 8;                    // frames one culling pass decides (lane = 8 frame + corner)

// kBits: the mask pass of bff_visibility_table.  The frames are the scene's depth slots (frame f reads depth slot f), and
// instead of counting, the ballot of `visible` over the wave's 64 points is stored per word: vis_mask[f][word].
template <bool kRaw, bool kBits = false>
__global__ __launch_bounds__(kBlock) void viewed_count_kernel(
    const double *__restrict__ xyz, int64_t n_points, int64_t n_pad,
    const double *__restrict__ inv_pose, CameraK K, int n_frames, int frames_per_block,
    const void *__restrict__ depth, RawDepth raw, const int32_t *__restrict__ depth_index, int H, int W, double thresh,
    int32_t *__restrict__ viewed_count, const double *__restrict__ tile_bounds,
    uint64_t *__restrict__ vis_mask = nullptr, int64_t vis_stride = 0)
{
    extern __shared__ uint32_t s_taps[];
    if (kRaw) fill_lds_taps(s_taps, raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t word0 = (int64_t)blockIdx.x * kWordsPerBlock + (int64_t)wave * kPPT;
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    const int64_t hw = (int64_t)H * W;
    const double dW = (double)W, dH = (double)H;

    double px[kPPT], py[kPPT], pz[kPPT];
    bool valid[kPPT];
    int vcount[kPPT];
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int64_t n = (word0 + j) * kWave + lane;
        valid[j] = n < n_points;
        const int64_t m = valid[j] ? n : 0;
        px[j] = xyz[m];
        py[j] = xyz[n_pad + m];
        pz[j] = xyz[2 * n_pad + m];
        vcount[j] = 0;
    }

    for (int g0 = f0; g0 < f1; g0 += kCullGroup) {
        const int g1 = min(f1, g0 + kCullGroup);
        // frustum culling of the wave's 256 points against the <= 8 frames [g0, g1) (geom.h: exact)
        uint64_t culled = 0;
        if (tile_bounds && word0 * kWave < n_points)       // wave-uniform; the table has one box per tile that holds points
            culled = cull_frames(tile_bounds + 6 * (word0 / kPPT), inv_pose, K, g0, g1, lane, dW, dH);
        for (int f = g0; f < g1; ++f) {
            if ((culled >> (8 * (f - g0))) & 1) continue;      // wave-uniform
            const double *P = inv_pose + 16 * (int64_t)f;
            const int64_t slot = kBits ? f : depth_index[f];
            const float *dimg = kRaw ? nullptr : reinterpret_cast<const float *>(depth) + slot * hw;
            const char *rimg = kRaw ? raw_frame(depth, slot, raw) : nullptr;
            // the fused sweep's three phases: geometry of the 4 points, all gathers in flight together, then the test
            int pix[kPPT], pu[kPPT];
            double cz[kPPT];
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                double u, v;
                camera_pixel(P, K, px[j], py[j], pz[j], cz[j], u, v);
                const bool inb = valid[j] && pixel_in_bounds(u, v, dW, dH);
                pix[j] = inb ? (int)v * W + (int)u : -1;
                pu[j] = inb ? (int)u | ((int)v << 16) : 0;
            }
            float dval[kPPT];
            PixelTexels tex[kPPT];
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                dval[j] = 0.0f;
                if (kRaw) tex[j] = PixelTexels{};
                if (pix[j] >= 0) {
                    if (kRaw) tex[j] = fetch_texels(s_taps, W, pu[j] & 0xffff, pu[j] >> 16, rimg, raw);
                    else dval[j] = dimg[pix[j]];
                }
            }
            if (kRaw) {
#pragma unroll
                for (int j = 0; j < kPPT; ++j)
                    if (pix[j] >= 0) dval[j] = bilinear_depth(tex[j]);
            }
            uint64_t mine = 0;                              // kBits: lane j keeps the ballot of word j
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                const bool vis = (pix[j] >= 0) && depth_visible(cz[j], dval[j], thresh);
                vcount[j] += vis ? 1 : 0;
                if constexpr (kBits) {
                    const uint64_t bal = __ballot(vis);
                    if (lane == j) mine = bal;
                }
            }
            // the wave's 32-B sector of the slot's mask row; vis_stride holds the words of whole blocks (a culled frame
            // keeps the zeros the caller filled in)
            if constexpr (kBits)
                if (lane < kPPT) vis_mask[slot * vis_stride + word0 + lane] = mine;
        }
    }
    if constexpr (!kBits) {
#pragma unroll
        for (int j = 0; j < kPPT; ++j) {
            const int64_t n = (word0 + j) * kWave + lane;
            if (valid[j] && vcount[j]) atomicAdd(viewed_count + n, vcount[j]);
        }
    }
}

// Visibility table, step 2: off[i] = number of set bits in mask[0 .. i), total[0] = all of them.  One block walks the
// words 4096 at a time (thread t: words 4 t .. 4 t + 3 of the piece, 32 contiguous bytes) with a running carry; n is a
// multiple of 4.  The table is built once per resident scene, so one block's pace (~0.5 us per piece) is enough.
constexpr int kScanBlock = 1024;

__global__ __launch_bounds__(kScanBlock) void vis_offsets_kernel(const uint64_t *__restrict__ mask, int64_t n,
                                                                 uint32_t *__restrict__ off, uint64_t *__restrict__ total)
{
    __shared__ uint32_t s_wave[kScanBlock / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;
    for (int64_t base = 0; base < n; base += 4 * kScanBlock) {
        const int64_t i = base + 4 * tid;
        uint32_t c[4] = {0, 0, 0, 0};
        if (i < n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = (uint32_t)__popcll(mask[i + q]);
        }
        const uint32_t sum = c[0] + c[1] + c[2] + c[3];
        uint32_t inc = sum;                                    // inclusive scan over the wave, then over the 16 waves
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == kWave - 1) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0, piece = 0;
#pragma unroll
        for (int w = 0; w < kScanBlock / kWave; ++w) {
            const uint32_t t = s_wave[w];
            before += w < wave ? t : 0;
            piece += t;
        }
        __syncthreads();                                       // s_wave is rewritten by the next piece
        if (i < n) {
            uint32_t at = (uint32_t)carry + before + inc - sum;    // 32-bit offsets: the entry point refuses 2^32 pairs
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                off[i + q] = at;
                at += c[q];
            }
        }
        carry += piece;
    }
    if (tid == 0) total[0] = carry;
}

// Visibility table, step 3: the pixels of the visible pairs.  One wave per (slot, word) with a non-zero mask word; a
// lane whose bit is set repeats the sweep's geometry for its point (camera_pixel: the pixel the mask pass tested) and
// stores it at the pair's place.  No depth access.
__global__ __launch_bounds__(kBlock) void vis_pixels_kernel(const double *__restrict__ xyz, int64_t n_pad,
                                                            const double *__restrict__ inv_pose, CameraK K,
                                                            const uint64_t *__restrict__ mask, const uint32_t *__restrict__ off,
                                                            int64_t stride, uint32_t *__restrict__ pixels, int64_t pix_cap)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int slot = blockIdx.y;
    if (w >= stride) return;
    const uint64_t m = mask[slot * stride + w];
    if (!((m >> lane) & 1)) return;
    const int64_t n = w * kWave + lane;                        // a set bit is a valid point
    double cz, u, v;
    camera_pixel(inv_pose + 16 * (int64_t)slot, K, xyz[n], xyz[n_pad + n], xyz[2 * n_pad + n], cz, u, v);
    const int64_t at = (int64_t)off[slot * stride + w] + __popcll(m & ((1ull << lane) - 1));
    if (at < pix_cap) pixels[at] = (uint32_t)(int)u | ((uint32_t)(int)v << 16);
}

}  // namespace bff

using namespace bff;

extern "C" int bff_count_viewed(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                                const double *cam_intr_host, int32_t n_frames, const void *depth, int32_t depth_h,
                                int32_t depth_w, int32_t depth_layout, const int32_t *depth_index, int32_t height,
                                int32_t width, double depth_thresh, int32_t frames_per_block, int32_t *viewed_count,
                                const double *tile_bounds, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && n_pad >= n_points && n_frames >= 0 && frames_per_block >= 0, "bff_count_viewed: bad sizes");
    BFF_REQUIRE(height > 0 && width > 0, "bff_count_viewed: bad image size");
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "bff_count_viewed: image larger than 2^31 pixels");
    BFF_REQUIRE(depth_layout >= -1 && depth_layout <= 2, "bff_count_viewed: depth_layout must be -1, 0, 1 or 2");
    if (n_points == 0 || n_frames == 0) return BFF_OK;
    BFF_REQUIRE(xyz && inv_pose && cam_intr_host && depth && depth_index && viewed_count, "bff_count_viewed: null pointer");
    hipStream_t st = as_stream(stream);
    RawDepth rd{};
    size_t taps_bytes = 0;
    if (depth_layout >= 0) {
        BFF_LIMIT(height < (1 << 15) && width < (1 << 16), "bff_count_viewed: image too large");
        const int rc = raw_depth_launch(depth_h, depth_w, height, width, depth_layout, st, &rd, &taps_bytes,
                                        "bff_count_viewed: the resize's tap table exceeds 48 KB of LDS: resize in a separate "
                                        "pass (bff_depth_from_u16)");
        if (rc != BFF_OK) return rc;
    }
    const CameraK K = camera_k(cam_intr_host);
    const int64_t gx = ceil_div(n_points, kPtsPerBlock);
    int fpb = frames_per_block;
    if (fpb == 0) fpb = bff_sweep_frames_per_block(n_points, n_frames);     // c2, 300 frames: 16 and 32 are slower
    BFF_LIMIT(ceil_div(n_frames, fpb) <= 65535, "bff_count_viewed: too many frame tiles");
    dim3 grid((unsigned)gx, (unsigned)ceil_div(n_frames, fpb));
    if (depth_layout >= 0)
        viewed_count_kernel<true><<<grid, kBlock, (unsigned)taps_bytes, st>>>(xyz, n_points, n_pad, inv_pose, K, n_frames, fpb,
            depth, rd, depth_index, height, width, depth_thresh, viewed_count, tile_bounds);
    else
        viewed_count_kernel<false><<<grid, kBlock, 0, st>>>(xyz, n_points, n_pad, inv_pose, K, n_frames, fpb,
            depth, rd, depth_index, height, width, depth_thresh, viewed_count, tile_bounds);
    return launched("bff_count_viewed");
}

extern "C" int64_t bff_visibility_words(int64_t n_points)
{
    return n_points <= 0 ? 0 : ceil_div(n_points, (int64_t)kPtsPerBlock) * kWordsPerBlock;
}

extern "C" int bff_visibility_table_bytes(int64_t n_points, int32_t n_slots, int64_t n_pixels, int64_t *bytes)
{
    BFF_REQUIRE(n_points >= 0 && n_slots >= 0 && n_pixels >= 0 && bytes, "bff_visibility_table_bytes: bad arguments");
    const int64_t entries = bff_visibility_words(n_points) * n_slots;
    bytes[0] = (int64_t)sizeof(uint64_t) * entries;
    bytes[1] = (int64_t)sizeof(uint32_t) * entries;
    bytes[2] = (int64_t)sizeof(uint32_t) * n_pixels;
    return BFF_OK;
}

static std::atomic<int64_t> g_vis_builds{0};

extern "C" int64_t bff_visibility_builds(void) { return g_vis_builds.load(); }

extern "C" int bff_visibility_table(const double *xyz, int64_t n_points, int64_t n_pad, const double *slot_inv_pose,
                                    const double *cam_intr_host, int32_t n_slots, const void *depth, int32_t depth_h,
                                    int32_t depth_w, int32_t depth_layout, int32_t height, int32_t width,
                                    double depth_thresh, const double *tile_bounds, uint64_t *vis_mask, uint32_t *vis_off,
                                    uint32_t *vis_pix, int64_t pix_cap, uint64_t *n_pixels, int32_t phase, void *stream)
{
    BFF_REQUIRE(n_points >= 0 && n_pad >= n_points && n_slots >= 0 && pix_cap >= 0 && phase >= 0 && phase <= 2,
                "bff_visibility_table: bad sizes");
    BFF_REQUIRE(height > 0 && width > 0, "bff_visibility_table: bad image size");
    BFF_LIMIT(height < (1 << 15) && width < (1 << 15), "bff_visibility_table: image too large for packed pixels");
    BFF_REQUIRE(depth_layout >= -1 && depth_layout <= 2, "bff_visibility_table: depth_layout must be -1, 0, 1 or 2");
    BFF_LIMIT(n_slots <= 65535, "bff_visibility_table: too many depth slots");
    if (n_points == 0 || n_slots == 0) return BFF_OK;
    BFF_REQUIRE(xyz && slot_inv_pose && cam_intr_host && vis_mask && vis_off && n_pixels, "bff_visibility_table: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t stride = bff_visibility_words(n_points), entries = stride * n_slots;
    const CameraK K = camera_k(cam_intr_host);
    if (phase != 2) {
        BFF_REQUIRE(depth, "bff_visibility_table: null pointer");
        RawDepth rd{};
        size_t taps_bytes = 0;
        if (depth_layout >= 0) {
            const int rc = raw_depth_launch(depth_h, depth_w, height, width, depth_layout, st, &rd, &taps_bytes,
                                            "bff_visibility_table: the resize's tap table exceeds 48 KB of LDS");
            if (rc != BFF_OK) return rc;
        }
        hipError_t e = hipMemsetAsync(vis_mask, 0, sizeof(uint64_t) * (size_t)entries, st);     // culled frames store nothing
        if (e != hipSuccess) return fail((int)e, "bff_visibility_table: memset: %s", hipGetErrorString(e));
        // 1: the mask pass, bff_count_viewed's kernel with the ballots as output
        const int fpb = bff_sweep_frames_per_block(n_points, n_slots);
        dim3 grid((unsigned)ceil_div(n_points, kPtsPerBlock), (unsigned)ceil_div(n_slots, fpb));
        if (depth_layout >= 0)
            viewed_count_kernel<true, true><<<grid, kBlock, (unsigned)taps_bytes, st>>>(xyz, n_points, n_pad, slot_inv_pose, K,
                n_slots, fpb, depth, rd, nullptr, height, width, depth_thresh, nullptr, tile_bounds, vis_mask, stride);
        else
            viewed_count_kernel<false, true><<<grid, kBlock, 0, st>>>(xyz, n_points, n_pad, slot_inv_pose, K,
                n_slots, fpb, depth, rd, nullptr, height, width, depth_thresh, nullptr, tile_bounds, vis_mask, stride);
        // 2: the offsets
        vis_offsets_kernel<<<1, kScanBlock, 0, st>>>(vis_mask, entries, vis_off, n_pixels);
        const int rc = launched("bff_visibility_table");
        if (rc != BFF_OK) return rc;
    }
    if (phase != 1) {
        // 3: the pixels
        BFF_REQUIRE(vis_pix || pix_cap == 0, "bff_visibility_table: null pointer");
        BFF_LIMIT(pix_cap < (1ll << 32), "bff_visibility_table: more than 2^32 visible pairs");
        dim3 grid((unsigned)ceil_div(stride, kBlock / kWave), (unsigned)n_slots);
        vis_pixels_kernel<<<grid, kBlock, 0, st>>>(xyz, n_pad, slot_inv_pose, K, vis_mask, vis_off, stride, vis_pix, pix_cap);
        g_vis_builds.fetch_add(1);
        return launched("bff_visibility_table");
    }
    return BFF_OK;
}
