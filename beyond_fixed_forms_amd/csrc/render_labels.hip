// 3-D instances rendered back into the views (include/bff_hip.h: bff_point_labels, bff_render_labels_u16,
// bff_label_runs_count / bff_label_runs_emit): instance bit rows -> one label per point -> a z-buffer that carries the
// label next to the depth -> run tables of the label image at the working resolution, the form every preparation
// function takes 2-D masks in (masks2d.DeviceRuns).
//
// Data layout in HBM
//   rows     u64 [K][nw]                       instance bit rows in the caller's point order; row order = priority
//   lab      u16 [n_points]                    1 + first row that holds the point, 0 = background; sorted cloud's order
//   xyz      f64 [3][n_pad]                    the sorted cloud of the sweep (a wave reads 3 x 512 B contiguous + 128 B of lab)
//   scratch  u32 [n_frames][depth_h * depth_w] all ones = empty; key = millimetres << 16 | label, unsigned min by
//                                              returnless vector atomics (as render_depth.hip's scratch)
//   labels   u16 [n_frames][depth_h][depth_w]  the key's low half, 0 = background or empty
//   depth    u16 [n_frames][depth_h][depth_w]  the key's high half = render_depth.hip's frame (optional)
// The z-buffer kernel is render_depth_kernel's / render_splat_depth_kernel's shape (1024 sorted points per block, 4 per
// thread in registers across the block's frame tile, poses wave-uniform, the tile culled in groups of 8 frames), a sibling
// with its own lines: the footprint helpers are copied here so that those kernels keep their machine code.
// Further down: the label image -> run tables without a dense plane per instance (label_runs_*).
#include <algorithm>
#include <cmath>

#include "geom.h"

namespace bff {

constexpr int kRlBlock = 256;
constexpr int kRlPPT = 4;                                          // points per thread
constexpr int kRlWordsPerBlock = (kRlBlock / kWave) * kRlPPT;      // 16 x 64 points
constexpr int kRlPtsPerBlock = kRlWordsPerBlock * kWave;           // 1024
constexpr int kRlCullGroup = 8;                                    // frames one culling pass decides
constexpr int kRlLaneBox = 64;                                     // texels a lane walks alone; beyond: the wave path
constexpr uint32_t kRlEmpty = 0xffffffffu;
constexpr int kRlMaxLabel = 65534;                                 // 65535 << 16 | 65535 is the empty key

// ---------------------------------------------------------------------------------------------------------------------
// One thread per point; a wave's 64 points share the word of every row, so the row loop reads one word per wave and row
// and ends as soon as every lane has found its first row.
__global__ __launch_bounds__(256) void point_labels_kernel(const uint64_t *__restrict__ rows, int n_rows, int64_t nw,
                                                            int64_t n_points, const int32_t *__restrict__ unsort,
                                                            uint16_t *__restrict__ lab)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = p < n_points;
    const int64_t w = in ? (p >> 6) : 0;                           // < nw (checked by the entry point)
    const int bit = (int)(p & 63);
    uint32_t found = 0;
    for (int k = 0; k < n_rows; ++k) {
        if (__all(found != 0 || !in)) break;                       // wave-uniform
        const uint64_t word = rows[(int64_t)k * nw + w];
        if (!found && in && ((word >> bit) & 1)) found = (uint32_t)k + 1;
    }
    if (!in) return;
    const int64_t dst = unsort ? (int64_t)unsort[p] : p;
    if ((uint64_t)dst < (uint64_t)n_points) lab[dst] = (uint16_t)found;      // a bad unsort entry writes nothing
}

// ---------------------------------------------------------------------------------------------------------------------
// render_depth.hip's texel_range / splat_range, operation by operation (see there for why the run they give is exact)
struct LabelBox { int j0, i0, bw, count; };                        // first column, first row, width, texels (0 = empty)

__device__ __forceinline__ void label_texel_range(double lo, double hi, double s, int n, int &first, int &last)
{
    const double a = fmax(floor((lo + 0.5) / s - 0.5) - 1.0, 0.0);
    const double b = fmin(ceil((hi + 0.5) / s - 0.5) + 1.0, (double)(n - 1));
    first = 0, last = -1;
    if (a <= b) first = (int)a, last = (int)b;                      // 0 <= a <= b <= n - 1: the conversions are exact
}

__device__ __forceinline__ void label_splat_range(double c, double R, double s, int n, int &first, int &last)
{
    label_texel_range(__dsub_rn(c, R), __dadd_rn(c, R), s, n, first, last);
    auto passes = [&](int t) { return fabs(__dsub_rn(__dsub_rn(__dmul_rn((double)t + 0.5, s), 0.5), c)) <= R; };
    while (first <= last && !passes(first)) ++first;
    while (last >= first && !passes(last)) --last;
}

// kSplat = false: every point offers its key to its own texel (render_depth_kernel's points and texels);
// kSplat = true: also to the texels of its footprint rectangle (render_splat_depth_kernel's), walked by the point's lane up
// to kRlLaneBox texels and by the whole wave beyond.
template <bool kSplat>
__global__ __launch_bounds__(kRlBlock) void render_labels_kernel(
    const double *__restrict__ xyz, int64_t n_points, int64_t n_pad, const uint16_t *__restrict__ lab,
    const double *__restrict__ inv_pose, CameraK K, int n_frames, int frames_per_block, int H, int W, int dh, int dw,
    double radius, uint32_t *__restrict__ scratch, const double *__restrict__ tile_bounds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t word0 = (int64_t)blockIdx.x * kRlWordsPerBlock + (int64_t)wave * kRlPPT;     // the wave's first 64 points
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    const int64_t plane = (int64_t)dh * dw;
    const double dW = (double)W, dH = (double)H;
    const double sx = dW / (double)dw, sy = dH / (double)dh;
    const double krx = __dmul_rn(K.k[0], radius), kry = __dmul_rn(K.k[4], radius);

    double px[kRlPPT], py[kRlPPT], pz[kRlPPT];
    uint32_t pl[kRlPPT];
    bool valid[kRlPPT];
#pragma unroll
    for (int j = 0; j < kRlPPT; ++j) {
        const int64_t n = (word0 + j) * kWave + lane;
        valid[j] = n < n_points;                                   // padding lanes take no part (they read point 0)
        const int64_t m = valid[j] ? n : 0;
        px[j] = xyz[m];
        py[j] = xyz[n_pad + m];
        pz[j] = xyz[2 * n_pad + m];
        pl[j] = lab[m];                                            // lab has n_points entries: m < n_points
    }

    for (int g0 = f0; g0 < f1; g0 += kRlCullGroup) {
        const int g1 = min(f1, g0 + kRlCullGroup);
        uint64_t culled = 0;
        if (tile_bounds && word0 * kWave < n_points)               // wave-uniform; only in-bounds points take part, so
            culled = cull_frames(tile_bounds + 6 * (word0 / kRlPPT), inv_pose, K, g0, g1, lane, dW, dH);   // culling stays exact
        for (int f = g0; f < g1; ++f) {
            if ((culled >> (8 * (f - g0))) & 1) continue;          // wave-uniform
            const double *P = inv_pose + 16 * (int64_t)f;
            uint32_t *img = scratch + (int64_t)f * plane;
#pragma unroll
            for (int j = 0; j < kRlPPT; ++j) {
                double cz, u, v;
                camera_pixel(P, K, px[j], py[j], pz[j], cz, u, v);
                // millimetres, half to even; a surface the camera sees lies in front of it (NaN fails cz > 0)
                const double m = rint(__dmul_rn(cz, 1000.0));
                const bool splat = valid[j] && pixel_in_bounds(u, v, dW, dH) && (cz > 0.0) && (m >= 1.0) && (m <= 65535.0);
                const uint32_t key = splat ? (((uint32_t)m << 16) | pl[j]) : kRlEmpty;
                // own texel: u < W and v < H, so tx < dw and ty < dh; W * dw and H * dh < 2^31 (checked by the entry point)
                if (splat)
                    atomicMin(img + ((int)(((unsigned)(int)v * (unsigned)dh) / (unsigned)H) * dw +
                                     (int)(((unsigned)(int)u * (unsigned)dw) / (unsigned)W)), key);   // result unused: returnless
                if constexpr (kSplat) {
                    LabelBox b = {0, 0, 0, 0};
                    if (splat) {
                        int j1, i1;
                        label_splat_range(u, krx / cz, sx, dw, b.j0, j1);
                        label_splat_range(v, kry / cz, sy, dh, b.i0, i1);
                        if (j1 >= b.j0 && i1 >= b.i0) {
                            b.bw = j1 - b.j0 + 1;
                            b.count = b.bw * (i1 - b.i0 + 1);      // <= dh * dw < 2^31
                        }
                    }
                    if (b.count > 0 && b.count <= kRlLaneBox)      // the lane's own walk, row by row
                        for (int k = 0, i = b.i0, t = b.j0; k < b.count; ++k) {
                            atomicMin(img + (i * dw + t), key);
                            if (++t == b.j0 + b.bw) t = b.j0, ++i;
                        }
                    uint64_t big = __ballot(b.count > kRlLaneBox); // every lane of the wave is here: no early exit above
                    while (big) {
                        const int src = __ffsll((unsigned long long)big) - 1;
                        big &= big - 1;
                        const uint32_t wkey = __shfl(key, src);
                        const int wj0 = __shfl(b.j0, src), wi0 = __shfl(b.i0, src), wbw = __shfl(b.bw, src), wcount = __shfl(b.count, src);
                        for (unsigned k = lane; k < (unsigned)wcount; k += kWave)       // unsigned: wcount + 63 may pass 2^31
                            atomicMin(img + ((wi0 + (int)(k / (unsigned)wbw)) * dw + wj0 + (int)(k % (unsigned)wbw)), wkey);
                    }
                }
            }
        }
    }
}

// scratch -> the two uint16 frames: low half = label, high half = millimetres, all ones (nothing offered) = 0 in both
__global__ __launch_bounds__(256) void render_labels_narrow_kernel(const uint32_t *__restrict__ scratch, int64_t total,
                                                                    uint16_t *__restrict__ labels, uint16_t *__restrict__ depth)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t s = scratch[i];
    const bool empty = s == kRlEmpty;
    labels[i] = empty ? 0 : (uint16_t)(s & 0xffffu);
    if (depth) depth[i] = empty ? 0 : (uint16_t)(s >> 16);
}

// ---------------------------------------------------------------------------------------------------------------------
// Label image -> run tables at the working resolution.  up[f][v][u] = labels[f][(v * dh) / H][(u * dw) / W] is never
// stored: a thread walks kLrPPT consecutive pixels of the flat index p = v * W + u and keeps the source texel by
// remainders (no division per pixel).  Where the label changes between p - 1 and p (a "transition at p") a run of the old
// label ends at p and one of the new label starts there; p = 0 starts and p = H * W ends whatever is there.
constexpr int kLrThreads = 256;
constexpr int kLrPPT = 32;                                         // pixels per thread
constexpr int kLrTile = kLrThreads * kLrPPT;                       // pixels per block (8192)

struct LabelWalk {
    const uint16_t *img;                                           // the frame's texels
    unsigned H, W, dh, dw;
    unsigned v, u, ty, ry, tx, rx;                                 // pixel, its texel, and (v * dh) % H, (u * dw) % W

    __device__ __forceinline__ void seek(int64_t p)
    {
        v = (unsigned)(p / W), u = (unsigned)(p % W);
        const uint64_t a = (uint64_t)v * dh, b = (uint64_t)u * dw;  // < 2^62
        ty = (unsigned)(a / H), ry = (unsigned)(a % H);
        tx = (unsigned)(b / W), rx = (unsigned)(b % W);
    }
    __device__ __forceinline__ unsigned label() const { return img[(int64_t)ty * dw + tx]; }
    __device__ __forceinline__ void next()
    {
        if (++u == W) {
            u = 0, tx = 0, rx = 0, ++v;
            uint64_t r = (uint64_t)ry + dh;                        // ry < H, so the sum may pass 2^32 only in 64 bits
            while (r >= H) r -= H, ++ty;
            ry = (unsigned)r;
        } else {
            uint64_t r = (uint64_t)rx + dw;
            while (r >= W) r -= W, ++tx;
            rx = (unsigned)r;
        }
    }
};

// The thread's stretch [p0, p1) of frame f: fn_edge(q, old, new) at every transition inside it (old = 0 at q = 0; the
// thread that owns the last pixel also gets (n_pixels, last, 0)), fn_seg(label, pixels) for every piece of one label.
template <typename Edge, typename Seg>
__device__ __forceinline__ void label_walk(const uint16_t *__restrict__ labels, int f, int H, int W, int dh, int dw,
                                           int64_t n_pixels, int64_t p0, Edge fn_edge, Seg fn_seg)
{
    if (p0 >= n_pixels) return;
    const int64_t p1 = min(p0 + (int64_t)kLrPPT, n_pixels);
    LabelWalk wk = {labels + (int64_t)f * dh * dw, (unsigned)H, (unsigned)W, (unsigned)dh, (unsigned)dw, 0, 0, 0, 0, 0, 0};
    unsigned prev = 0;
    if (p0 > 0) {
        wk.seek(p0 - 1);
        prev = wk.label();
        wk.next();
    } else {
        wk.seek(0);
    }
    int len = 0;
    for (int64_t q = p0; q < p1; ++q) {
        const unsigned cur = wk.label();
        if (cur != prev || q == 0) {
            if (len) fn_seg(prev, len);
            len = 0;
            fn_edge(q, q == 0 ? 0u : prev, cur);
            prev = cur;
        }
        ++len;
        wk.next();
    }
    if (len) fn_seg(prev, len);
    if (p1 == n_pixels) fn_edge(n_pixels, prev, 0u);
}

// grid (pixel tiles, frames).  n_runs, n_pix: int32 [n_frames][n_labels], entry (f, L - 1); exact, order independent
__global__ __launch_bounds__(kLrThreads) void label_runs_count_kernel(const uint16_t *__restrict__ labels, int H, int W, int dh,
                                                                       int dw, int64_t n_pixels, int n_labels,
                                                                       int32_t *__restrict__ n_runs, int32_t *__restrict__ n_pix)
{
    const int f = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kLrTile + (int64_t)threadIdx.x * kLrPPT;
    int32_t *runs = n_runs + (int64_t)f * n_labels, *pix = n_pix + (int64_t)f * n_labels;
    label_walk(labels, f, H, W, dh, dw, n_pixels, p0,
               [&](int64_t, unsigned, unsigned cur) { if (cur >= 1 && cur <= (unsigned)n_labels) atomicAdd(runs + (cur - 1), 1); },
               [&](unsigned l, int len) { if (l >= 1 && l <= (unsigned)n_labels) atomicAdd(pix + (l - 1), len); });
}

// grid (pixel tiles, frames).  mask_index: int32 [n_frames][n_labels], the mask (f, L) became or -1.  Every kept run's
// start and end are appended as (mask << 31) | p to start_keys / end_keys: a block counts its own, takes its places with
// one atomicAdd per list on cursor[0], cursor[1], and writes.  The places depend on the run; the sorted lists do not.
__global__ __launch_bounds__(kLrThreads) void label_runs_emit_kernel(const uint16_t *__restrict__ labels, int H, int W, int dh,
                                                                      int dw, int64_t n_pixels, int n_labels,
                                                                      const int32_t *__restrict__ mask_index, int64_t total_runs,
                                                                      uint32_t *__restrict__ cursor, int64_t *__restrict__ start_keys,
                                                                      int64_t *__restrict__ end_keys)
{
    __shared__ int wsum[kLrThreads / kWave];
    __shared__ uint32_t base[2];
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * kLrTile + (int64_t)tid * kLrPPT;
    const int32_t *index = mask_index + (int64_t)f * n_labels;
    auto mask_of = [&](unsigned l) { return (l >= 1 && l <= (unsigned)n_labels) ? index[l - 1] : -1; };
    int ns = 0, ne = 0;
    label_walk(labels, f, H, W, dh, dw, n_pixels, p0,
               [&](int64_t, unsigned old, unsigned cur) { ne += mask_of(old) >= 0; ns += mask_of(cur) >= 0; },
               [](unsigned, int) {});
    const int packed = ns | (ne << 16);                            // <= 32 of either per thread, 256 threads: no carry
    int incl = packed;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int excl = incl - packed, total = 0;
#pragma unroll
    for (int q = 0; q < kLrThreads / kWave; ++q) { if (q < wave) excl += wsum[q]; total += wsum[q]; }
    if (tid == 0) {
        base[0] = (total & 0xFFFF) ? atomicAdd(cursor, (uint32_t)(total & 0xFFFF)) : 0u;
        base[1] = (total >> 16) ? atomicAdd(cursor + 1, (uint32_t)(total >> 16)) : 0u;
    }
    __syncthreads();
    int64_t ps = (int64_t)base[0] + (excl & 0xFFFF), pe = (int64_t)base[1] + (excl >> 16);
    label_walk(labels, f, H, W, dh, dw, n_pixels, p0,
               [&](int64_t q, unsigned old, unsigned cur) {
                   const int mo = mask_of(old), mc = mask_of(cur);
                   if (mo >= 0) { if (pe < total_runs) end_keys[pe] = ((int64_t)mo << 31) | q; ++pe; }     // nothing is written
                   if (mc >= 0) { if (ps < total_runs) start_keys[ps] = ((int64_t)mc << 31) | q; ++ps; }   // past the lists
               },
               [](unsigned, int) {});
}

}  // namespace bff

using namespace bff;

extern "C" int bff_point_labels(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *unsort,
                                uint16_t *lab, void *stream)
{
    BFF_REQUIRE(n_rows >= 0 && nw >= 0 && n_points >= 0, "bff_point_labels: bad sizes");
    BFF_REQUIRE(nw >= ceil_div(n_points, 64), "bff_point_labels: rows of %lld words for %lld points", (long long)nw,
                (long long)n_points);
    BFF_LIMIT(n_rows <= kRlMaxLabel, "bff_point_labels: %d rows, at most %d", n_rows, kRlMaxLabel);
    const int64_t grid = ceil_div(n_points, 256);
    BFF_LIMIT(grid < (1ll << 31), "bff_point_labels: too many points for one launch");
    if (n_points == 0) return BFF_OK;
    BFF_REQUIRE(lab && (rows || n_rows == 0), "bff_point_labels: null pointer");
    point_labels_kernel<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(rows, n_rows, nw, n_points, unsort, lab);
    return launched("bff_point_labels");
}

extern "C" int bff_render_labels_u16(const double *xyz, int64_t n_points, int64_t n_pad, const uint16_t *lab,
                                     const double *inv_pose, const double *cam_intr_host, int32_t n_frames, int32_t height,
                                     int32_t width, int32_t depth_h, int32_t depth_w, double splat_radius,
                                     int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *labels_u16,
                                     uint16_t *depth_u16, const double *tile_bounds, void *stream)
{
    const char *what = "bff_render_labels_u16";
    BFF_REQUIRE(n_points >= 0 && n_pad >= n_points && n_frames >= 0 && frames_per_block >= 0, "%s: bad sizes", what);
    BFF_REQUIRE(height > 0 && width > 0 && depth_h > 0 && depth_w > 0, "%s: bad image size", what);
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "%s: image larger than 2^31 pixels", what);
    BFF_LIMIT((int64_t)depth_h * depth_w < (1ll << 31), "%s: depth frame larger than 2^31 texels", what);
    BFF_LIMIT((int64_t)height * depth_h < (1ll << 31) && (int64_t)width * depth_w < (1ll << 31),
              "%s: pixel x texel products beyond 2^31 (height * depth_h, width * depth_w)", what);
    BFF_LIMIT(n_frames <= 65535, "%s: too many frames", what);
    const int64_t total = (int64_t)n_frames * depth_h * depth_w;
    const int64_t gx = ceil_div(n_points, kRlPtsPerBlock);
    const int64_t n_narrow = ceil_div(total, 256);
    BFF_LIMIT(gx < (1ll << 31) && n_narrow < (1ll << 31), "%s: too many points / texels for one launch", what);
    // the comparisons fail on NaN; checked before the early returns, as the sizes are (K: where the caller gave one)
    BFF_REQUIRE(splat_radius >= 0.0 && std::isfinite(splat_radius), "%s: splat_radius must be finite and >= 0", what);
    const bool splat = splat_radius > 0.0;
    BFF_REQUIRE(!splat || !cam_intr_host || (cam_intr_host[0] > 0.0 && std::isfinite(cam_intr_host[0]) && cam_intr_host[4] > 0.0 &&
                                             std::isfinite(cam_intr_host[4])), "%s: K00 and K11 must be finite and > 0", what);
    if (n_frames == 0) return BFF_OK;
    BFF_REQUIRE(labels_u16, "%s: null pointer", what);
    hipStream_t st = as_stream(stream);
    if (n_points == 0) {                                             // nothing is offered: every texel is empty
        hipError_t e = hipMemsetAsync(labels_u16, 0, sizeof(uint16_t) * (size_t)total, st);
        if (e == hipSuccess && depth_u16) e = hipMemsetAsync(depth_u16, 0, sizeof(uint16_t) * (size_t)total, st);
        if (e != hipSuccess) return fail((int)e, "%s: memset: %s", what, hipGetErrorString(e));
        return BFF_OK;
    }
    BFF_REQUIRE(xyz && lab && inv_pose && cam_intr_host && scratch_u32, "%s: null pointer", what);
    hipError_t e = hipMemsetAsync(scratch_u32, 0xff, sizeof(uint32_t) * (size_t)total, st);
    if (e != hipSuccess) return fail((int)e, "%s: memset: %s", what, hipGetErrorString(e));
    CameraK K;
    for (int i = 0; i < 9; ++i) K.k[i] = cam_intr_host[i];
    // the culling table's tiles are the sweep's (bff_point_tile_bounds): they must be this kernel's waves
    BFF_REQUIRE(!tile_bounds || bff_point_tile_size() == kRlPPT * kWave, "%s: tile_bounds holds tiles of %d points, the "
                "renderer's waves own %d", what, bff_point_tile_size(), kRlPPT * kWave);
    int fpb = frames_per_block;
    if (fpb == 0) {                                                  // >= ~4096 blocks in flight, tiles of up to 8 frames
        fpb = (int)((int64_t)n_frames * gx / 4096);
        fpb = fpb < 1 ? 1 : (fpb > kRlCullGroup ? kRlCullGroup : fpb);
    }
    dim3 grid((unsigned)gx, (unsigned)ceil_div(n_frames, fpb));
    if (splat)
        render_labels_kernel<true><<<grid, kRlBlock, 0, st>>>(xyz, n_points, n_pad, lab, inv_pose, K, n_frames, fpb, height,
                                                              width, depth_h, depth_w, splat_radius, scratch_u32, tile_bounds);
    else
        render_labels_kernel<false><<<grid, kRlBlock, 0, st>>>(xyz, n_points, n_pad, lab, inv_pose, K, n_frames, fpb, height,
                                                               width, depth_h, depth_w, 0.0, scratch_u32, tile_bounds);
    int rc = launched(what);
    if (rc != BFF_OK) return rc;
    render_labels_narrow_kernel<<<(unsigned)n_narrow, 256, 0, st>>>(scratch_u32, total, labels_u16, depth_u16);
    return launched(what);
}

// the checks both passes of the run encoder share
static int label_runs_check(const char *what, int32_t n_frames, int32_t depth_h, int32_t depth_w, int32_t height, int32_t width,
                            int32_t n_labels)
{
    BFF_REQUIRE(n_frames >= 0 && n_labels >= 0, "%s: bad sizes", what);
    BFF_REQUIRE(height > 0 && width > 0 && depth_h > 0 && depth_w > 0, "%s: bad image size", what);
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "%s: image larger than 2^31 - 1 pixels", what);
    BFF_LIMIT((int64_t)depth_h * depth_w < (1ll << 31), "%s: label frame larger than 2^31 texels", what);
    BFF_LIMIT(n_frames <= 65535, "%s: too many frames", what);
    BFF_LIMIT(n_labels <= kRlMaxLabel, "%s: %d labels, at most %d", what, n_labels, kRlMaxLabel);
    return BFF_OK;
}

extern "C" int32_t bff_label_runs_tile_pixels(void) { return kLrTile; }

extern "C" int bff_label_runs_count(const uint16_t *labels, int32_t n_frames, int32_t depth_h, int32_t depth_w, int32_t height,
                                    int32_t width, int32_t n_labels, int32_t *n_runs, int32_t *n_pix, void *stream)
{
    int rc = label_runs_check("bff_label_runs_count", n_frames, depth_h, depth_w, height, width, n_labels);
    if (rc != BFF_OK) return rc;
    if (n_frames == 0 || n_labels == 0) return BFF_OK;
    BFF_REQUIRE(labels && n_runs && n_pix, "bff_label_runs_count: null pointer");
    hipStream_t st = as_stream(stream);
    const size_t bytes = sizeof(int32_t) * (size_t)n_frames * (size_t)n_labels;
    hipError_t e = hipMemsetAsync(n_runs, 0, bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(n_pix, 0, bytes, st);
    if (e != hipSuccess) return fail((int)e, "bff_label_runs_count: memset: %s", hipGetErrorString(e));
    const int64_t n_pixels = (int64_t)height * width;
    dim3 grid((unsigned)ceil_div(n_pixels, kLrTile), (unsigned)n_frames);
    label_runs_count_kernel<<<grid, kLrThreads, 0, st>>>(labels, height, width, depth_h, depth_w, n_pixels, n_labels, n_runs,
                                                         n_pix);
    return launched("bff_label_runs_count");
}

extern "C" int bff_label_runs_emit(const uint16_t *labels, int32_t n_frames, int32_t depth_h, int32_t depth_w, int32_t height,
                                   int32_t width, int32_t n_labels, const int32_t *mask_index, int64_t total_runs,
                                   uint32_t *cursor, int64_t *start_keys, int64_t *end_keys, void *stream)
{
    int rc = label_runs_check("bff_label_runs_emit", n_frames, depth_h, depth_w, height, width, n_labels);
    if (rc != BFF_OK) return rc;
    BFF_REQUIRE(total_runs >= 0, "bff_label_runs_emit: bad sizes");
    BFF_LIMIT(total_runs < (1ll << 31), "bff_label_runs_emit: %lld runs, at most 2^31 - 1", (long long)total_runs);
    if (n_frames == 0 || n_labels == 0 || total_runs == 0) return BFF_OK;
    BFF_REQUIRE(labels && mask_index && cursor && start_keys && end_keys, "bff_label_runs_emit: null pointer");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(cursor, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess) return fail((int)e, "bff_label_runs_emit: memset: %s", hipGetErrorString(e));
    const int64_t n_pixels = (int64_t)height * width;
    dim3 grid((unsigned)ceil_div(n_pixels, kLrTile), (unsigned)n_frames);
    label_runs_emit_kernel<<<grid, kLrThreads, 0, st>>>(labels, height, width, depth_h, depth_w, n_pixels, n_labels, mask_index,
                                                        total_runs, cursor, start_keys, end_keys);
    return launched("bff_label_runs_emit");
}
