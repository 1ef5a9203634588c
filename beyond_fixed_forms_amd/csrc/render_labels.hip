// 3-D instances rendered back into the views (include/bff_hip.h: bff_point_labels, bff_label_runs_count /
// bff_label_runs_emit): instance bit rows -> one label per point -> [the label z-buffer, bff_render_labels_u16: the
// labelled form of render_depth.hip's point z-buffer, there] -> run tables of the label image at the working resolution,
// the form every preparation function takes 2-D masks in (masks2d.DeviceRuns).
//
// Data layout in HBM
//   rows     u64 [K][nw]                       instance bit rows in the caller's point order; row order = priority
//   lab      u16 [n_points]                    1 + first row that holds the point, 0 = background; sorted cloud's order
//   labels   u16 [n_frames][depth_h][depth_w]  the z-buffer's label frames, 0 = background or empty
#include "geom.h"

namespace bff {

constexpr int kRlMaxLabel = 65534;                                 // the z-buffer's key: 65535 << 16 | 65535 is the empty one

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
