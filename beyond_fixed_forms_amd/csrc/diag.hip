// Measurement aids (scripts/diag_membw.py, bench.py): access patterns with a KNOWN number of distinct cache lines, to
// calibrate the FETCH_SIZE counter for the sweep's 4-byte gathers (MI355X_MICROARCH.md: only wide coalesced reads are
// calibrated -- x2 on gfx950 -- "calibrate on a known byte count in your own access pattern"), and the 128-byte lines one
// sweep touches (sweep_lines_kernel).
#include "sweep.h"

using namespace bff;

namespace {

// Every lane reads ONE float at element  ((wave * 64 + lane) * stride + jitter(lane))  of src, with
//   stride = 1   : 256 contiguous bytes per wave (2 x 128-B lines): the coalesced reference point
//   stride = 16  : one lane per 64-B half line
//   stride = 32  : one lane per 128-B line
//   stride = 1296: consecutive lanes in consecutive image rows (the worst case of the sweep's depth gather)
// Each element is touched exactly once per launch, the footprint is n_lanes * stride * 4 bytes (>> every cache).
template <int kTag>
__global__ void gather_stride_kernel(const float *__restrict__ src, int64_t n_lanes, int64_t stride, float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_lanes) return;
    const float v = src[t * stride];
    if (v == 12345.678f) out[t] = v;           // never true for the zero-filled table: keeps the load alive, writes nothing
}

}  // namespace

// pattern: 1, 16, 32 or any other stride (tagged 0 in the kernel name).  src must hold n_lanes * stride floats.
extern "C" int bff_diag_gather(const float *src, int64_t n_lanes, int64_t stride, float *out, void *stream)
{
    BFF_REQUIRE(src && out && n_lanes > 0 && stride > 0, "bff_diag_gather: bad arguments");
    const unsigned grid = (unsigned)ceil_div(n_lanes, 256);
    hipStream_t st = as_stream(stream);
    if (stride == 1) gather_stride_kernel<1><<<grid, 256, 0, st>>>(src, n_lanes, stride, out);
    else if (stride == 16) gather_stride_kernel<16><<<grid, 256, 0, st>>>(src, n_lanes, stride, out);
    else if (stride == 32) gather_stride_kernel<32><<<grid, 256, 0, st>>>(src, n_lanes, stride, out);
    else gather_stride_kernel<0><<<grid, 256, 0, st>>>(src, n_lanes, stride, out);
    return launched("bff_diag_gather");
}

namespace bff {

// Measurement aid: which 128-byte lines of the depth images and of the mask-word images does one sweep touch?
// One thread per (frame, point) recomputes the pixel with the sweep's own arithmetic and marks bit (pixel / ppl) of the
// frame's bitmap (ppl = pixels per 128-B line: 32 for float depth and 32-bit mask words, 16 for 64-bit words; with
// label_lines the segment bitmap is bff_rle_to_labels' and segments in label form mark that bitmap, 128 pixels per line); the
// caller counts the bits.  The COMPULSORY HBM traffic of the sweep is 128 B per marked line (each line has to come
// in at least once; everything beyond that is re-fetching), plus the cloud once per frame tile and the counters.
template <typename WordT>
__global__ void sweep_lines_kernel(const double *__restrict__ xyz, int64_t n_points, int64_t n_pad,
                                   const double *__restrict__ inv_pose, CameraK K, int n_frames,
                                   const void *__restrict__ depth, RawDepth raw, bool is_raw,
                                   const int32_t *__restrict__ depth_index, int H, int W,
                                   double thresh, const uint32_t *__restrict__ segmap, int64_t seg_words,
                                   const int32_t *__restrict__ frame_mask, uint32_t *__restrict__ depth_lines,
                                   uint32_t *__restrict__ mask_lines, int64_t line_words, uint32_t *__restrict__ label_lines)
{
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (n >= n_points) return;
    double cz, u, v;
    camera_pixel(inv_pose + 16 * (int64_t)f, K, xyz[n], xyz[n_pad + n], xyz[2 * n_pad + n], cz, u, v);
    if (!pixel_in_bounds(u, v, (double)W, (double)H)) return;
    const int pix = (int)v * W + (int)u;
    float d;
    if (is_raw) {                                                       // source texels: 64 (uint16) or 32 (float32) per 128-B line
        const char *img = raw_frame(depth, depth_index[f], raw);
        auto mark = [&](uint32_t t) {
            const int l = (int)(t >> (raw.texel_f32 ? 5 : 6));
            atomicOr(depth_lines + (int64_t)f * line_words + (l >> 5), 1u << (l & 31));
            return sensor_texel(img, t, raw);
        };
        const PixelTaps p = pixel_taps(raw.taps, W, (int)u, (int)v);    // the table in place, not a block's copy
        d = bilinear_depth(mark(p.t00), mark(p.t01), mark(p.t10), mark(p.t11), p.a, p.b);
    } else {
        const int dl = pix >> 5;                                        // 32 floats per 128-B line
        atomicOr(depth_lines + (int64_t)f * line_words + (dl >> 5), 1u << (dl & 31));
        d = reinterpret_cast<const float *>(depth)[(int64_t)depth_index[f] * H * W + pix];
    }
    const int mi = frame_mask ? frame_mask[f] : -1;
    if (mi < 0 || !depth_visible(cz, d, thresh)) return;
    if (label_lines) {
        const uint32_t *sm = segmap + 2 * ((int64_t)mi * seg_words + (pix >> 12));
        if (!((sm[0] >> ((pix >> 7) & 31)) & 1)) return;
        if (!((sm[1] >> ((pix >> 7) & 31)) & 1)) {                      // label form: 128 pixels per line
            const int ll = pix >> 7;
            atomicOr(label_lines + (int64_t)f * line_words + (ll >> 5), 1u << (ll & 31));
            return;
        }
    } else if (segmap && !((segmap[(int64_t)mi * seg_words + (pix >> 12)] >> ((pix >> 7) & 31)) & 1)) return;
    const int ml = pix / (int)(128 / sizeof(WordT));
    atomicOr(mask_lines + (int64_t)f * line_words + (ml >> 5), 1u << (ml & 31));
}

}  // namespace bff

// Marks the 128-byte lines one sweep touches (see sweep_lines_kernel).  depth_lines / mask_lines: uint32
// [n_frames][line_words] bitmaps, zeroed by the caller, line_words >= ceil(ceil(H*W / 16) / 32).
static int diag_sweep_lines(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                            const double *cam_intr_host, int32_t n_frames, const void *depth, const RawDepth *raw,
                            const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                            const uint32_t *segmap, int32_t word_bits, const int32_t *frame_mask,
                            uint32_t *depth_lines, uint32_t *mask_lines, int64_t line_words,
                            uint32_t *label_lines, void *stream)
{
    BFF_REQUIRE(xyz && inv_pose && cam_intr_host && depth && depth_index && depth_lines && mask_lines && n_points > 0 &&
                n_frames > 0 && (word_bits == 32 || word_bits == 64), "bff_diag_sweep_lines: bad arguments");
    BFF_REQUIRE(!label_lines || segmap, "bff_diag_sweep_lines: label lines need the label segment bitmap");
    BFF_LIMIT(n_frames <= 65535, "bff_diag_sweep_lines: too many frames");
    const CameraK K = camera_k(cam_intr_host);
    const int64_t seg_words = ceil_div(ceil_div((int64_t)height * width, 128), 32);
    dim3 grid((unsigned)ceil_div(n_points, 256), (unsigned)n_frames);
    const RawDepth rd = raw ? *raw : RawDepth{};
    if (word_bits == 32)
        sweep_lines_kernel<uint32_t><<<grid, 256, 0, as_stream(stream)>>>(xyz, n_points, n_pad, inv_pose, K, n_frames, depth, rd,
            raw != nullptr, depth_index, height, width, depth_thresh, segmap, seg_words, frame_mask, depth_lines, mask_lines,
            line_words, label_lines);
    else
        sweep_lines_kernel<uint64_t><<<grid, 256, 0, as_stream(stream)>>>(xyz, n_points, n_pad, inv_pose, K, n_frames, depth, rd,
            raw != nullptr, depth_index, height, width, depth_thresh, segmap, seg_words, frame_mask, depth_lines, mask_lines,
            line_words, label_lines);
    return launched("bff_diag_sweep_lines");
}

extern "C" int bff_diag_sweep_lines(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                                    const double *cam_intr_host, int32_t n_frames, const float *depth,
                                    const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                                    const uint32_t *segmap, int32_t word_bits, const int32_t *frame_mask,
                                    uint32_t *depth_lines, uint32_t *mask_lines, int64_t line_words,
                                    uint32_t *label_lines, void *stream)
{
    return diag_sweep_lines(xyz, n_points, n_pad, inv_pose, cam_intr_host, n_frames, depth, nullptr, depth_index, height, width,
                            depth_thresh, segmap, word_bits, frame_mask, depth_lines, mask_lines, line_words, label_lines, stream);
}

extern "C" int bff_diag_sweep_lines_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                                        const double *cam_intr_host, int32_t n_frames, const void *depth_raw,
                                        int32_t depth_h, int32_t depth_w, int32_t depth_layout,
                                        const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                                        const uint32_t *segmap, int32_t word_bits, const int32_t *frame_mask,
                                        uint32_t *depth_lines, uint32_t *mask_lines, int64_t line_words,
                                        uint32_t *label_lines, void *stream)
{
    RawDepth raw;
    BFF_REQUIRE(height > 0 && width > 0, "bff_diag_sweep_lines_u16: bad image size");
    const int rc = raw_depth_launch(depth_h, depth_w, height, width, depth_layout, as_stream(stream), &raw);
    if (rc != BFF_OK) return rc;
    return diag_sweep_lines(xyz, n_points, n_pad, inv_pose, cam_intr_host, n_frames, depth_raw, &raw, depth_index, height, width,
                            depth_thresh, segmap, word_bits, frame_mask, depth_lines, mask_lines, line_words, label_lines, stream);
}
