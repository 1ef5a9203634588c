/* bff_hip.h -- C ABI of libbff_hip.so: the MI355X (gfx950) kernels behind the 2D->3D mask
 * projection + multi-view fusion + refinement hot path of Beyond-Fixed-Forms.
 *
 * The reference has no FFI/operator ABI for this path: its boundary is files + Python dicts
 * (SURVEY.md section 8b).  This header is therefore the seam between this repo's Python host
 * (the beyond_fixed_forms_amd Python modules, which mirror the reference's dict/CLI interface) and its HIP
 * kernels.  Each entry point cites the reference lines whose arithmetic it replaces; paths are
 * relative to the reference checkout (tools/projection_2d_to_3d.py = P, tools/refinement.py = R,
 * tools/utils/rle_encode_decode.py = RLE, tools/segmentation_2d.py = SEG).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory
 *     (the host allocates through torch); no entry point allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - return value: 0 = launched, <0 = rejected argument (BFF_E_*), >0 = hipError_t of the launch;
 *     bff_last_error() gives a message for the calling thread;
 *   - "bit rows": a boolean row over N points is stored as ceil(N/64) uint64 words, point n is bit
 *     (n & 63) of word (n >> 6); padding bits of the last word are always 0;  `nw` = ceil(N/64);
 *   - integers are exact, float64 geometry is bit-exact w.r.t. the reference (see bff_project_views).
 */
#ifndef BFF_HIP_H
#define BFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFF_OK 0
#define BFF_E_ARG (-1)      /* null pointer / negative size / unsupported parameter */
#define BFF_E_LIMIT (-2)    /* size beyond what a kernel supports (documented per call) */

#define BFF_ABI_VERSION 16

int bff_abi_version(void);
const char *bff_last_error(void);
/* gfx target the library was compiled for ("gfx950"). */
const char *bff_arch(void);

/* Host-side helper (plain CPU code, all pointers are HOST pointers, no stream): component ids -> the groups
 * merge_masks keeps (P:203-226) as CSR.  comp[i] in [0, n) names the component of row i (e.g. the output of
 * bff_merge_components); kept: components with >= max(min_members, 1) members except isolated rows without
 * a self loop (the reference's `[]`, counted in *n_void when min_members <= 0); order: by smallest member,
 * members ascending.  Returns K (offs[0..K], members[0..offs[K]), sizes[0..K)); -1 = id out of range. */
int bff_host_component_csr(const int32_t *comp, const uint8_t *has_self_loop, int32_t n, int32_t min_members,
                           int32_t *offs, int32_t *members, int32_t *sizes, int32_t *n_void);

/* ------------------------------------------------------------------------------------------
 * a1 -- 2-D RLE masks -> per-pixel mask words.   Replaces RLE.rle_decode_batch (RLE:35-61) +
 * decode_2d_masks (RLE:82-99) + the float conversion at P:417-421; the dense (M,1,H,W) uint8
 * tensors (11.3 GB per scene at 200k x 300 x 30) are never materialised.
 *
 * Mask-view v owns masks [view_mask_offs[v], view_mask_offs[v+1]) (at most `word_bits` of them);
 * mask g owns runs [mask_run_offs[g], mask_run_offs[g+1]); run r covers flattened row-major pixels
 * [run_start[r], run_end[r]) (0-based, end exclusive, clipped to H*W by the host).  Runs of one
 * mask must be sorted and disjoint (what rle_encode_batch RLE:10-32 emits; the host normalises
 * anything else).  Output: maskbits[v][p] has bit b set iff pixel p lies in mask view_mask_offs[v]+b.
 * word_bits = 32 -> uint32 words, 64 -> uint64 words.
 * segmap (optional): uint32 [n_views][ceil(ceil(n_pixels/128)/32)] bitmap, bit s of a view = "128-pixel
 * segment s contains a mask pixel".  When given, all-zero segments of maskbits are NOT written (their
 * content is undefined) and bff_project_views must be given the same bitmap; NULL = every word is written.
 */
int bff_rle_to_maskbits(const int32_t *run_start, const int32_t *run_end, const int32_t *mask_run_offs,
                        const int32_t *view_mask_offs, int32_t n_views, int64_t n_pixels, int32_t word_bits,
                        void *maskbits, uint32_t *segmap, void *stream);

/* The same decode, each 128-pixel segment written in the cheaper of two forms:
 *   palette form  one 128-byte block of `labels` (uint8, rows of bff_label_plane_stride(n_pixels) bytes; block s of view
 *                 v = bytes [128 s, 128 s + 128) of its row): 64 bytes of 4-bit indices, pixel p's in byte (p mod 128) / 2,
 *                 low nibble for even p; then the palette: the words of the segment's PIECES (maximal runs of pixels
 *                 with the same word, the empty word included) in order -- 16 entries of 32 bits or 8 of 64 bits.  Pixel
 *                 p's word is palette[index(p)].  Index bytes of pixels past the image edge are unspecified;
 *   word form     words[v][p] = the word of bff_rle_to_maskbits (same layout, same word_bits) -- when the segment has
 *                 more pieces than the palette holds.
 * segmap (required): uint32 [n_views][2 * ceil(ceil(n_pixels/128)/32)]: word 2k = "segment holds a mask pixel" for
 * segments 32k..32k+31 (others are not written at all), word 2k + 1 = "segment is in word form".  Only the plane a
 * segment's form names is written for it.  Mask words change only where a run of some mask starts or ends, so a
 * 128-pixel stretch of a row has a handful of pieces whether masks overlap or not: the decoder -- bound by its writes --
 * stores, and the sweep gathers from, ONE 128-byte line per segment instead of four (word_bits 32) or eight.
 * labels must be 128-byte aligned, segmap 8-byte aligned. */
int64_t bff_label_plane_stride(int64_t n_pixels);
int bff_rle_to_labels(const int32_t *run_start, const int32_t *run_end, const int32_t *mask_run_offs,
                      const int32_t *view_mask_offs, int32_t n_views, int64_t n_pixels, int32_t word_bits,
                      uint8_t *labels, void *words, uint32_t *segmap, void *stream);

/* ------------------------------------------------------------------------------------------
 * a1b -- dense 2-D masks -> the run tables of a1, on the device.  Replaces RLE.rle_encode_batch (RLE:10-32: one
 * nonzero + one host copy per mask) + encode_2d_masks (RLE:63-80) for a caller that holds the (M,1,H,W) bool tensors
 * of SEG:276-305 on the device.  Two passes with one scan of n_runs in between (the host's: a device cumsum); the
 * dense bytes are read once, by the first.
 *
 * Dense 2-D masks -> bit planes + run counts.  masks: uint8 [n_masks][n_pixels] (the layout of a contiguous
 * torch.bool / torch.uint8 (M,1,H,W) tensor; ANY non-zero byte is a set pixel), n_pixels = H*W < 2^31.
 * bits: uint64 [n_masks][nw], nw = ceil(n_pixels/64), bit p%64 of word p/64 = pixel p, padding bits zero
 * (the row layout of bff_pack_rows).  n_runs: int32 [n_masks] = number of maximal runs of set pixels of each mask
 * (written, not accumulated: the caller clears nothing).  masks needs no alignment (mask g starts at byte
 * g * n_pixels) and no byte past masks + n_masks * n_pixels is read; bits and n_runs must not overlap masks. */
int bff_masks2d_count(const uint8_t *masks, int32_t n_masks, int64_t n_pixels, uint64_t *bits, int32_t *n_runs, void *stream);
/* Bit planes -> run tables in the layout bff_rle_to_maskbits reads: mask g writes its runs, ascending, as
 * run_start[k] / run_end[k] (0-based, end exclusive) for k in [run_offs[g], run_offs[g+1]).  run_offs: int32
 * [n_masks + 1] on the device, absolute positions in the caller's tables (so frames append into one table);
 * run_offs[g+1] - run_offs[g] must be the mask's n_runs (nothing is written outside those slots whatever it is).
 * run_start / run_end may be NULL when no mask has a run. */
int bff_masks2d_runs(const uint64_t *bits, int32_t n_masks, int64_t n_pixels, const int32_t *run_offs,
                     int32_t *run_start, int32_t *run_end, void *stream);
/* Pixels of one mask a block of the count pass reads (the tile of its grid; tests put sizes around it). */
int32_t bff_masks2d_tile_pixels(void);

/* ------------------------------------------------------------------------------------------
 * a2-a7 (+a15) -- fused per-frame: world->camera transform, projection, rounding, bounds +
 * depth test, mask-word gather, instance bit rows and the two per-point vote counters.
 * Replaces, per frame: P:424-425 (inv(pose) @ cloud), compute_projected_pts_tensor P:37-48,
 * compute_visibility_mask_tensor P:51-70 (depth_thresh is passed by the caller: 0.08 at P:438,565),
 * compute_visible_masked_pts_tensor P:73-92, the scatter-adds P:459-461 and, for the
 * detection-ratio sweep, P:548-567.
 *
 *   xyz          float64 [3][n_pad] structure-of-arrays (x row, y row, z row), n_pad >= n_points
 *   inv_pose     float64 [n_frames][16] row-major inverse camera pose (np.linalg.inv on the host)
 *   cam_intr     float64 [9] row-major K (HOST pointer; copied into kernel arguments)
 *   depth        float32 [n_depth][H*W] metres; frame f uses image depth_index[f]
 *   maskbits     mask words of bff_rle_to_maskbits, or -- with `labels` -- the word plane of bff_rle_to_labels
 *   labels       palette plane of bff_rle_to_labels (then maskbits and segmap are its companions) or NULL
 *   segmap       the decoder's segment bitmap (see bff_rle_to_maskbits) or NULL
 *   frame_mask   int32 [n_frames]: index of the frame's mask-word image in `maskbits`, or -1
 *   frame_rowbase int32 [n_frames]: first instance row of the frame (row = rowbase + bit)
 *   frame_nmask  int32 [n_frames]: number of masks (bits) of the frame, 0..word_bits
 *   frame_flags  int32 [n_frames]: bit0 = add visibility to viewed_count (P:567)
 *   rows         uint64 [n_rows][nw] instance bit rows, ZEROED BY THE CALLER (hipMemsetAsync on the same
 *                stream): row (rowbase+b) receives the points of mask b of every frame with a mask image;
 *                only 32-byte sectors that hold a point are stored                                (a6, a8)
 *   chunk_mask   optional uint64 [n_rows][bff_chunk_mask_words(nw)], zeroed by the caller too: bit c of a row =
 *                "chunk c (words 8c..8c+7, 512 points) of the row holds a point" -- exactly what bff_row_stats
 *                computes, for free here; lets bff_row_stats / bff_or_reduce_groups skip the empty 99 %
 *   masked_count int32 [n_points], += number of masks of the frame containing the visible point
 *                (P:459-461 adds 1 per mask, not per view); may be NULL
 *   viewed_count int32 [n_points], += visibility for frames with flag bit0; may be NULL
 *   tile_bounds  optional float64 table from bff_point_tile_bounds (frustum culling per wave and frame); NULL = off
 *
 * Arithmetic contract (bit-exact with NumPy/OpenBLAS float64 as used by the reference):
 *   c_i = fma chain over k = 0..3 of inv_pose[i][k] * (x, y, z, 1)[k] starting from +0.0;
 *   p_i = fma chain over k = 0..2 of K[i][k] * c[k];  u = rint(p_0 / c_2), v = rint(p_1 / c_2)
 *   (IEEE division, round half to even); in bounds iff 0 <= u < W and 0 <= v < H evaluated on the
 *   doubles (NaN/inf/out-of-int64-range fail, which equals the reference's INT64_MIN cast);
 *   visible iff depth != 0 and fabs(c_2 - (double)depth) < depth_thresh.  No z > 0 test.
 */
int bff_project_views(const double *xyz, int64_t n_points, int64_t n_pad,
                      const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                      const float *depth, const int32_t *depth_index, int32_t height, int32_t width,
                      double depth_thresh,
                      const void *maskbits, const uint8_t *labels, const uint32_t *segmap, int32_t word_bits,
                      const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                      const int32_t *frame_flags,
                      uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                      int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds, void *stream);

/* The same sweep with the depth frames resident as the PNGs store them (P:431-436): depth_raw uint16
 * [n_depth][depth_h][depth_w] millimetres at the sensor's resolution.  `astype(float32) / 1000` and the bilinear resize
 * to (height, width) are evaluated per point at the pixel it projects to, with exactly the float32 operations of
 * bff_depth_from_u16 (tap coefficients as io._axis_taps: float64 source coordinate cast to float32 before its floor is
 * subtracted, border columns copied, row indices clamped) -- results are bit-identical to bff_depth_from_u16 followed by
 * bff_project_views, the (height, width) float32 images (8 x the bytes) are never built.  height < 2^15, width < 2^16.
 * depth_layout: 0 uint16 frames row-major as stored; 1 uint16 in 8 x 8-texel tiles; 2 float32 METRES in 8 x 8-texel tiles
 * (bff_depth_tile_u16: `astype(float32) / 1000` done once per texel there) -- same values, fewer 128-byte lines per wave
 * (a wave's points project onto a compact patch and a point's four taps are neighbours in both directions) and, for
 * layout 2, no conversion or division left in the sweep.  The tap table of the resize (12 bytes per image row and column:
 * two texel offsets and the fraction, as io._axis_taps) is built on the device once per size combination and staged in
 * LDS by every block of the sweep; it must fit 48 KB (height + width <= 4096). */
int64_t bff_depth_tiled_texels(int32_t h_src, int32_t w_src);      /* texels of one tiled frame (padded to whole tiles) */
/* dst: uint16 [n][tiled texels] (out_f32 == 0) or float32 metres [n][tiled texels] (out_f32 != 0) */
int bff_depth_tile_u16(const uint16_t *src, int32_t n_frames, int32_t h_src, int32_t w_src, void *dst, int32_t out_f32,
                       void *stream);
int bff_project_views_u16(const double *xyz, int64_t n_points, int64_t n_pad,
                          const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                          const void *depth_raw, int32_t depth_h, int32_t depth_w, int32_t depth_layout,
                          const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                          const void *maskbits, const uint8_t *labels, const uint32_t *segmap, int32_t word_bits,
                          const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                          const int32_t *frame_flags,
                          uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                          int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds, void *stream);

/* The detection-ratio sweep alone (P:538-567), for a frame list that carries no masks: viewed_count[n] += 1 for every
 * frame f < n_frames in which point n is visible.  Visibility is bff_project_views' bit for bit (the same fma chains,
 * rint, bounds on the doubles, resize taps and operation order, depth test), so the counts equal what that sweep adds
 * under frame flag bit 0 -- computed once per scene, they serve every query class of the scene
 * (bff_scene_project_viewed).  viewed_count is int32 [n_points], NOT cleared here (the caller zeroes it).
 *   depth_layout -1: depth is float32 [n_depth][height * width] metres (depth_h, depth_w unused); 0, 1, 2: depth is the
 *                sensor-resolution frames of bff_project_views_u16 in that layout (height + width <= 4096)
 *   frames_per_block  frames one block visits (its frame tile); 0 = the library's choice
 *   tile_bounds  optional bff_point_tile_bounds table (exact frustum culling, as bff_project_views) */
int bff_count_viewed(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                     const double *cam_intr_host, int32_t n_frames, const void *depth, int32_t depth_h, int32_t depth_w,
                     int32_t depth_layout, const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                     int32_t frames_per_block, int32_t *viewed_count, const double *tile_bounds, void *stream);

/* ------------------------------------------------------------------------------------------
 * Depth frames rendered from the cloud: a point z-buffer for scenes that come without a depth image per frame (posed
 * colour captures with a reconstructed cloud).  It supplies the `depth` operand of the visibility test (P:51-70) that
 * P:431-436 otherwise reads from depth/<frame>.png.  out_u16: uint16 [n_frames][depth_h][depth_w] row-major millimetres,
 * 0 = no depth -- the frames bff_depth_tile_u16, bff_depth_from_u16 and bff_project_views_u16 (depth_layout 0) take.
 * For frame f and every point n < n_points (points at n >= n_points are never read as points):
 *   c, p, u = rint(p_0 / c_2), v = rint(p_1 / c_2) by the arithmetic contract of bff_project_views (fma chains from +0.0,
 *   IEEE division, round half to even; in bounds iff 0 <= u < width and 0 <= v < height on the doubles, so NaN, inf and
 *   huge values fail);
 *   the point splats iff it is in bounds, c_2 > 0 (a surface the camera sees lies in front of it -- the sweep has no such
 *   test) and m = rint(c_2 * 1000.0) (float64 product, half to even) satisfies 1 <= m <= 65535;
 *   its texel is tx = (u * depth_w) / width, ty = (v * depth_h) / height in integer arithmetic on the integer pixel;
 *   out[f][ty][tx] = the minimum m over the points that splat there, 0 if there is none.
 * A minimum of integers does not depend on the order of its operands: the frames are the same bytes on every run and
 * equal a sequential evaluation.  scratch_u32: uint32 [n_frames][depth_h * depth_w], set to all ones by the call itself,
 * which the points lower with returnless unsigned atomic minima; a second kernel narrows it to out_u16.
 *   xyz, inv_pose, cam_intr_host, tile_bounds   as bff_project_views (tile_bounds: exact frustum culling, same frames
 *                                               with and without it)
 *   frames_per_block  frames one block visits (its frame tile, as bff_count_viewed's); 0 = the library's choice.  The
 *                frames do not depend on it
 * Limits: height * width, depth_h * depth_w, height * depth_h and width * depth_w < 2^31; n_frames <= 65535. */
int bff_render_depth_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                         const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width,
                         int32_t depth_h, int32_t depth_w, int32_t frames_per_block, uint32_t *scratch_u32,
                         uint16_t *out_u16, const double *tile_bounds, void *stream);

/* ------------------------------------------------------------------------------------------
 * bff_render_depth_u16 with a surfel footprint per point: every point is a camera-facing square of half-width
 * splat_radius metres and is offered to every texel whose sample point its projection reaches, so a near surface closes
 * its own gaps (a fine frame of bff_render_depth_u16 is mostly empty texels, through which the background shows) and a
 * far one has depth in every texel.  Everything not named here -- the other arguments, out_u16, scratch_u32, the limits
 * and the early returns -- is bff_render_depth_u16's.
 *   splat_radius  r, metres: a finite double > 0 (anything else, NaN included, is BFF_E_ARG); K00 and K11 (cam_intr_host[0]
 *                 and [4]) must be finite and > 0 (BFF_E_ARG)
 * Every operation below is one IEEE float64 operation in the order written, without contraction.  For frame f and point
 * n < n_points:
 *   c, u, v and m = rint(c_2 * 1000.0) are exactly bff_render_depth_u16's (the sweep's fma chains, IEEE division, half to
 *   even, bounds tested on the doubles);
 *   the point takes part iff it would splat there: in bounds, c_2 > 0, 1 <= m <= 65535;
 *   Own texel   as bff_render_depth_u16: texel ((v * depth_h) / height, (u * depth_w) / width) is offered m;
 *   Footprint   radii in pixels:  Rx = (K00 * r) / c_2,  Ry = (K11 * r) / c_2.  Sample points of the texels are the mesh
 *     renderer's:  X_j = (j + 0.5) * (width / depth_w) - 0.5,  Y_i = (i + 0.5) * (height / depth_h) - 0.5.  Texel (i, j) of
 *     the frame is offered m iff fabs(X_j - u) <= Rx and fabs(Y_i - v) <= Ry.  The centre is the INTEGER pixel (u, v), the
 *     pixel the visibility test looks up for this point: there a point always finds its own depth or a nearer one.  The
 *     footprint is clipped to the frame; a point near the camera may cover all of it.
 *   out[f][i][j] = the minimum over everything texel (i, j) was offered, 0 if it was offered nothing.
 * Consequences:
 *   wherever bff_render_depth_u16's frame holds a depth, this frame holds a value that is not larger;
 *   the result is a minimum of integers: the frames do not depend on point order, frame tile or run;
 *   only in-bounds points take part, so the culling by tile_bounds stays exact: the same frames with and without the table;
 *   for the same reason a surface within a radius of the image border gets no help from points just outside the image:
 *     texels there may stay empty although the surface continues;
 *   the squares are flat (one depth per point), so on a surface tilted against the view a footprint reaches texels where
 *     the surface itself lies farther, and the minimum is biased towards the camera by about the radius times the slope:
 *     r should be about the cloud's point spacing, not larger.  Which value serves a dataset best is untuned. */
int bff_render_splat_depth_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                               const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width,
                               int32_t depth_h, int32_t depth_w, double splat_radius, int32_t frames_per_block,
                               uint32_t *scratch_u32, uint16_t *out_u16, const double *tile_bounds, void *stream);

/* Texels of a point's footprint rectangle up to which the point's own lane walks it; a larger rectangle is walked by the
 * whole wave. */
int bff_splat_lane_box(void);

/* ------------------------------------------------------------------------------------------
 * 3-D instances rendered back into the views as 2-D masks: instance bit rows -> one label per point (bff_point_labels)
 * -> a point z-buffer that carries the label next to the depth (bff_render_labels_u16) -> run tables of the label image
 * at the working resolution (bff_label_runs_count / bff_label_runs_emit), the form bff_rle_to_maskbits and
 * bff_mask_row_directory read 2-D masks in.
 *
 * bff_point_labels: rows uint64 [n_rows][nw] (nw >= ceil(n_points / 64)) in the caller's point order;
 *   lab[p] = 1 + min{k : bit p of row k is set}, 0 when no row holds point p: priority is row order.
 *   unsort (optional, int32 [n_points], a permutation as DeviceScene.unsort): the value of point o is written to
 *   lab[unsort[o]] instead of lab[o], i.e. lab comes out in the sorted cloud's order (an entry outside [0, n_points) writes
 *   nothing).  lab: uint16 [n_points].  n_rows <= 65534, more is BFF_E_LIMIT. */
int bff_point_labels(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *unsort,
                     uint16_t *lab, void *stream);

/* bff_render_labels_u16: the point z-buffer of bff_render_depth_u16 (splat_radius == 0) or of bff_render_splat_depth_u16
 * (splat_radius > 0) with a label per point.  Which points take part, their u, v, m = rint(c_2 * 1000.0), own texel,
 * footprint rectangle and sample points are exactly that call's, operation by operation; every argument not named here,
 * the early returns and the limits are that call's too.
 *   splat_radius  metres: 0 or a finite double > 0; NaN, a negative value or inf is BFF_E_ARG (> 0: K00 and K11 must be
 *                 finite and > 0 as there)
 *   lab           uint16 [n_points] in the order of xyz (bff_point_labels with the scene's unsort), every value <= 65534
 *   A point offers  key = (m << 16) | lab[n]  to each texel where the depth renderer offers m.  scratch_u32 (uint32
 *   [n_frames][depth_h * depth_w], set to all ones by the call) keeps the unsigned minimum of the keys; a narrowing kernel
 *   writes the key's low half to labels_u16 [n_frames][depth_h][depth_w] and its high half to depth_u16 (same shape, may be
 *   NULL); a texel that was offered nothing holds 0 in both.
 * Consequences:
 *   the nearest surface wins whether it carries an instance or not: background points (lab 0) occlude;
 *   at equal millimetres the smaller label wins: background before instance 0 before instance 1;
 *   depth_u16 equals the frame the matching depth renderer produces for the same arguments, byte for byte (m sits in the
 *     key's high half, so the minimum key holds the minimum m);
 *   the result is a minimum of integers: it does not depend on point order, frame tile, culling table or run;
 *   the flat surfels of splat_radius > 0 bleed a label by about one radius across a silhouette (the footprint of a near
 *     point reaches texels where only a farther surface lies, and the near key wins there).
 * Limits: bff_render_depth_u16's, and lab <= 65534 (65535 at m = 65535 would be the empty key). */
int bff_render_labels_u16(const double *xyz, int64_t n_points, int64_t n_pad, const uint16_t *lab, const double *inv_pose,
                          const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width, int32_t depth_h,
                          int32_t depth_w, double splat_radius, int32_t frames_per_block, uint32_t *scratch_u32,
                          uint16_t *labels_u16, uint16_t *depth_u16, const double *tile_bounds, void *stream);

/* Label image -> run tables at the working resolution, without a dense plane per instance.
 *   labels  uint16 [n_frames][depth_h][depth_w]; the upsampled image  up[f][v][u] = labels[f][(v * depth_h) / height]
 *           [(u * depth_w) / width]  (the renderer's own integer map, inverted) is never materialised
 *   Label L in [1, n_labels] of frame f: its runs are the maximal intervals [start, end) of the flat index p = v * width
 *   + u with up == L (they may cross a row end, as bff_masks2d_runs emits them).  Labels above n_labels are ignored.
 * bff_label_runs_count: n_runs, n_pix int32 [n_frames][n_labels] (entry (f, L - 1); cleared by the call) receive the
 *   number of runs and of pixels of every (f, L): integer atomics, exact on every run.
 * The caller decides which (f, L) become masks (pixel count >= its threshold), numbers them in (f, L) order into
 *   mask_index int32 [n_frames][n_labels] (-1 = no mask) and sums their run counts to total_runs.
 * bff_label_runs_emit: every run of a mask m appends (m << 31) | start to start_keys and (m << 31) | end to end_keys
 *   (int64 [total_runs] each; cursor: uint32 [2] scratch, cleared by the call).  The order inside the two lists depends on
 *   the run; as sets they are a function of the label image, and sorted ascending (bff_argsort_i64) the i-th start and the
 *   i-th end belong to one run and the runs stand in mask order, ascending inside a mask: the low 31 bits are the tables.
 * Limits: height * width < 2^31, depth_h * depth_w < 2^31, total_runs < 2^31, n_frames <= 65535, n_labels <= 65534. */
int32_t bff_label_runs_tile_pixels(void);                          /* pixels of a frame per block of both passes */
int bff_label_runs_count(const uint16_t *labels, int32_t n_frames, int32_t depth_h, int32_t depth_w, int32_t height,
                         int32_t width, int32_t n_labels, int32_t *n_runs, int32_t *n_pix, void *stream);
int bff_label_runs_emit(const uint16_t *labels, int32_t n_frames, int32_t depth_h, int32_t depth_w, int32_t height,
                        int32_t width, int32_t n_labels, const int32_t *mask_index, int64_t total_runs, uint32_t *cursor,
                        int64_t *start_keys, int64_t *end_keys, void *stream);

/* ------------------------------------------------------------------------------------------
 * Depth frames rendered from a triangle mesh: what bff_render_depth_u16 supplies, without its holes (fine frames) and
 * without the nearest point of a texel shadowing the whole texel (coarse frames).  out_u16, scratch_u32, inv_pose,
 * cam_intr_host (K, row-major) and frames_per_block are bff_render_depth_u16's; the call fills the scratch itself,
 * allocates nothing and synchronises nothing.
 *   vertices  float64 SoA [3][nv_pad], n_vertices of them
 *   faces     int32 [n_faces][3] on the device, indices into the vertices.  The caller has validated them
 *             (0 <= index < n_vertices); a triangle that names another index is not drawn.  The frames do not depend
 *             on the triangles' order.
 * Every operation below is an IEEE float64 operation in the order written, without contraction.
 * Vertex n in frame f:  c_0, c_1, c_2 by the fma chains of bff_project_views (k ascending from +0.0), so the vertex's
 *   depth c_2 is exactly what the visibility test compares.  Screen position in pixels, pixel centres at integers:
 *     px = ((K00 * c_0 + K01 * c_1) + K02 * c_2) / c_2,  py = ((K10 * c_0 + K11 * c_1) + K12 * c_2) / c_2
 *   (plain products and sums, no fma), and r = 1.0 / c_2.
 * Triangle in frame f:  takes part iff all three vertices have c_2 > 0, |px| < 2^24 and |py| < 2^24 (comparisons on the
 *   doubles: NaN fails).  A triangle that crosses the camera plane is therefore dropped, not clipped
 *   (bff_render_mesh_depth_clip_u16 clips it at a near plane instead).
 * Sample point of texel (i, j):  X = (j + 0.5) * (width / depth_w) - 0.5,  Y = (i + 0.5) * (height / depth_h) - 0.5
 *   (the quotients in float64): the pixel position the bilinear resize maps to the centre of that texel.
 * Coverage, with (x_k, y_k) = (px, py) of the triangle's vertex k:
 *     e0 = (x1 - X) * (y2 - Y) - (x2 - X) * (y1 - Y)
 *     e1 = (x2 - X) * (y0 - Y) - (x0 - X) * (y2 - Y)
 *     e2 = (x0 - X) * (y1 - Y) - (x1 - X) * (y0 - Y)
 *     S  = (e0 + e1) + e2
 *   the texel is covered iff S != 0 and (e0, e1, e2 all >= 0, or all <= 0): both windings count, and there is no fill
 *   rule -- a texel on a shared edge may be covered twice, which a minimum does not notice.
 * Depth:  z = S / ((e0 * r0 + e1 * r1) + e2 * r2) (perspective-correct), m = rint(z * 1000.0); the texel takes m iff
 *   1 <= m <= 65535.
 * Result:  out[f][i][j] = the minimum m over all triangles, 0 if there is none.  A minimum of integers has no order:
 *   the frames are the same bytes on every run.  The result is defined over all texels; the texel box a triangle's
 *   thread walks is an optimisation.
 * Limits: those of bff_render_depth_u16, and n_faces < 2^31.  n_frames = 0 returns at once; n_faces = 0 (or no vertex) gives frames
 * of zeros. */
int bff_render_mesh_depth_u16(const double *vertices, int64_t n_vertices, int64_t nv_pad, const int32_t *faces,
                              int64_t n_faces, const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                              int32_t height, int32_t width, int32_t depth_h, int32_t depth_w, int32_t frames_per_block,
                              uint32_t *scratch_u32, uint16_t *out_u16, void *stream);

/* ------------------------------------------------------------------------------------------
 * bff_render_mesh_depth_u16 with the triangles clipped at a near plane instead of dropped when they reach behind the
 * camera: a closed room seen from inside has depth in every texel.  Everything not named here is exactly
 * bff_render_mesh_depth_u16's definition (sample points, coverage test, S, perspective-correct z, m = rint(z * 1000.0),
 * 1 <= m <= 65535, minimum per texel, 0 if none; every operation one IEEE float64 operation in the order written, without
 * contraction), and so are the other arguments, the limits and the early returns.
 *   near_clip  zn, metres: a finite double with 0 < zn < 65.535 (anything else, NaN included, is BFF_E_ARG)
 * Per triangle and frame:
 *   Camera points  c_k = (c_0, c_1, c_2) of the three vertices by the fma chains, as above.  The triangle takes part only
 *     if all nine values are finite.
 *   Inside test    vertex k is inside iff its c_2 >= zn.
 *   Polygon        walk the edges k -> (k + 1) mod 3 for k = 0, 1, 2: if k is inside, emit vertex k; if k and k + 1 lie on
 *     different sides, emit the intersection.  The result has 0, 3 or 4 vertices.
 *   Intersection   always computed from the inside vertex p towards the outside vertex q, whichever way the edge is
 *     walked:  t = (p_2 - zn) / (p_2 - q_2),  I_0 = p_0 + t * (q_0 - p_0),  I_1 = p_1 + t * (q_1 - p_1),  I_2 = zn exactly.
 *     Two triangles that share a straddling edge therefore get bit-identical cut points: no crack opens between them.
 *   Screen position  an original vertex has its px, py and r = 1.0 / c_2 as above; a cut point has
 *     px = ((K00 * I_0 + K01 * I_1) + K02 * zn) / zn,  py likewise with K's second row,  r = 1.0 / zn.
 *   Fan            the polygon (v0, v1, ...) in emission order is drawn as (v0, v1, v2) and, with four vertices, also
 *     (v0, v2, v3).  Each is a triangle of the definition above: dropped if one of its three vertices fails |px| < 2^24,
 *     |py| < 2^24; S = 0 where two of its vertices coincide; the texel-box argument is the same.
 * Consequences:
 *   a triangle wholly nearer than zn is dropped;
 *   a triangle wholly at or beyond zn is drawn with exactly bff_render_mesh_depth_u16's arithmetic, so a mesh that never
 *     comes nearer than zn gives the same bytes as bff_render_mesh_depth_u16;
 *   a vertex with c_2 == zn gives t = 0, hence a fan triangle with two vertices at one position, which draws nothing;
 *   the result is still a minimum of integers: the same bytes on every run, independent of face order and frame tile.
 * zn bounds the nearest depth a frame can hold (rint(zn * 1000) mm); which value serves a dataset best is untuned. */
int bff_render_mesh_depth_clip_u16(const double *vertices, int64_t n_vertices, int64_t nv_pad, const int32_t *faces,
                                   int64_t n_faces, const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                                   int32_t height, int32_t width, int32_t depth_h, int32_t depth_w, double near_clip,
                                   int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *out_u16, void *stream);

/* Texels of a triangle's clipped texel box up to which the triangle's own lane walks the box; a larger box is walked
 * by the whole wave.  The box of a triangle along one axis: the texels t with floor((lo + 0.5) / s - 0.5) - 1 <= t <=
 * ceil((hi + 0.5) / s - 0.5) + 1, clipped to the frame (lo, hi: the vertices' extent in pixels, s: pixels per texel). */
int bff_mesh_lane_box(void);

/* Frustum culling for bff_project_views (optional, exact).  bounds: float64 [ceil(n_points / bff_point_tile_size())][6]
 * = (xmin, ymin, zmin, xmax, ymax, zmax) of every tile of bff_point_tile_size() consecutive points -- the points
 * one wave of the sweep owns.  Given the table, a wave skips a frame when the box of its points cannot contain a
 * point whose pixel is in bounds (a conservative half-space test of the 8 corners against the four image
 * borders, both in front of and behind the camera: the reference has no z > 0 test, P:57-67); results are
 * bit-identical with and without it.  It pays when the cloud is spatially sorted (scene.morton_order). */
int bff_point_tile_bounds(const double *xyz, int64_t n_points, int64_t n_pad, double *bounds, void *stream);
int bff_point_tile_size(void);

/* Frames one block of bff_project_views / _u16 / _lookup visits (its frame tile) for a cloud of n_points and a list of
 * n_frames: clamp(n_frames * ceil(n_points / 1024) / 4096, 1, 8), also bff_count_viewed's choice under
 * frames_per_block == 0.  Read-only: results never depend on it; tests ask it to know which tile sizes they reach. */
int32_t bff_sweep_frames_per_block(int64_t n_points, int32_t n_frames);

/* Profiling aid.  bff_profile_next_sweep(start, stop): the next bff_project_views launch of the calling host
 * thread carries the two events on its dispatch (hipExtLaunchKernelGGL), so that bff_event_elapsed_ms(start,
 * stop) is the kernel's own duration, as a profiler reports it (events recorded around a launch add the
 * latency of two barrier packets, ~50 us here).  bff_event_create returns a hipEvent_t (NULL on failure);
 * bff_event_elapsed_ms waits for `stop`. */
int bff_profile_next_sweep(void *start_event, void *stop_event);
void *bff_event_create(void);
int bff_event_destroy(void *event);
int bff_event_elapsed_ms(void *start_event, void *stop_event, float *ms);
/* hipEventRecord / hipEventSynchronize on such an event (hosts that hold a raw stream handle: a torch.cuda.Event.record()
 * looks the current stream up first, which costs more than the record). */
int bff_event_record(void *event, void *stream);
int bff_event_synchronize(void *event);

/* ------------------------------------------------------------------------------------------
 * Bit-row primitives (a8-a13, a16-a20).
 */

/* Row counts that become the y extent of a launch are limited to 65535: bff_pack_rows, bff_unpack_rows, bff_and_rows,
 * bff_gather_rows (n_out), bff_permute_bits, bff_rle_to_rows, bff_scatter_bits and bff_ids_to_rows (n_values) answer
 * BFF_E_LIMIT beyond that, before anything is launched or written. */

/* area[r] = popcount(rows[idx ? idx[r] : r])          (torch.sum(dim=1) at P:161,592,596; R:86-87)
 * nw == 0 (zero-width rows; rows may be NULL then): every area is 0. */
int bff_popcount_rows(const uint64_t *rows, const int32_t *idx, int32_t n_rows, int64_t nw,
                      int32_t *area, void *stream);

/* inter[i][j] = popcount(a[ia[i]] & b[ib[j]]), int32 [na][nb]: the {0,1} matmuls of
 * calculate_iou_between_stages R:84 and the any-overlap test of solve_overlapping P:289-292.
 * ia / ib may be NULL (identity).  nw == 0 (zero-width rows; a and b may be NULL then): inter is all zero, nothing
 * but the clear is issued. */
int bff_cross_popcount(const uint64_t *a, const int32_t *ia, int32_t na,
                       const uint64_t *b, const int32_t *ib, int32_t nb, int64_t nw,
                       int32_t *inter, void *stream);
/* The z extent of that launch: the words of a row are split over this many blocks per 64 x 64 tile (fewer than 512
 * tiles: slices of >= 64 words until ~512 blocks run; else 1).  1 = every entry is stored once; > 1 = partial counts
 * meet through atomics in a zeroed matrix; 0 = nothing is launched (an empty operand or nw == 0).  Read-only: results
 * never depend on it; tests ask it to know which path a shape reaches. */
int bff_cross_popcount_slices(int32_t na, int32_t nb, int64_t nw);

/* Per-row statistics that make the Gram block-sparse: area[r] = popcount(row r); mean_word[r] = mean word
 * index of its set bits (INT32_MAX for an empty row; a sort key that groups rows covering the same part of
 * the cloud when the points are spatially sorted); chunk_mask[r] = occupancy bits over chunks of 8 words
 * (512 points), bff_chunk_mask_words(nw) uint64 words per row; hist[r] = uint32 [64] histogram of the
 * row's set bits over 64 equal word ranges (bin width ceil(nw/64) words); signature[r] = 30-bit key: the indices
 * of the (at most 6, here: first 5) bins holding >= 15 % of the row, ascending, 6 bits each, most significant
 * first, unused slots = 63 (an empty row is all 63s and sorts last): rows showing the same object
 * get the same key, so sorting by it clusters them into the same 64-row tiles.
 * chunk_mask_given != 0: chunk_mask is an INPUT (as written by bff_project_views) and only the flagged chunks
 * of every row are read; 0: chunk_mask is computed here from a full pass over the rows.
 * chunk_pop (optional, may be NULL): uint16 [n_rows][64 * bff_chunk_mask_words(nw)], points of the row in each of
 * its 512-point chunks (0 where the row has none): the bins of bff_merge_components' second-level bound. */
int bff_row_stats(const uint64_t *rows, int32_t n_rows, int64_t nw, int32_t *area, int32_t *mean_word,
                  uint64_t *chunk_mask, int32_t chunk_mask_given, uint32_t *hist, int64_t *signature,
                  uint16_t *chunk_pop, void *stream);
int bff_chunk_mask_words(int64_t nw);

/* rows[r][chunk c] = 0 for every chunk flagged in chunk_mask (as written by bff_project_views): returns a
 * zero-filled row buffer to all-zero after a scene at the cost of the ~1 % of it that was ever stored, so the
 * buffer can serve the next scene without another full zero-fill. */
int bff_clear_flagged_chunks(uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *chunk_mask, void *stream);

/* a9-a11: merge adjacency of `aggregate` P:100-146.  For every pair (i, j):
 *   I = popcount(rows[i] & rows[j]);  iou = (float)I / ((float)area[i] + (float)area[j] - (float)I)
 *   (IEEE float32 division; 0/0 = NaN compares false, P:149-166);
 *   adjacent = label_id[i] == label_id[j]  &&  iou > iou_thres   (float32 compare, P:120-122)
 * label_id replaces the string compare of calculate_feature_similarity P:169-187.
 * `order` (int32 [n_rows], may be NULL = identity) is the order in which rows are tiled: tile t holds rows
 * order[64t .. 64t+63].  adj: uint64 [n_rows][ceil(n_rows/64)], bit q of row p <=> rows order[p] and
 * order[q] are adjacent (i.e. indexed by POSITION in `order`), fully written.
 * chunk_mask (from bff_row_stats) + tile_mask (scratch, uint64 [ceil(n_rows/64)][bff_chunk_mask_words(nw)])
 * enable chunk skipping: a 64x64 tile pair only visits chunks both tiles occupy (exact: skipped words
 * contribute 0 to every intersection); both NULL = visit every word.
 * hist (from bff_row_stats, may be NULL; used only together with chunk_mask and when inter == NULL): a tile
 * pair first bounds every intersection by UB = sum_bins min(hist_i, hist_j) >= I and evaluates the same
 * float32 IoU test on min(UB, area_i, area_j) (the test is monotone in I); tiles without a possible edge
 * skip their word loop.  Sound: the adjacency is unchanged.
 * inter (optional, may be NULL): int32 [n_rows][n_rows] Gram matrix in ROW index space, for tests. */
int bff_merge_adjacency(const uint64_t *rows, int32_t n_rows, int64_t nw, const int32_t *order,
                        const uint64_t *chunk_mask, uint64_t *tile_mask, const uint32_t *hist,
                        const int32_t *area,
                        const int32_t *label_id, float iou_thres,
                        uint64_t *adj, int32_t *inter, void *stream);

/* a9-a12 in one pass, the production path: connected components of the merge graph of `aggregate`
 * (same adjacency definition as bff_merge_adjacency) WITHOUT materialising the adjacency matrix and
 * without the transitive-closure matmuls of find_unconnected_subgraphs_tensor P:250-274.  64x64 tile pairs
 * are visited diagonal-first in `order`; a pair is examined only if the histogram bound allows an edge AND
 * its two rows are not yet in one component; edges found are merged into a disjoint-set forest
 * (`parent`, int32 [n_rows]; init_parent != 0: start from singletons, == 0: continue from the forest
 * already in `parent`, e.g. a coarser partition known to the caller) with compare-and-swap.  Exact: a pair is skipped only when it cannot
 * be an edge or when adding the edge could not change the components.
 * `order` may list only n_order <= n_rows of the rows (a sample): only pairs among the listed rows are
 * examined, which is how the caller builds a coarse forest first (every 8th row) and then refines it with the
 * full order and init_parent = 0.  comp (int32 [n_rows], out, may be NULL): comp[i] = smallest row index of
 * i's component.  Rows with an empty
 * adjacency row (area 0, or thr >= 1) form singleton components here; the host turns them into the
 * reference's empty lists (it knows area and thr).  All other arguments as for bff_merge_adjacency;
 * chunk_mask, tile_mask and hist are required; scratch: uint32 [bff_merge_scratch_words(n_rows)], 8-byte aligned
 * (sorted histograms, tile bounds, position-indexed row tables, the two tile-pair lists; layout: merge.hip, MergeScratch).
 * Inside a tile pair the block keeps disjoint sets of its 128 rows in LDS (started from the global forest): every
 * few chunks it settles the pairs whose PARTIAL intersection already passes the IoU test (the float32 expression is
 * monotone in I, so the edge exists) or whose rows have become connected meanwhile, and stops as soon as no pair is
 * open; only edges that merge two local sets are pushed into `parent`.
 * chunk_pop (optional, from bff_row_stats): second-level bound -- pairs that pass the 64-bin histogram bound are
 * bounded again by sum over the shared 512-point chunks of min(points of i, points of j) before any word is read.
 * diag (optional, NULL in production): int32 [16 + 2 * capacity], zeroed by the caller: += {tile pairs evaluated,
 * chunks visited, candidate pairs, unions, phase clocks ...} (scripts/diag_merge_phases.py).  The counters, summed
 * over the blocks of the tile pass (a split tile pair runs one block per part, and each part counts):
 *   [0] blocks that got past the bounds (some candidate pair left), [1] chunks on their chunk lists, [2] candidate
 *   pairs, [3] unions pushed into the global forest, [9] blocks that took the pair-list path, [10] blocks that took
 *   the dense 4x4 path ([9] + [10] = [0]); [4]-[8] and [11] are phase clocks, [14] / [15] select the block timeline. */
int64_t bff_merge_scratch_words(int32_t n_rows);
/* Whether bff_merge_components applies the chunk bound for rows of nw words (clouds of >= ~0.5 M points; the environment
 * variable BFF_CHUNK_BOUND=0/1 overrides): callers can skip computing chunk_pop otherwise. */
int32_t bff_merge_uses_chunk_bound(int64_t nw);
/* Profiling aid: the next tile-pass dispatch of bff_merge_components on this host thread carries the two events
 * (like bff_profile_next_sweep). */
int bff_profile_next_merge(void *start_event, void *stop_event);
int bff_merge_components(const uint64_t *rows, int32_t n_rows, int64_t nw, const int32_t *order, int32_t n_order,
                         const uint64_t *chunk_mask, uint64_t *tile_mask, const uint32_t *hist,
                         uint32_t *scratch, const int32_t *area, const int32_t *label_id, float iou_thres,
                         int32_t *parent, int32_t init_parent, int32_t *comp, int32_t *diag,
                         const uint16_t *chunk_pop, void *stream);

/* rows_out[r] bit o = rows_in[r] bit idx[o], o < n_out (bit gather).  Undoes the spatial point sort the
 * host applies at upload: idx[o] = position of original point o in the sorted cloud. */
int bff_permute_bits(const uint64_t *rows_in, int32_t n_rows, int64_t nw_in, const int32_t *idx,
                     int64_t n_out, int64_t nw_out, uint64_t *rows_out, void *stream);

/* a12: connected components of a symmetric bit adjacency (find_unconnected_subgraphs_tensor
 * P:250-274 computes the transitive closure by n rounds of clamp(R@A + A); for the symmetric
 * matrices produced by bff_merge_adjacency its rows are the connected components).
 * One call = one propagation round: label[i] <- min(label[i], min over neighbours j of label[j]),
 * followed by pointer jumping; *changed (int32, device) is set to 1 if any label moved.
 * The host initialises label[i] = i, zeroes *changed and iterates until it stays 0; the result is
 * label[i] = smallest member index of i's component. */
int bff_components_round(const uint64_t *adj, int32_t n_nodes, const int32_t *label_in, int32_t *label_out,
                         int32_t *changed, void *stream);

/* a13: out[g] = OR of rows[members[group_offs[g] .. group_offs[g+1])]      (merge_masks P:219-224;
 * also the `.any(dim=0)` merge of R:269).  max_group_size >= the largest group (host knows the groups);
 * it only sizes the launch.  conf / conf_mean (optional, both or neither; dtype as bff_group_conf_mean): the
 * same launch also computes bff_group_conf_mean on extra blocks, so the long sequential sums run beside the OR.
 * chunk_mask (optional, the rows' chunk flags): long rows are read through it.
 * A group without members (group_offs[g] == group_offs[g+1]) gets an all-zero row, whatever max_group_size is, and
 * the mean 0 / 0 = NaN. */
int bff_or_reduce_groups(const uint64_t *rows, int64_t nw, const int32_t *group_offs, const int32_t *members,
                         int32_t n_groups, int32_t max_group_size, uint64_t *out, const void *conf,
                         int32_t conf_dtype, void *conf_mean, const uint64_t *chunk_mask, void *stream);

/* a13: mean[g] = (((c[m0] + c[m1]) + c[m2]) ...) / len, every step rounded to the confidence dtype
 * (P:225: python `sum(conf) / len(conf)` over 0-dim tensors).  dtype: 0 = float32, 1 = float16. */
int bff_group_conf_mean(const void *conf, int32_t dtype, const int32_t *group_offs, const int32_t *members,
                        int32_t n_groups, void *mean, void *stream);

/* a16 + a14 + the two popcounts around them in one pass, k <= bff_resolve_overlaps_max_rows() (4096) rows:
 *   before[i] = popcount(rows[i])                             (before any edit, P:592)
 *   solve_overlapping P:277-301 on `rows` in place.  The reference visits the pairs (i < j) that overlap before any
 *     edit in (i, j) order; the row merged from fewer raw masks (size[], ties: row i) loses the points of the other.
 *     For a single point that walk is a champion scan over the rows holding it, so the point ends up in exactly one of
 *     them: the one with the largest size, among equals the largest index (derivation: resolve.hip,
 *     resolve_priority_kernel) -- an exclusive prefix OR over the rows in that order, no intersections needed;
 *   rows[i] &= keep (P:595; keep may be NULL);  after[i] = popcount(rows[i])  (P:596).
 * The literal ordered replay stays available as bff_overlap_ops + bff_apply_row_ops (tests compare the two). */
int bff_resolve_overlaps(uint64_t *rows, int32_t k, int64_t nw, const int32_t *size, const uint64_t *keep,
                         int32_t *before, int32_t *after, void *stream);
int bff_resolve_overlaps_max_rows(void);

/* a16/a20: sequential row program applied independently to every word column.
 * ops: int32 [n_ops][3] = (opcode, dst, src) executed in order;
 *   opcode 0: rows[dst] &= ~rows[src]   (solve_overlapping P:295-299)
 *   opcode 1: rows[dst] |=  rows[src]   (stage-1 duplicate merge R:248)
 *   opcode 2: rows[dst]  =  rows[src]
 * n_ops < 0: the list lives on the device as [count, triples...] (as written by bff_overlap_ops). */
int bff_apply_row_ops(uint64_t *rows, int64_t nw, const int32_t *ops, int32_t n_ops, void *stream);

/* a16: the pair loop of solve_overlapping P:285-299 without a host round trip.  inter = K x K intersections
 * of the aggregated rows before any edit (bff_cross_popcount), size[i] = number of raw masks merged into row
 * i (P:285).  ops (int32 [1 + 3*K*(K-1)/2]) receives [count, (0, loser, winner)...] in the reference's pair
 * order: the row built from fewer masks loses the overlap, ties: the first row loses. */
int bff_overlap_ops(const int32_t *inter, const int32_t *size, int32_t k, int32_t *ops, void *stream);

/* a16: rows[r] &= keep for r < n_rows                                                   (P:595) */
int bff_and_rows(uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *keep, void *stream);

/* out[r] = rows[idx[r]] (row gather; P:601-607 row selection, R:310). */
int bff_gather_rows(const uint64_t *rows, const int32_t *idx, int32_t n_out, int64_t nw, uint64_t *out,
                    void *stream);

/* bit rows <-> dense boolean rows (uint8 0/1, the layout of torch.bool), for the dict contract
 * {"ins": bool (K,N)} (P:630-634, R:411). */
int bff_unpack_rows(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, uint8_t *dense,
                    void *stream);
int bff_pack_rows(const uint8_t *dense, int32_t n_rows, int64_t n_points, int64_t nw, uint64_t *rows,
                  void *stream);

/* a18: 1-D RLE (Open3DIS stage-1 "ins") -> bit rows.  rle_decode R:26-39.  Same run layout as
 * bff_rle_to_maskbits: row g owns runs [row_run_offs[g], row_run_offs[g+1]), sorted, disjoint. */
int bff_rle_to_rows(const int32_t *run_start, const int32_t *run_end, const int32_t *row_run_offs,
                    int32_t n_rows, int64_t n_points, int64_t nw, uint64_t *rows, void *stream);

/* SURVEY section 8f row 1 -- bit rows -> 1-D RLE in the reference's format (rle_encode_batch RLE:10-32: 1-based
 * start, length pairs), so results can be stored like Open3DIS stage-1 files (eval_scannet200.py:123-124 reads
 * them).  bff_rle_count_runs: n_runs[r] = number of runs of row r.  The host turns that into exclusive offsets
 * run_offs (int64 [n_rows]) and a total; bff_rle_encode_rows then fills counts (int64 [2 * n_runs_total]) with
 * row r's pairs at counts[2*run_offs[r] ...].  Padding bits of the rows must be zero (they always are here). */
int bff_rle_count_runs(const uint64_t *rows, int32_t n_rows, int64_t nw, int32_t *n_runs, void *stream);
int bff_rle_encode_rows(const uint64_t *rows, int32_t n_rows, int64_t nw, const int64_t *run_offs,
                        int64_t n_runs_total, int64_t *counts, void *stream);

/* SURVEY section 8f row 4 -- the consumer right after the path: ScanNet instance evaluation intersects every
 * predicted mask with every ground-truth instance (`count_nonzero(logical_and(gts == instance_id, pred_mask))`,
 * evaluation/eval/scannetv2_inst_eval.py:334).  bff_ids_to_rows turns the per-point id vector into one bit row
 * per requested value (rows[v] bit p = ids[p] == values[v]); the intersections are then one bff_cross_popcount. */
int bff_ids_to_rows(const int64_t *ids, int64_t n_points, const int64_t *values, int32_t n_values, int64_t nw,
                    uint64_t *rows, void *stream);

/* ------------------------------------------------------------------------------------------
 * a14/a15 -- point filters (P:512-583), kept entirely on the device.
 * bff_point_values: vals[n] = (float)masked[n] / ((float)viewed[n] + 1.0f) (P:571; IEEE float32), or
 * (float)masked[n] when viewed == NULL (P:513).  The caller sorts vals ascending (bff_sort_f32), then
 * bff_select_unique_rank writes *thr = distinct_values[floor(fraction * n_distinct)]
 * -- the reference's `x.unique()[math.floor(t * x.unique().shape[0])]` (P:516-518, 574-576; float64 product;
 * NaN when the index is out of range, where python raises IndexError) -- and *n_unique.  block_scratch:
 * int32 [ceil(n/1024)].
 * bff_ratio_keep: keep bit n = masked[n] > 0 && !(value[n] < thr) with value as above (P:522,578,583);
 * the threshold is read from thr_dev (device) when non-NULL, else the immediate `thr`; use_thr == 0 -> keep =
 * masked > 0. */
int bff_point_values(const int32_t *masked, const int32_t *viewed, int64_t n_points, float *vals, void *stream);
/* The same (thr, n_unique) without sorting n_points values: the statistic is a function of the integer pair (masked,
 * viewed), of which a scene holds only ~10^3..10^5 different ones: every block collects the distinct values of its
 * 1024 points in LDS and writes them to its slice of `scratch` (no global atomics, nothing to clear); 64 blocks, one per
 * 1/64 of the hash space, merge the slices in LDS sets (together = x.unique() of P:516 / P:574); one block radix-selects
 * the rank: three launches.  scratch: uint32 [bff_point_threshold_scratch_words(n_points)]; *overflow (device, not
 * cleared by the call) is set to 1 if a partition holds more distinct values than bff_point_threshold_capacity(): use
 * the sorting path then. */
int64_t bff_point_threshold_scratch_words(int64_t n_points);
int32_t bff_point_threshold_capacity(void);
int32_t bff_point_threshold_capacity_set(int32_t cap);     /* test hook: smaller capacity (0 = default); returns the new one */
int bff_point_threshold_pairs(const int32_t *masked, const int32_t *viewed, int64_t n_points, double fraction,
                              uint32_t *scratch, float *thr, int32_t *n_unique, int32_t *overflow, void *stream);
int bff_select_unique_rank(const float *sorted, int64_t n, double fraction, int32_t *block_scratch,
                           float *thr, int32_t *n_unique, void *stream);
int bff_ratio_keep(const int32_t *masked, const int32_t *viewed, int64_t n_points, float thr,
                   const float *thr_dev, int32_t use_thr, int64_t nw, uint64_t *keep, void *stream);

/* ------------------------------------------------------------------------------------------
 * a4 / SURVEY section 8f row 2 -- depth ingestion on the device.  src: uint16 [n_frames][h_src][w_src] raw
 * depth in millimetres (the decoded 16-bit PNGs, P:432-433); dst: float32 [n_frames][height][width] =
 * resize(src.astype(f32) / depth_scale, (width, height)) with the bilinear rule of cv2.resize (INTER_LINEAR:
 * half-pixel centres, edge clamp, horizontal then vertical 2-tap passes in float32, P:436).  The host passes
 * the tap tables it computed in float64 (x0/x1/ax [width], y0/y1/ay [height]; io.bilinear_taps); with equal
 * source and target size the tables may be NULL and the call is the plain division.  Uploading 2 B/pixel at
 * sensor resolution instead of 4 B/pixel at colour resolution cuts the per-scene H2D volume ~8x. */
int bff_depth_from_u16(const uint16_t *src, int32_t n_frames, int32_t h_src, int32_t w_src,
                       const int32_t *x0, const int32_t *x1, const float *ax,
                       const int32_t *y0, const int32_t *y1, const float *ay,
                       int32_t height, int32_t width, float depth_scale, float *dst, void *stream);

/* ------------------------------------------------------------------------------------------
 * Library sorts (rocPRIM radix sort) so that the ABI is self-sufficient.  Both follow the usual two-call
 * protocol: temp == NULL -> only *temp_bytes is written (no launch); then call again with that much device
 * scratch.  bff_sort_f32: keys_out = keys_in ascending (the input of bff_select_unique_rank).
 * bff_argsort_i64: order_out = stable ascending argsort of int64 keys (ties keep index order), keys_scratch =
 * int64 [n]; key_bits = 64 sorts the full signed keys, key_bits < 64 promises 0 <= key < 2^key_bits and sorts
 * only those bits (fewer radix passes).  Used to order the Gram tiles by row signature (30 bits) and, stably on
 * top, by label id. */
int bff_sort_f32(const float *keys_in, float *keys_out, int64_t n, void *temp, size_t *temp_bytes, void *stream);
int bff_argsort_i64(const int64_t *keys, int64_t *keys_scratch, int32_t *order_out, int32_t n, int32_t key_bits,
                    void *temp, size_t *temp_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * a21/a24 -- cosine similarity GEMM on the matrix cores (MFMA f16 -> f32).
 *   cos[i][j] = <a_i, b_j> / (||a_i|| * ||b_j||), float32 accumulate and normalisation
 * (compute_clip_similarity R:93-115; bbox_filter SEG:388-393).  a: f16 [na][dim], b: f16 [nb][dim],
 * dim % 32 == 0, cos: float32 [na][nb].  A zero row of a gives NaN across its row of cos and a zero row of b NaN down
 * its column (0 / 0, as the reference's expression dot / (|a| |b|) does). */
int bff_cosine_gemm_f16(const void *a, int32_t na, const void *b, int32_t nb, int32_t dim,
                        float *cos, void *stream);
/* a24 -- the box filter's product  F.normalize(box_emb) @ text.T  (SEG:388-393): rows of a are normalised, rows of b
 * are taken as they are (the reference normalises the text mean beforehand, SEG:336).  Same kernels, same limits.
 * F.normalize divides by max(|a_i|, 1e-12), so a zero row of a gives 0.0 across its row of sim (never NaN); a zero row
 * of b is not normalised at all and gives 0.0 down its column. */
int bff_normalized_gemm_f16(const void *a, int32_t na, const void *b, int32_t nb, int32_t dim,
                            float *sim, void *stream);
/* Host only, launches nothing: the kernel the two entry points above launch for this shape in this process --
 * 0 small (one wave per 16 x 16 tile; nb <= 64), 1 rows (nb > 64, na < 2048), 2 tile64 (nb > 64, na >= 2048, bank through
 * LDS), 3 / 4 bank-stationary at dim 768 with 2 / 4 staged pieces per thread, 5 bank-stationary at dim 512 (3..5:
 * na >= 2048, 65 <= nb <= 256) -- or -1 where they refuse the sizes or return without a launch (na or nb 0).  The
 * environment switches BFF_GEMM_BANK (0: paths 3..5 become 2) and BFF_GEMM_STAGE (other than 2: path 3 becomes 4) are
 * read once per process.  The launcher switches on this same function. */
int bff_cosine_gemm_path(int32_t na, int32_t nb, int32_t dim);
/* a24 -- compute_avg_description_encodings (SEG:324-337): per class c, rows [offs[c], offs[c+1]) of desc (float16 or
 * float32 [n][dim]) are L2-normalised (eps 1e-12 as F.normalize), averaged, and the mean is normalised again;
 * out: same dtype [n_classes][dim]; float32 arithmetic. */
int bff_description_means(const void *desc, const int32_t *offs, int32_t n_classes, int32_t dim, int32_t dtype,
                          void *out, void *stream);

/* a21 -- the per-class text cosines in the dtype of the embeddings: cos[i][j] with every tensor op of
 *   (e1 @ e2.T) / (e1.norm() * e2.norm().T)  (compute_clip_similarity R:109-114) rounded to that dtype, so that
 * the SET of similarities the class threshold is taken from (R:321-324) ties exactly where the reference's
 * does (fp16 CLIP on a GPU: multiples of 2^-11).  dtype 0: a, b float32; dtype 1: a, b float16; cos float32
 * (holding float16 values for dtype 1); float64 accumulation; any dim. */
int bff_cosine_rows(const void *a, int32_t na, const void *b, int32_t nb, int32_t dim, int32_t dtype,
                    float *cos, void *stream);


/* ------------------------------------------------------------------------------------------
 * Groups formed on the device (P:203-226 without the host round trip) and the whole scene in one call.
 */
#define BFF_GROUP_CAP 256         /* groups the device forms by itself (= rows of the fused overlap pass): the default ... */
#define BFF_GROUP_CAP_MAX 512     /* ... and the largest capacity a workspace may ask for (bff_scene_workspace.group_cap) */
#define BFF_SIGNATURE_BITS 30     /* bff_row_stats signatures are 30-bit keys */

/* Device twin of bff_host_component_csr for at most `cap` <= BFF_GROUP_CAP_MAX kept groups.  comp[i] = smallest row index
 * of i's component (bff_merge_components) -- an INPUT when parent == NULL; with parent (the disjoint-set forest
 * bff_merge_components leaves behind when called with comp == NULL) comp is an OUTPUT, flattened here on the way.
 * Outputs (device): info[4] = {K kept groups (may exceed cap), flags (bit 0:
 * K > cap, bit 1: min_members <= 0 and empty components exist -- both: use the host path), largest group, number of
 * 32-member slices}; sizes[cap], first[cap] (= smallest member = where the group's label comes from), offs[cap+1],
 * members[n_rows] (ascending inside a group), slices[3 * bff_group_slice_cap(n_rows, cap)] (work items of
 * bff_or_reduce_grouped); count: scratch int32 [n_rows] (count_is_zero != 0: the caller has cleared it). */
int32_t bff_group_slice_cap(int32_t n_rows, int32_t cap);
int bff_group_components(int32_t *comp, int32_t *parent, const int32_t *area, int32_t n_rows, float iou_thres,
                         int32_t min_members, int32_t cap, int32_t *count, int32_t count_is_zero, int32_t *info,
                         int32_t *sizes, int32_t *first, int32_t *offs, int32_t *members, int32_t *slices, void *stream);
/* bff_or_reduce_groups for those groups: out [cap][nw] (zeroed here; rows >= K stay zero), conf_mean [cap] in the
 * confidence dtype.  chunk_mask (optional, the rows' chunk flags): long rows are read through it. */
int bff_or_reduce_grouped(const uint64_t *rows, int64_t nw, int32_t n_rows, const int32_t *info, int32_t cap,
                          const int32_t *offs, const int32_t *members, const int32_t *slices, uint64_t *out,
                          const void *conf, int32_t conf_dtype, void *conf_mean, const uint64_t *chunk_mask, void *stream);
/* bff_resolve_overlaps with the row count on the device (*k_dev <= k_cap, else nothing is touched). */
int bff_resolve_overlaps_dev(uint64_t *rows, int32_t k_cap, int64_t nw, const int32_t *size, const uint64_t *keep,
                             int32_t *before, int32_t *after, const int32_t *k_dev, void *stream);
/* out[r] bit perm[s] = in[r] bit s, set bits only (undoes the spatial point sort by scatter: aggregated rows are
 * sparse); out must be zero; rows >= *k_dev (when given) are skipped. */
int bff_scatter_bits(const uint64_t *rows_in, int32_t n_rows, int64_t nw_in, const int32_t *perm, int64_t n,
                     int64_t nw_out, uint64_t *rows_out, const int32_t *k_dev, void *stream);
/* bff_cross_popcount when only the first *k_dev rows of b's leading `lead` rows (and of a, with limit_a) are
 * non-zero: tiles inside the zero part are skipped; inter is zeroed first. */
int bff_cross_popcount_dev(const uint64_t *a, int32_t na, const uint64_t *b, int32_t nb, int64_t nw, int32_t *inter,
                           const int32_t *k_dev, int32_t limit_a, int32_t lead, void *stream);
/* bff_clear_flagged_chunks unless *veto != 0 (device flag). */
int bff_clear_flagged_chunks_unless(uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *chunk_mask,
                                    const int32_t *veto, void *stream);

/* Row directory of the 2-D masks: what the sweep's look-up mode (bff_project_views_lookup) asks instead of a decoded
 * image.  Inputs: the run tables of bff_rle_to_maskbits (per mask sorted, disjoint, non-empty runs inside
 * [0, height * width)) for n_masks masks.  Outputs (formats: beyond_fixed_forms_amd/csrc/mask_rows.h):
 *   mask_tab  uint32 [n_masks + 1][4], 16-byte aligned: per mask its box (c0 | R0 << 16, c1 | R1 << 16; R0 / R1 the rows of
 *             its first / last pixel, c0 / c1 the smallest / largest column a run touches, full width when a run crosses
 *             a row end; a mask without runs: 0xffffffff, 0), dir_offs (exclusive scan of the boxes' heights, computed on the
 *             device) and its first run; entry n_masks closes the table with the totals
 *   mask_dir  uint32, capacity n_masks * height: one entry per row of every box for the runs that intersect the row --
 *             0 (none), cs | ce << 15 (one run, clipped to the row), or 1 << 31 | count << 27 | first run relative to the
 *             mask, count saturated at 15 = "search from there to the mask's last run"
 * width, height < 2^15.  Deterministic: every word depends on the run tables only. */
int bff_mask_row_directory(const int32_t *run_start, const int32_t *run_end, const int32_t *mask_run_offs,
                           int32_t n_masks, int32_t height, int32_t width, uint32_t *mask_tab, uint32_t *mask_dir,
                           void *stream);
/* 1: bff_scene_project looks masks up in the row directory for images of this size with n_masks masks in all; 0: it decodes
 * them (BFF_MASK_LOOKUP=dense, read once per process, or an image the packed entries / the sweep's LDS do not hold). */
int32_t bff_mask_lookup_rows(int32_t height, int32_t width, int64_t n_masks);
/* bff_project_views / bff_project_views_u16 with the masks looked up in the row directory: same outputs, bit for bit, for
 * run tables under the contract above.  depth_layout -1: `depth` is float32 [n_depth][height * width] (depth_h / depth_w
 * unused), else as bff_project_views_u16.  view_mask_offs names a frame's masks (frame_mask[f] indexes it). */
int bff_project_views_lookup(const double *xyz, int64_t n_points, int64_t n_pad,
                             const double *inv_pose, const double *cam_intr_host, int32_t n_frames,
                             const void *depth, int32_t depth_h, int32_t depth_w, int32_t depth_layout,
                             const int32_t *depth_index, int32_t height, int32_t width, double depth_thresh,
                             const uint32_t *mask_tab, const uint32_t *mask_dir, const int32_t *run_start,
                             const int32_t *run_end, const int32_t *view_mask_offs, int32_t word_bits,
                             const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                             const int32_t *frame_flags,
                             uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                             int32_t *masked_count, int32_t *viewed_count, const double *tile_bounds,
                             void *stream);

/* The visibility table of a resident scene: what the sweep's geometry and depth test answer per (depth slot, point),
 * kept from call to call (it depends on the cloud, the poses, the depth frames and depth_thresh -- not on the masks).
 * For slot s (what depth_index[f] holds), sorted point word w and lane l, with stride = bff_visibility_words(n_points)
 * (the words of whole sweep blocks, >= ceil(n_points / 64)):
 *   vis_mask uint64 [n_slots][stride]  bit l set iff point 64 w + l passes exactly the sweep's test in that frame (valid,
 *            u and v in bounds on the doubles, depth != 0, |z - depth| < depth_thresh)
 *   vis_off  uint32 [n_slots][stride]  exclusive prefix of the popcounts in (slot, word) order
 *   vis_pix  uint32 [n_pixels]         each visible pair's pixel u | v << 16 at vis_off + popcount(mask & lanes below l)
 * height, width < 2^15, fewer than 2^32 visible pairs.
 * bff_visibility_table builds it on `stream`: 1 the mask pass (bff_count_viewed's kernel and arithmetic, storing the ballots;
 * frame s reads depth slot s with pose slot_inv_pose[s]), 2 the offsets and *n_pixels (device, uint64), 3 the pixel pass
 * (geometry only, for words with a set bit; pairs at or beyond pix_cap are dropped).  phase 0: all three with a caller's
 * bound pix_cap; phase 1: steps 1 and 2 (vis_pix unused); phase 2: step 3 alone, after the caller has read *n_pixels and
 * allocated vis_pix.  Nothing in it waits for the host.  `depth`, `depth_h`, `depth_w`, `depth_layout`, `tile_bounds` as
 * bff_project_views_lookup. */
int64_t bff_visibility_words(int64_t n_points);
/* bytes[3] = sizes of vis_mask, vis_off and of vis_pix for n_pixels visible pairs */
int bff_visibility_table_bytes(int64_t n_points, int32_t n_slots, int64_t n_pixels, int64_t *bytes);
int bff_visibility_table(const double *xyz, int64_t n_points, int64_t n_pad, const double *slot_inv_pose,
                         const double *cam_intr_host, int32_t n_slots, const void *depth, int32_t depth_h,
                         int32_t depth_w, int32_t depth_layout, int32_t height, int32_t width, double depth_thresh,
                         const double *tile_bounds, uint64_t *vis_mask, uint32_t *vis_off, uint32_t *vis_pix,
                         int64_t pix_cap, uint64_t *n_pixels, int32_t phase, void *stream);
/* pixel passes issued by this process so far (one per table built) */
int64_t bff_visibility_builds(void);
/* bff_project_views_lookup answered from the table: same grid, frame tiles, outputs (bit for bit) and profiling events; the
 * cloud, the poses and the depth frames are not read.  The table must have been built for the scene's cloud, the frames'
 * poses and depth slots, and the depth_thresh the caller would have swept with. */
int bff_project_views_cached(int64_t n_points, int32_t n_frames, const int32_t *depth_index, int32_t height,
                             int32_t width, const uint64_t *vis_mask, const uint32_t *vis_off, const uint32_t *vis_pix,
                             const uint32_t *mask_tab, const uint32_t *mask_dir, const int32_t *run_start,
                             const int32_t *run_end, const int32_t *view_mask_offs, int32_t word_bits,
                             const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                             const int32_t *frame_flags, uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                             int32_t *masked_count, int32_t *viewed_count, void *stream);

/* Pixel-sorted companion of the visibility table: the visible pairs of every slot ordered by (flat pixel, point), so that a
 * run [start, end) of a 2-D mask covers one contiguous range of its frame's slot.
 *   vis_spix     uint32 [n_pixels]           flat pixel v * width + u
 *   vis_spt      uint32 [n_pixels]           point index
 *   vis_rowstart uint32 [n_slots][height+1]  absolute position of the slot's first pair with pixel >= y * width; entry
 *                                            `height` is the slot's end (an empty slot: all equal)
 * A pure function of the table: a stable radix sort of the pairs, which arrive in (slot, point) order, on the 32-bit key
 * slot * height * width + pixel (n_slots * height * width <= 2^32), then one lower bound per (slot, image row).  No global
 * atomics.  temp == NULL: only *temp_bytes is written (size query, no launch); the scratch (12 bytes per pair + the
 * sort's own) is free again once the work on `stream` has run.  n_points == 0 or n_slots == 0: nothing is written. */
int bff_visibility_sorted(const uint64_t *vis_mask, const uint32_t *vis_off, const uint32_t *vis_pix, int64_t n_pixels,
                          int64_t n_points, int32_t n_slots, int32_t height, int32_t width, uint32_t *vis_spix,
                          uint32_t *vis_spt, uint32_t *vis_rowstart, void *temp, size_t *temp_bytes, void *stream);
/* bytes[3] = sizes of vis_spix, vis_spt and vis_rowstart: the persistent bytes the companion adds to the table's */
int bff_visibility_sorted_bytes(int32_t n_slots, int32_t height, int64_t n_pixels, int64_t *bytes);

/* bff_project_views_cached asked from the masks' side (same outputs, bit for bit, and profiling events): one workgroup per
 * instance row = mask m of frame f walks the mask's runs over the slot's pixel-sorted pairs and ORs the covered points into
 * a bitmap of the row in LDS, then stores its non-zero 32-byte sectors and the row's chunk flags (plain stores: `rows` is
 * all zero on entry and a row belongs to one (frame, mask)); masked_count += the rows' column sums over the flagged chunks;
 * viewed_count (may be NULL) += the table's bits of the frames with flag bit 0.  No row directory.  chunk_mask is required.
 * The row must fit the LDS bound: bff_sweep_runs_ok(n_points) != 0 (64 KB: n_points <= 524 288; BFF_SWEEP_RUNS=0 answers 0
 * for every scene and BFF_SWEEP_RUNS_LDS_BYTES lowers the bound, both read per call) -- bff_scene_project asks it and
 * keeps bff_project_views_cached otherwise. */
int32_t bff_sweep_runs_ok(int64_t n_points);
int bff_project_views_runs(int64_t n_points, int32_t n_frames, const int32_t *depth_index, int32_t height, int32_t width,
                           const uint64_t *vis_mask, const uint32_t *vis_spix, const uint32_t *vis_spt,
                           const uint32_t *vis_rowstart, const int32_t *run_start, const int32_t *run_end,
                           const int32_t *mask_run_offs, const int32_t *view_mask_offs, int32_t word_bits,
                           const int32_t *frame_mask, const int32_t *frame_rowbase, const int32_t *frame_nmask,
                           const int32_t *frame_flags, uint64_t *rows, int64_t n_rows, int64_t nw, uint64_t *chunk_mask,
                           int32_t *masked_count, int32_t *viewed_count, void *stream);

/* Device-resident inputs of one scene (what scene.prepare_scene uploads; all pointers are device pointers). */
typedef struct bff_scene {
    int64_t n_points, n_pad, nw;
    const double *xyz;              /* [3][n_pad] */
    const double *tile_bounds;      /* bff_point_tile_bounds table or NULL */
    const double *inv_pose;         /* [n_frames][16] */
    double cam_intr[9];
    const float *depth;             /* [n_depth][height * width] metres, or NULL when depth_raw is given */
    const void *depth_raw;          /* sensor-resolution frames in layout `depth_tiled` (bff_project_views_u16), or NULL */
    const int32_t *depth_index, *frame_mask, *frame_rowbase, *frame_nmask, *frame_flags;   /* [n_frames] */
    const int32_t *run_start, *run_end, *mask_run_offs, *view_mask_offs;                     /* 2-D RLE run tables */
    const void *conf;               /* [n_rows] float16 / float32 */
    const int32_t *label_id;        /* [n_rows] */
    const int32_t *unsort;          /* [n_points] position of original point o in the sorted cloud, or NULL */
    const int32_t *perm;            /* [n_points] original index of sorted position s (inverse of unsort), or NULL */
    const int32_t *s1_run_start, *s1_run_end, *s1_row_run_offs;     /* stage-1 run tables or NULL */
    int32_t height, width, n_frames, n_mviews, word_bits, n_rows, conf_f16, n_label_ids, s1_rows, depth_h, depth_w,
            depth_tiled;            /* depth_layout of bff_project_views_u16: 0 uint16 rows, 1 uint16 tiles, 2 float32 tiles */
    const uint64_t *vis_mask;       /* the scene's visibility table (bff_visibility_table, built for params.depth_thresh) or */
    const uint32_t *vis_off, *vis_pix;     /* NULL: with all three set and masks looked up, the sweep is bff_project_views_cached */
    const uint32_t *vis_spix, *vis_spt, *vis_rowstart;    /* the table's pixel-sorted companion (bff_visibility_sorted) or NULL:
                                       with these set too and bff_sweep_runs_ok(n_points), the sweep is bff_project_views_runs
                                       and no row directory is built */
} bff_scene;

typedef struct bff_scene_params {
    double depth_thresh;            /* 0.08 at P:438,565 */
    double filter_fraction;         /* occurance_threshold / detected_ratio_threshold */
    float iou_thres;
    int32_t min_members;            /* cfg.min_aggragated_masks */
    int32_t filter_mode;            /* 0 none, 1 occurrence (P:512-522), 2 detection ratio (P:524-578) */
    int32_t filter_sort;            /* != 0: threshold by sorting all values (after header word BFF_HDR_OVERFLOW was set) */
} bff_scene_params;

/* Scratch of bff_scene_project, allocated by the caller for the scene's sizes (beyond_fixed_forms_amd/pipeline.py).
 * `rows` must be all zero on entry; it is all zero again when the call's work has run on the fast path.
 * Masks are looked up in the row directory (mask_tab, mask_dir) when bff_mask_lookup_rows(height, width, n_rows) says so;
 * then maskbits, labels and segmap are not used and may be NULL.  Otherwise the directory buffers may be NULL.
 * Every buffer the call's steps expect zeroed -- masked, viewed, count, chunk_mask, segmap, hdr, agg, merge_scratch
 * and (clouds that use the chunk bound) chunk_pop -- must lie inside ONE allocation of `zero_bytes` bytes
 * starting at `masked`: the call clears it with a single fill (checked; beyond_fixed_forms_amd/pipeline.py lays it out). */
typedef struct bff_scene_workspace {
    void *maskbits; uint32_t *segmap;  /* word plane and two-word segment bitmap of bff_rle_to_labels */
    uint8_t *labels;                /* palette blocks, [n_mviews][bff_label_plane_stride(H*W)] */
    uint64_t *rows, *chunk_mask, *keep, *tile_mask, *agg, *both;
    int32_t *masked, *viewed, *sel_scratch, *area, *mean_word, *order, *parent, *comp, *count;
    int32_t *gmembers, *goffs, *slices;
    uint32_t *pair_scratch;         /* bff_point_threshold_scratch_words(n_points) */
    float *vals, *vals_sorted;
    uint32_t *hist, *merge_scratch;
    uint16_t *chunk_pop;            /* [n_rows][64 * chunk-mask words] */
    int64_t *sig, *sig_keys, *sig_sorted;
    void *sort_temp;
    uint32_t *mask_tab, *mask_dir;  /* bff_mask_row_directory: [n_rows + 1][4] and n_rows * height words */
    size_t sort_temp_bytes;
    size_t zero_bytes;              /* size of the block that starts at `masked` (see above) */
    int32_t *hdr;                   /* device, bff_scene_header_words(s1_rows, group_cap) int32 */
    int32_t *hdr_host;              /* pinned host mirror of the same size */
    int32_t group_cap;              /* BFF_GROUP_CAP or BFF_GROUP_CAP_MAX: kept groups formed on the device; agg, both and the
                                       header are sized by it.  More groups than that: header flag, the host continues */
    int32_t pad_;
    void *heavy_stream;             /* optional hipStream_t for the chip-filling kernels (decode, sweep, tile pass): callers that keep
                                       several scenes in flight give the SAME stream to a few of them, so that at most as many
                                       chip-filling kernels run side by side as there are heavy streams while the scenes' chains of
                                       small kernels overlap freely.  NULL: everything on the call's stream */
    void *events[4];                /* four hipEvent_t of this workspace for the hand-overs between the two streams (heavy_stream != NULL) */
    void *aux_stream;               /* optional second hipStream_t of this workspace: the point filter's threshold chain (four small
                                       launches that only the overlap resolution at the end waits for) runs there, beside the row
                                       statistics / tile order / components chain.  NULL: everything in one chain */
    void *aux_events[2];            /* two hipEvent_t for the fork after the sweep and the join before the overlap resolution */
} bff_scene_workspace;

/* Header layout (int32 words). */
#define BFF_HDR_K 0                 /* info[4] of bff_group_components: K, flags, largest group, slices */
#define BFF_HDR_NUNIQUE 4           /* distinct filter values (0: the reference would raise IndexError) */
#define BFF_HDR_THR 5               /* float32 threshold */
#define BFF_HDR_OVERFLOW 6          /* != 0: more distinct filter values than bff_point_threshold_pairs holds: run the
                                       scene again with params.filter_sort = 1 (everything after the sweep is void) */
/* cap = the workspace's group_cap (BFF_GROUP_CAP or BFF_GROUP_CAP_MAX) */
#define BFF_HDR_SIZES(cap) 16                         /* [cap] members per group */
#define BFF_HDR_FIRST(cap) (16 + (cap))               /* [cap] smallest member of the group */
#define BFF_HDR_BEFORE(cap) (16 + 2 * (cap))          /* [cap] popcount before overlap resolution (P:592) */
#define BFF_HDR_AFTER(cap) (16 + 3 * (cap))           /* [cap] popcount after overlaps + point filter (P:596) */
#define BFF_HDR_CONF(cap) (16 + 4 * (cap))            /* [cap] confidence means, in the confidence dtype, packed */
#define BFF_HDR_CROSS(cap) (16 + 5 * (cap))           /* [s1_rows][cap + s1_rows] stage-1 x (stage-2 groups | stage-1) */
int32_t bff_scene_header_words(int32_t s1_rows, int32_t cap);
int32_t bff_scene_struct_bytes(int32_t which);     /* 0 bff_scene, 1 bff_scene_params, 2 bff_scene_workspace */

/* The whole device side of one scene on `stream`, ending with an asynchronous copy of the header into
 * ws->hdr_host: nothing in it waits for the host.  After the stream has reached that copy the host reads K,
 * flags, sizes, first members, before/after counts, confidence means and the refinement's intersections from
 * the header; ws->both holds the K aggregated, overlap-resolved, filtered rows in the caller's point order followed
 * by the decoded stage-1 rows.  flags != 0: the group tables are incomplete -- continue from ws->comp / ws->area on
 * the host (projection._projection_back), ws->rows is then still intact. */
int bff_scene_project(const bff_scene *scene, const bff_scene_params *params, const bff_scene_workspace *ws,
                      void *stream);
/* bff_scene_project with the detection ratio's denominator given: viewed_in int32 [n_points] (the scene's sorted point
 * order) as bff_count_viewed computes it over the scene's viewed frames.  The sweep then counts no visibility (pass only
 * the class's mask frames, frame_flags all 0) and the point filter reads viewed_in instead of ws->viewed.  viewed_in ==
 * NULL is bff_scene_project. */
int bff_scene_project_viewed(const bff_scene *scene, const bff_scene_params *params, const bff_scene_workspace *ws,
                             const int32_t *viewed_in, void *stream);

/* ------------------------------------------------------------------------------------------
 * Ingestion: cloud layout on the device.  pts: float64 [n][stride] exactly as <scene>.npy
 * holds it (P:387: stride 6, xyz first).  Writes the structure-of-arrays cloud the sweep reads (soa [3][n_pad], pad
 * zeroed) and, with sort != 0, orders the points along a 30-bit Morton curve over their bounding box first (same
 * codes and a stable sort as scene.morton_order on the host -> the same permutation): unsort[o] = position of
 * original point o, perm = its inverse.  codes: uint32 [2 n], box: float64 [6], temp: sort scratch (temp == NULL:
 * size query into *temp_bytes). */
int bff_cloud_layout(const double *pts, int64_t n, int64_t stride, int64_t n_pad, int32_t sort, double *soa,
                     int32_t *unsort, int32_t *perm, uint32_t *codes, double *box, void *temp, size_t *temp_bytes,
                     void *stream);

/* Measurement aid: the 128-byte lines of the depth and mask-word images that one sweep touches, as bitmaps (uint32
 * [n_frames][line_words], zeroed by the caller; line index = pixel / (pixels per 128 B)).  128 B per marked line is
 * the sweep's compulsory HBM traffic for these images (bench.py: roofline.compulsory).  label_lines != NULL: segmap is
 * bff_rle_to_labels' two-word bitmap; segments in palette form mark label_lines (128 pixels per line) instead. */
int bff_diag_sweep_lines(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                         const double *cam_intr_host, int32_t n_frames, const float *depth, const int32_t *depth_index,
                         int32_t height, int32_t width, double depth_thresh, const uint32_t *segmap, int32_t word_bits,
                         const int32_t *frame_mask, uint32_t *depth_lines, uint32_t *mask_lines, int64_t line_words,
                         uint32_t *label_lines, void *stream);
/* The same for bff_project_views_u16: depth_lines counts the 128-byte lines of the uint16 source frames (64 texels
 * per line; line_words >= ceil(ceil(depth_h * depth_w / 64) / 32) as well). */
int bff_diag_sweep_lines_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                             const double *cam_intr_host, int32_t n_frames, const void *depth_raw, int32_t depth_h,
                             int32_t depth_w, int32_t depth_layout, const int32_t *depth_index, int32_t height, int32_t width,
                             double depth_thresh, const uint32_t *segmap, int32_t word_bits, const int32_t *frame_mask,
                             uint32_t *depth_lines, uint32_t *mask_lines, int64_t line_words, uint32_t *label_lines,
                             void *stream);
/* Measurement aid: n_lanes lanes each read one float at element lane * stride of src (every element once per launch)
 * -- a gather with a known number of distinct cache lines, to calibrate the FETCH_SIZE counter (scripts/diag_membw.py). */
int bff_diag_gather(const float *src, int64_t n_lanes, int64_t stride, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D instances split into spatially connected parts (no counterpart in the reference).
 * The definition is connectivity on a voxel grid: a pure function of the inputs, independent of point order, thread
 * schedule and run.
 *
 * Inputs: points float64 [N][stride >= 3] in the caller's point order; a cell size c > 0, finite, in metres; rows
 * u64 [K][nw], nw >= ceil(N / 64), whose bits at positions >= N are ignored whatever they hold.
 *
 * Grid (class independent, built once per scene).  A point is finite when all three coordinates are.  lo[a] = the minimum
 * of coordinate a over the finite points; q[p][a] = floor((x[p][a] - lo[a]) / c) in float64 (IEEE subtraction, IEEE
 * division, floor: NumPy's np.floor((xyz - lo) / c), also where a coordinate sits exactly on a cell boundary).
 * Limit: q < 2^21 on every axis, else BFF_E_LIMIT.  key[p] = q0 + (q1 << 21) + (q2 << 42); keys[V] = the distinct keys
 * of the finite points, ascending; vox[p] = the rank of key[p] in keys, -1 for a non-finite point (it belongs to no cell
 * and appears in no output row); nbr[V][13] = for each cell the ranks of its 13 forward neighbours, the offsets
 * (d2, d1, d0) in {-1, 0, 1}^3 lexicographically greater than (0, 0, 0), in that order, -1 where the cell is empty or
 * would lie outside [0, 2^21) on an axis (the axis is tested, the key never wraps).
 *
 * Components of row k.  Its occupied cells are those holding at least one point of the row.  Two occupied cells are
 * linked when they differ by at most 1 on every axis (26-adjacency, corner contact included); a component is a class of
 * the transitive closure, its point count the number of the row's points in its cells, its anchor its smallest cell
 * rank.  Rows are independent: a cell shared by two rows links nothing between them.
 *
 * Output for min_points >= 1: every component with at least min_points points becomes an output row ("split"), ordered
 * by parent row ascending, point count descending, anchor ascending; or per parent row only the first of that order
 * ("largest").  The choice and the order are the host's (spatial.split_rows); the entry points below are the steps.
 *
 * Elements: the T occupied (row, cell) pairs, numbered in (row, cell) order:
 *   e = elem_offs[k] + prefix[k][v >> 6] + popcount(occ[k][v >> 6] below bit (v & 63)).
 * Limits: N, V < 2^31; K * ceil(V / 64) * 64 < 2^31 (so T < 2^31).  Zero sizes return 0 without a launch. */

/* box: u64 [6], min x, y, z then max x, y, z over the finite points as order-preserving integers (b = the double's bits;
 * b >> 63 ? ~b : b | 1 << 63); without a finite point the minima stay all ones. */
int bff_voxel_bounds(const double *points, int64_t n_points, int64_t stride, uint64_t *box, void *stream);
/* key: i64 [N], the cell key of every finite point, 2^63 - 1 for the others.  lo_host, hi_host: the box as doubles
 * (HOST pointers, 3 each); floor((hi - lo) / cell) >= 2^21 on an axis is BFF_E_LIMIT. */
int bff_voxel_keys(const double *points, int64_t n_points, int64_t stride, const double *lo_host, const double *hi_host,
                   double cell, int64_t *key, void *stream);
/* sorted_keys: `key` ascending (bff_argsort_i64 with 63 key bits).  head: i32 [N], 1 where a cell's first key stands. */
int bff_voxel_heads(const int64_t *sorted_keys, int64_t n_points, int32_t *head, void *stream);
/* order: the argsort (position i of sorted_keys holds point order[i]); heads_incl: i64 [N], the inclusive prefix sum of
 * head; n_voxels = its last entry.  Writes vox i32 [N] and keys i64 [V]. */
int bff_voxel_ranks(const int64_t *sorted_keys, const int32_t *order, const int64_t *heads_incl, int64_t n_points,
                    int64_t n_voxels, int32_t *vox, int64_t *keys, void *stream);
/* nbr: i32 [V][13]. */
int bff_voxel_neighbours(const int64_t *keys, int64_t n_voxels, int32_t *nbr, void *stream);

/* occ: u64 [K][vw], vw = ceil(V / 64), cleared here: bit v of row k = the row holds a point of cell v.  prefix: i32
 * [K][vw], the row's set bits below each word; row_total: i32 [K], the row's set bits.  The caller turns row_total into
 * elem_offs i32 [K + 1] (exclusive prefix sum; elem_offs[K] = T). */
int bff_split_occupancy(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *vox,
                        int64_t n_voxels, uint64_t *occ, int32_t *prefix, int32_t *row_total, void *stream);
/* parent: i32 [T].  Afterwards parent[e] is the smallest element of e's component (the anchor's element), whatever the
 * interleaving of the compare-and-swap unions was. */
int bff_split_union(const uint64_t *occ, const int32_t *prefix, const int32_t *elem_offs, int32_t n_rows,
                    int64_t n_voxels, const int32_t *nbr, int32_t n_elems, int32_t *parent, void *stream);
/* count: i32 [T], at a root the component's points (0 elsewhere).  kept: i32 [1 + T][2]: kept[0][0] = the number of
 * roots with count >= min_points, kept[1 + i] = (root element, points) of the i-th in an order that depends on the run
 * (the host sorts them). */
int bff_split_count(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *vox,
                    int64_t n_voxels, const uint64_t *occ, const int32_t *prefix, const int32_t *elem_offs,
                    const int32_t *parent, int32_t n_elems, int32_t min_points, int32_t *count, int32_t *kept,
                    void *stream);
/* table: i32 [T], root element -> output row in [0, n_out) or -1.  out: u64 [n_out][nw], cleared here; every point of a
 * parent row lands in at most one output row. */
int bff_split_emit(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *vox,
                   int64_t n_voxels, const uint64_t *occ, const int32_t *prefix, const int32_t *elem_offs,
                   const int32_t *parent, int32_t n_elems, const int32_t *table, int32_t n_out, uint64_t *out,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D instances snapped to superpoints (the reference only loads superpoint files:
 * evaluation/dataset/scannet_loader.py:92, read_spp).  Integer arithmetic throughout: a pure function of the inputs,
 * independent of thread schedule and run.
 *
 * Inputs: spp, one integer id per point of the cloud in the caller's point order (arbitrary int64 values: not dense, not
 * sorted); rows u64 [K][nw], nw >= ceil(N / 64), whose bits at positions >= N are ignored whatever they hold and are
 * zero in every output; ratio in (0, 1]; a mode.
 *
 * Index (class independent, built once per scene).  The distinct ids >= 0, ascending, are the S superpoints.  seg[p] =
 * the rank of point p's id, -1 for a negative id; size[s] = the number of points of superpoint s; order lists the
 * points of superpoint s at order[offs[s] .. offs[s + 1]) in ascending point index (a stable sort); free = one bit row
 * holding the points with seg = -1.  A point with a negative id belongs to no superpoint: its bit passes through every
 * step unchanged.  The index needs no entry point of its own: ids < 0 -> 2^63 - 1, bff_argsort_i64 with 63 key bits,
 * bff_voxel_heads, bff_voxel_ranks (seg = its vox, the ids = its keys), a prefix sum for offs, a packed comparison
 * for free.
 *
 * need[s] = max(1, ceil(float64(ratio) * size[s])): product and ceiling in float64, once per (index, ratio), outside
 * the kernels, which compare integers only (ratio 0.55 and 100 points need 56: 0.55 * 100 = 55.00000000000001).
 * count[k][s] = the number of points of row k in superpoint s.
 * Mode "snap": output row k = the union of every superpoint with count[k][s] >= need[s], plus rows[k] & free.  Rows are
 * independent and may overlap.
 * Mode "exclusive": among the rows that reach need[s], superpoint s goes to the one with the largest count, a tie to the
 * smallest row index; that row gets the whole superpoint and no other row any of it.  Free points as in "snap".
 * After: rows with fewer than min_points >= 1 points are dropped, the others keep their order (the host's:
 * superpoints.snap_rows).
 *
 * Limits: N, S < 2^31; K * S < 2^31, else BFF_E_LIMIT.  Zero sizes return 0 without a launch.  No call allocates or
 * synchronises. */

/* seg: i32 [N].  count: i32 [K][S], cleared here.  Entries of seg outside [0, S) count nowhere. */
int bff_spp_count(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const int32_t *seg,
                  int64_t n_segments, int32_t *count, void *stream);
/* need: i32 [S].  owner: i32 [S], the row that takes superpoint s in "exclusive" mode, -1 = none reaches need[s]. */
int bff_spp_owner(const int32_t *count, int32_t n_rows, int64_t n_segments, const int32_t *need, int32_t *owner,
                  void *stream);
/* owner: NULL = "snap" (superpoint s goes to every row with count[k][s] >= need[s]), else "exclusive" (to row owner[s]).
 * order: i32 [N']; offs: i32 [S + 1], ascending, offs[S] = N' = the points with seg >= 0.  out: u64 [K][nw], on entry
 * rows & free with the bits at positions >= N zero; the chosen superpoints' points are ORed in.  An entry of order
 * outside [0, 64 * nw) sets nothing. */
int bff_spp_fill(const int32_t *count, int32_t n_rows, int64_t n_segments, const int32_t *need, const int32_t *owner,
                 const int32_t *order, const int32_t *offs, uint64_t *out, int64_t nw, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D instances lifted from a subsampled cloud to the full cloud (no counterpart in the
 * reference).  A pure function of the inputs, independent of thread schedule and run; tests/lift_ref.py restates it in
 * NumPy and the results are equal bit for bit.
 *
 * Subsample.  grid = the grid above (bff_voxel_*) of the cloud at cell v.  The representative of an occupied cell is the
 * smallest point index in it; a non-finite point has no cell and is never sampled.  sample: int32 [V], the
 * representatives in ascending point index, so points[sample] keeps the file's order.  It needs no entry point: a
 * minimum of the point index per cell rank (vox), then the marked points in order (lift.subsample).
 *
 * Nearest source within a radius.  Inputs: source points S float64 [M][>= 3], a radius r > 0, finite, query points Q
 * float64 [N][>= 3].  The source index is the grid above of S with cell c = r, plus the points of every cell in
 * ascending point index (order, offs: bff_spp_fill's lists with the cells as superpoints).  The query's cell is
 * floor((x - lo) / c) per axis in float64, with the grid's lo and bff_voxel_keys' IEEE operations, and is tested on the
 * doubles before any conversion: a query with a non-finite coordinate has nn = -1, and so has one whose cell lies outside
 * [-1, 2^21] on some axis.  Candidates: the source points whose cell differs from the query's by at most 1 on every
 * axis.  d2 = (dx * dx + dy * dy) + dz * dz with dx = q.x - s.x, every operation rounded to float64, no fma.  nn[p] =
 * the candidate with the smallest d2 among those with d2 <= float64(r) * float64(r), equal d2 to the smallest source
 * index; -1 without one.  d2[p] = that squared distance, +inf without one.
 *
 * Lift.  rows_in u64 [K][nw_in] over the M source points, nw_in >= ceil(M / 64); rows_out u64 [K][ceil(N / 64)].  Bit p
 * of output row k = bit nn[p] of input row k where 0 <= nn[p] < M, and 0 for any other value of nn[p] (-1, and anything
 * out of range: the device never follows a bad index).  Input bits at positions >= M are ignored, output bits at
 * positions >= N are zero.  Two steps: the rows transposed into one column of ceil(K / 64) words per source point, then
 * one gather of a column per target point (K gathers of a bit per target is the wrong shape at K ~ 100).
 *
 * Limits: N, M, V < 2^31; K * ceil(N / 64) < 2^31 and M * ceil(K / 64) < 2^31 words, else BFF_E_LIMIT.  Zero sizes
 * return 0 without a launch.  No call allocates or synchronises. */

/* src: f64 [n_source][3], the source points that have a cell, in (cell, point index) order; order: i32 [n_source], the
 * source index of each; offs: i32 [V + 1] into both, offs[V] = n_source; keys: i64 [V], the grid's distinct keys,
 * ascending.  lo_host: the grid's minimum (HOST pointer, 3 doubles); cell: the grid's cell (= radius by the definition
 * above).  queries: f64 [n_queries][stride >= 3].  nn: i32 [n_queries]; d2: f64 [n_queries] or NULL.  With n_voxels = 0
 * every query gets -1. */
int bff_nn_search(const double *src, const int64_t *keys, const int32_t *offs, const int32_t *order, int64_t n_voxels,
                  int64_t n_source, const double *lo_host, double cell, double radius, const double *queries,
                  int64_t n_queries, int64_t stride, int32_t *nn, double *d2, void *stream);
/* cols: u64 [n_source][ceil(n_rows / 64)] (caller-provided scratch, written whole): bit k of cols[s] = bit s of row k,
 * the bits of rows >= n_rows zero. */
int bff_rows_to_columns(const uint64_t *rows_in, int32_t n_rows, int64_t nw_in, int64_t n_source, uint64_t *cols,
                        void *stream);
/* cols: what bff_rows_to_columns wrote for the same n_rows and n_source.  nn: i32 [n_target].  rows_out: u64
 * [n_rows][ceil(n_target / 64)], written whole. */
int bff_lift_bits(const uint64_t *cols, int64_t n_source, int32_t n_rows, const int32_t *nn, int64_t n_target,
                  uint64_t *rows_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D instances clustered by density: DBSCAN(eps, min_samples) with a deterministic border rule (DESIGN.md section 7j;
 * no counterpart in the reference).  A pure function of the inputs, independent of point order, thread schedule and run;
 * tests/density_ref.py restates it in NumPy by brute force and the results are equal bit for bit.
 *
 * Inputs: points float64 [N][stride >= 3] in the caller's point order; eps > 0, finite, in metres; min_samples >= 1; rows
 * u64 [K][nw], nw >= ceil(N / 64), whose bits at positions >= N are ignored whatever they hold and are zero in every
 * output; min_points >= 1; a mode.
 *
 * Finite points.  A point is finite when all three coordinates are.  A non-finite point has no cell, is nobody's
 * neighbour and appears in no output row.
 * Distance.  d2(p, q) = (dx * dx + dy * dy) + dz * dz with dx = x[p] - x[q], every operation rounded to float64, no fma
 * (bff_nn_search's expression; the unit is compiled with -ffp-contract=off).
 * Neighbours.  p and q are neighbours when d2 <= float64(eps) * float64(eps).  A point is its own neighbour.
 *
 * Rows are independent: a point shared by two rows links nothing between them.  Per row k, over its finite set points:
 *   Core.     count[p] = the row's points that are neighbours of p, p included; p is core when count[p] >= min_samples
 *             (sklearn's convention).
 *   Clusters. Two core points are linked when they are neighbours; a cluster is a class of the transitive closure over
 *             the core points, its anchor its smallest core point index.
 *   Border.   A non-core point with at least one core neighbour joins the cluster of its nearest core neighbour: the
 *             smallest d2, equal d2 going to the smallest point index.  (sklearn gives such a point to whichever cluster
 *             reaches it first in index order: the one deliberate difference, and why the result does not depend on a
 *             traversal.)
 *   Noise.    Everything else; it is in no output row.
 *
 * Output, in the split's shape: mode "split": every cluster with at least min_points points (core + border) becomes a
 * row, ordered by parent row ascending, point count descending, anchor ascending; mode "largest": per parent row only the
 * first of those.  The choice and the order are the host's (density.cluster_rows); the entry points below are the steps.
 *
 * The search index is the lift's (bff_nn_search above): the grid (bff_voxel_*) of the cloud with the points of every cell
 * in ascending point index and the cloud gathered into that order.  Its cell is float64(eps) * (1 + 2^-20), not eps: two
 * points within eps of each other then differ by less than 1 - 9e-7 cells on every axis before rounding, the quotient
 * floor((x - lo) / cell) carries an error below 2^-31 cells (q < 2^21), so their cells differ by at most 1 on every axis
 * and the 27 cells around a point hold every neighbour -- with cell = eps a pair at d2 == eps^2 can round two cells
 * apart.  The distance test is the statement's, so the larger cell changes no result.
 *
 * How the steps are cut.  All passes run one wave per 64-bit word of a row, lane = point, in the caller's point order.
 *   bff_dbscan_elements  set = rows & finite with the bits >= N cleared; the elements are its set bits, numbered in (row,
 *                        point) order: e = elem_offs[k] + prefix[k][p >> 6] + popcount(set[k][p >> 6] below bit (p & 63))
 *   bff_dbscan_core      the density pass: core u64 [K][ceil(N / 64)]
 *   bff_dbscan_link      unions over the core elements (compare-and-swap, the larger root under the smaller), a flatten
 *                        that only reads, then every non-core element's slot written by its own thread: parent[e] = the
 *                        smallest core element of e's cluster, -1 for noise.  The forest's kernels are
 *                        bff_split_union's and the walk over a point's 27 cells is bff_nn_search's (csrc/cells.h)
 *   bff_split_count, bff_split_emit   unchanged, called with vox[p] = p (-1 for a non-finite point), n_voxels = N, rows =
 *                        occ = set: they accept any point-to-cell map, a parent of -1 is followed nowhere, and a root
 *                        is an element with parent[e] == e.  Within a row, element order is point order, so the root of a
 *                        cluster is its anchor.
 * Limits: N < 2^31; the grid's 2^21 cells per axis (bff_voxel_keys); K * ceil(N / 64) * 64 < 2^31 bits, which bounds the
 * elements T; else BFF_E_LIMIT from a host-side check before any launch.  Zero sizes return 0 without a launch.  No entry
 * point allocates or synchronises. */

/* finite: u64 [ceil(N / 64)], bit p = point p has a cell.  set: u64 [K][ceil(N / 64)]; prefix: i32 [K][ceil(N / 64)], the
 * row's set bits below each word; row_total: i32 [K].  The caller turns row_total into elem_offs i32 [K + 1] (exclusive
 * prefix sum; elem_offs[K] = T). */
int bff_dbscan_elements(const uint64_t *rows, int32_t n_rows, int64_t nw, int64_t n_points, const uint64_t *finite,
                        uint64_t *set, int32_t *prefix, int32_t *row_total, void *stream);
/* points: f64 [n_points][stride >= 3], the queries.  cloud, keys, offs, order, n_voxels, n_source, lo_host, cell: the
 * index as bff_nn_search takes it (src = cloud), n_source <= n_points the finite points, cell >= eps.  core: u64
 * [K][ceil(N / 64)], cleared here.  The count of a point stops at min_samples; the row's bit of a candidate is tested
 * before its distance.  An entry of order outside [0, N) is nobody's neighbour.  With n_voxels = 0 core stays zero. */
int bff_dbscan_core(const uint64_t *set, int32_t n_rows, int64_t n_points, const double *points, int64_t stride,
                    const double *cloud, const int64_t *keys, const int32_t *offs, const int32_t *order, int64_t n_voxels,
                    int64_t n_source, const double *lo_host, double cell, double eps, int32_t min_samples, uint64_t *core,
                    void *stream);
/* parent: i32 [n_elems], n_elems = T, written whole. */
int bff_dbscan_link(const uint64_t *set, const uint64_t *core, const int32_t *prefix, const int32_t *elem_offs, int32_t n_rows,
                    int64_t n_points, const double *points, int64_t stride, const double *cloud, const int64_t *keys,
                    const int32_t *offs, const int32_t *order, int64_t n_voxels, int64_t n_source, const double *lo_host,
                    double cell, double eps, int32_t n_elems, int32_t *parent, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D mask NMS over the rows of all query classes of a scene (assemble.py; the loop the
 * reference left unreachable at tools/refinement_single.py:62-91, with a stable sort).
 *
 * K non-empty bit rows with a score each.  Rank: score descending, ties by ascending input index; order[r] = the input
 * index of rank r (int32 [K], a permutation, made by the caller).  For ranks r < s with i = order[r], j = order[s],
 * I = |row i & row j| and areas a:
 *     BFF_NMS_IOU          v = (float)I / (float)(a_i + a_j - I)
 *     BFF_NMS_CONTAINMENT  v = (float)I / (float)min(a_i, a_j)
 * one float32 division of exactly converted integers (the caller guarantees 0 < a < 2^23), and r HITS s iff !(v < thres)
 * in float32 -- the reference's keep-test `iou < nms_thres`, which torch evaluates in float32 -- and, with cls given,
 * cls[i] == cls[j].  Greedy, in rank order: r is kept iff no kept q < r hits it.
 *
 * Limit: K <= 4096 (bff_resolve_overlaps_max_rows(); the Gram is K^2 int32), else BFF_E_LIMIT before anything is launched
 * or written.  K == 0 returns 0 without a launch.  Neither entry point allocates or synchronises; neither uses atomics. */
#define BFF_NMS_IOU 0
#define BFF_NMS_CONTAINMENT 1

/* inter: int32 [K][K] and area: int32 [K], both in INPUT order (bff_cross_popcount of the rows with themselves,
 * bff_popcount_rows); cls: int32 [K] in input order or NULL; thres: not NaN; a criterion other than the two is BFF_E_ARG.
 * sup: uint64 [K][ceil(K / 64)], written whole: bit s of row r is set iff r < s and r hits s; the bits with s <= r or
 * s >= K are zero.  An entry of order outside [0, K) hits nothing and is hit by nothing. */
int bff_nms_pairs(const int32_t *inter, const int32_t *area, const int32_t *order, const int32_t *cls, int32_t k,
                  int32_t criterion, float thres, uint64_t *sup, void *stream);

/* sup as bff_nms_pairs writes it (bits with s <= r zero).  keep_bits: uint64 [ceil(K / 64)], bit r = rank r is kept, the
 * bits >= K zero; by: int32 [K] by rank, the smallest kept rank that hits r, -1 for a kept r; n_kept: int32 [1].  One
 * wave walks the ranks (lane l holds word l of the removed set; the rows of sup are loaded ahead of the decisions), a
 * second launch finds `by` for 64 ranks per wave. */
int bff_nms_greedy(const uint64_t *sup, int32_t k, uint64_t *keep_bits, int32_t *by, int32_t *n_kept, void *stream);

/* ------------------------------------------------------------------------------------------
 * The best views of 3-D instances and the boxes to crop them with, read off the visibility table (views.py; DESIGN.md
 * section 7l; the reference has no such step).
 *
 * K instance bit rows in the SORTED point order (uint64 [K][nw], nw = ceil(n_points / 64), padding bits zero; rows may
 * overlap and may be empty) against the table of F slots (vis_mask, vis_off, vis_pix as bff_visibility_table writes them,
 * stride = bff_visibility_words(n_points) >= nw, n_pixels = the length of vis_pix).  S(k, f) = the points whose bit is
 * set in row k and in vis_mask[f]:
 *     visible int32 [K][F]      |S(k, f)|                               (= bff_cross_popcount of the rows and vis_mask)
 *     box     int32 [K][F][4]   (min u, min v, max u, max v) over the pixels of S(k, f), inclusive; (width, height, -1, -1)
 *                               where S is empty
 * Top views: the candidates of k are the slots with visible >= max(1, min_points), ordered by visible descending, ties by
 * ascending slot position:
 *     top         int32 [K][top_k]             the t-th candidate's slot position, -1 past the candidates
 *     top_visible int32 [K][top_k]             its count, 0 past the candidates
 *     crops       int32 [K][top_k][levels][4]  for level l and the view's box (u0, v0, u1, v1):
 *                     ex = (int)floor((double)(u1 - u0) * expand) * l,  ey = (int)floor((double)(v1 - v0) * expand) * l
 *                     (max(0, u0 - ex), max(0, v0 - ey), min(width - 1, u1 + ex), min(height - 1, v1 + ey));
 *                 (width, height, -1, -1) past the candidates.  One float64 product of exactly converted integers, the same
 *                 on host and device (-ffp-contract=off); it is cut at 2^15 before the conversion -- beyond every image
 *                 side, so the crop is the same and no expand overflows.
 * Everything else is integer; there are no atomics; every element of every output is written exactly once (no pre-fill).
 *
 * Limits, checked before anything is launched: n_slots <= 65535; height, width < 2^15; K * F * 4 < 2^31; 1 <= top_k <= 64;
 * 1 <= levels <= 8 -- else BFF_E_LIMIT; expand finite and >= 0, else BFF_E_ARG.  K == 0 or F == 0 returns 0 without a
 * launch (nothing is written).  box and crops must be 16-byte aligned.  Neither entry point allocates or synchronises. */

/* rows are read for w < nw only; vis_pix is never read at or beyond n_pixels (a pair there counts but moves no box).
 * One workgroup per (instance, 16 slots): the row's non-zero words are compacted into LDS once (up to
 * bff_instance_views_lds_words() of them; a fuller row is walked in global memory), one wave per slot walks them. */
int bff_instance_views(const uint64_t *rows, int32_t n_rows, int64_t nw, const uint64_t *vis_mask, const uint32_t *vis_off,
                       const uint32_t *vis_pix, int32_t n_slots, int64_t stride, int64_t n_pixels, int32_t height,
                       int32_t width, int32_t *visible, int32_t *box, void *stream);
int32_t bff_instance_views_lds_words(void);

/* visible, box: as bff_instance_views writes them.  One wave per instance: top_k rounds of an arg-max over the slots on the
 * key (count, -position), each below the key of the round before; the crops are written by the same kernel. */
int bff_select_views(const int32_t *visible, const int32_t *box, int32_t n_rows, int32_t n_slots, int32_t height,
                     int32_t width, int32_t top_k, int32_t min_points, int32_t levels, double expand, int32_t *top,
                     int32_t *top_visible, int32_t *crops, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BFF_HIP_H */
