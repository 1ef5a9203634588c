// Frames rendered from the geometry itself (include/bff_hip.h), for scenes that come without sensor depth and for putting
// 3-D instances back into the views:
//   bff_render_depth_u16, bff_render_splat_depth_u16   a point z-buffer over the cloud, one texel or a footprint per point
//   bff_render_labels_u16                              the same z-buffer with the point's label next to its depth
//   bff_render_mesh_depth_u16, ..._clip_u16            a triangle mesh rasterised, dropped or clipped at a near plane
// Every point (vertex) is projected into every frame with the sweep's geometry (geom.h); what takes part offers a key to
// texels of the (depth_h, depth_w) frame, and a texel keeps the minimum.
//
// Data layout in HBM
//   xyz      f64 [3][n_pad]                    the sorted cloud of the sweep (a wave reads 3 x 512 B contiguous)
//   lab      u16 [n_points]                    labels only: the label of every point, in the cloud's order (128 B per wave)
//   faces    i32 [n_faces][3]                  mesh only: launched sorted by their smallest vertex (a wave's gathers are neighbours)
//   scratch  u32 [n_frames][depth_h * depth_w] all ones = empty; key = millimetres, or millimetres << 16 | label; unsigned min
//                                              by returnless vector atomics (executed at the L2 / memory side: no
//                                              read-modify-write traffic in the CUs).  Every call fills it itself.
//   out      u16 [n_frames][depth_h][depth_w]  millimetres, 0 = no depth: what bff_depth_tile_u16, bff_depth_from_u16 and
//                                              bff_project_views_u16 (layout 0) take; labels: the key's two halves, two frames
// A minimum of integers does not depend on the order of its operands: the frames are the same bytes on every run.
#include "geom.h"

namespace bff {

constexpr int kRdBlock = 256;
constexpr int kRdPPT = 4;                                          // points per thread
constexpr int kRdWordsPerBlock = (kRdBlock / kWave) * kRdPPT;      // 16 x 64 points
constexpr int kRdPtsPerBlock = kRdWordsPerBlock * kWave;           // 1024
constexpr int kRdCullGroup = 8;                                    // frames one culling pass decides; the largest frame tile
constexpr uint32_t kRdEmpty = 0xffffffffu;
constexpr int kRsLaneBox = 64;                                     // footprint texels a lane walks alone; beyond: the wave path

struct TexelBox { int j0, i0, bw, count; };                        // first column, first row, width, texels (0 = empty)

// Texels whose sample point can lie inside [lo, hi] along one axis (sample of texel t: (t + 0.5) * s - 0.5), one texel
// wider at either end and clipped to [0, n): -> first, last (first > last = none).  |lo|, |hi| < 2^24 and s >= 2^-31, so
// the quotients stay below 2^56 and their rounding error far below the texel added at either end.
__device__ __forceinline__ void texel_range(double lo, double hi, double s, int n, int &first, int &last)
{
    const double a = fmax(floor((lo + 0.5) / s - 0.5) - 1.0, 0.0);
    const double b = fmin(ceil((hi + 0.5) / s - 0.5) + 1.0, (double)(n - 1));
    first = 0, last = -1;
    if (a <= b) first = (int)a, last = (int)b;                      // 0 <= a <= b <= n - 1: the conversions are exact
}

// Texels t of one axis with fabs(X_t - c) <= R, X_t = (t + 0.5) * s - 0.5 (the header's comparison, operation by
// operation), clipped to [0, n): -> first, last (first > last = none).  X_t ascends with t and so does the rounded
// difference, so the texels that pass are a run; texel_range gives a run that holds it (one texel wider at either end
// than [c - R, c + R] reaches: far more than the roundings here move), and both ends come in until they pass.
__device__ __forceinline__ void splat_range(double c, double R, double s, int n, int &first, int &last)
{
    texel_range(__dsub_rn(c, R), __dadd_rn(c, R), s, n, first, last);
    auto passes = [&](int t) { return fabs(__dsub_rn(__dsub_rn(__dmul_rn((double)t + 0.5, s), 0.5), c)) <= R; };
    while (first <= last && !passes(first)) ++first;
    while (last >= first && !passes(last)) --last;
}

// The texel rectangle [i0, i1] x [j0, j1] as a box; empty where either range is
__device__ __forceinline__ TexelBox texel_box(int j0, int j1, int i0, int i1)
{
    TexelBox b = {j0, i0, 0, 0};
    if (j1 >= j0 && i1 >= i0) {
        b.bw = j1 - j0 + 1;
        b.count = b.bw * (i1 - i0 + 1);                            // <= dh * dw < 2^31
    }
    return b;
}

// A footprint rectangle: key goes to every texel of b, no test left inside it.  A rectangle of at most kRsLaneBox texels
// is walked by its lane; a larger one (a point near the camera can cover the frame) by the whole wave: ballot, broadcast of
// the key and the rectangle, 64 lanes stride over it.  Every lane of the wave comes here (count = 0: nothing to offer).
__device__ __forceinline__ void offer_box(const TexelBox &b, uint32_t key, int lane, int dw, uint32_t *__restrict__ img)
{
    if (b.count > 0 && b.count <= kRsLaneBox)                      // the lane's own walk, row by row
        for (int k = 0, i = b.i0, t = b.j0; k < b.count; ++k) {
            atomicMin(img + (i * dw + t), key);                    // result unused: returnless
            if (++t == b.j0 + b.bw) t = b.j0, ++i;
        }
    uint64_t big = __ballot(b.count > kRsLaneBox);
    while (big) {
        const int src = __ffsll((unsigned long long)big) - 1;
        big &= big - 1;
        const uint32_t wkey = __shfl(key, src);
        const int wj0 = __shfl(b.j0, src), wi0 = __shfl(b.i0, src), wbw = __shfl(b.bw, src), wcount = __shfl(b.count, src);
        for (unsigned k = lane; k < (unsigned)wcount; k += kWave)   // unsigned: wcount + 63 may pass 2^31
            atomicMin(img + ((wi0 + (int)(k / (unsigned)wbw)) * dw + wj0 + (int)(k % (unsigned)wbw)), wkey);
    }
}

// The point z-buffer.  viewed_count_kernel's shape (visibility.hip): 256 threads own 1024 consecutive points, 4 per thread in
// registers across the frames of the block's frame tile (blockIdx.y), poses wave-uniform, the tile culled against
// tile_bounds in groups of 8 frames.  Per frame and point: the key to the point's own texel; kSplat: also to the texels
// whose sample point lies within (Rx, Ry) pixels of the point's integer pixel, a rectangle found per axis (splat_range).
// kLabels: key = millimetres << 16 | label, else millimetres.
template <bool kSplat, bool kLabels>
__global__ __launch_bounds__(kRdBlock) void point_zbuffer_kernel(
    const double *__restrict__ xyz, int64_t n_points, int64_t n_pad, const uint16_t *__restrict__ lab,
    const double *__restrict__ inv_pose, CameraK K, int n_frames, int frames_per_block, int H, int W, int dh, int dw,
    double radius, uint32_t *__restrict__ scratch, const double *__restrict__ tile_bounds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t word0 = (int64_t)blockIdx.x * kRdWordsPerBlock + (int64_t)wave * kRdPPT;     // the wave's first 64 points
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    const int64_t plane = (int64_t)dh * dw;
    const double dW = (double)W, dH = (double)H;
    const double sx = dW / (double)dw, sy = dH / (double)dh;
    const double krx = __dmul_rn(K.k[0], radius), kry = __dmul_rn(K.k[4], radius);

    double px[kRdPPT], py[kRdPPT], pz[kRdPPT];
    uint32_t pl[kRdPPT];
    bool valid[kRdPPT];
#pragma unroll
    for (int j = 0; j < kRdPPT; ++j) {
        const int64_t n = (word0 + j) * kWave + lane;
        valid[j] = n < n_points;                                   // padding lanes take no part (they read point 0)
        const int64_t m = valid[j] ? n : 0;
        px[j] = xyz[m];
        py[j] = xyz[n_pad + m];
        pz[j] = xyz[2 * n_pad + m];
        pl[j] = kLabels ? lab[m] : 0;                              // lab has n_points entries: m < n_points
    }

    for (int g0 = f0; g0 < f1; g0 += kRdCullGroup) {
        const int g1 = min(f1, g0 + kRdCullGroup);
        uint64_t culled = 0;
        if (tile_bounds && word0 * kWave < n_points)               // wave-uniform; only in-bounds points take part, so
            culled = cull_frames(tile_bounds + 6 * (word0 / kRdPPT), inv_pose, K, g0, g1, lane, dW, dH);   // culling stays exact
        for (int f = g0; f < g1; ++f) {
            if ((culled >> (8 * (f - g0))) & 1) continue;          // wave-uniform
            const double *P = inv_pose + 16 * (int64_t)f;
            uint32_t *img = scratch + (int64_t)f * plane;
#pragma unroll
            for (int j = 0; j < kRdPPT; ++j) {
                double cz, u, v;
                camera_pixel(P, K, px[j], py[j], pz[j], cz, u, v);
                // millimetres, half to even; a surface the camera sees lies in front of it (NaN fails cz > 0)
                const double m = rint(__dmul_rn(cz, 1000.0));
                const bool splat = valid[j] && pixel_in_bounds(u, v, dW, dH) && (cz > 0.0) && (m >= 1.0) && (m <= 65535.0);
                const uint32_t key = !splat ? kRdEmpty : kLabels ? (((uint32_t)m << 16) | pl[j]) : (uint32_t)m;
                // own texel: u < W and v < H, so tx < dw and ty < dh; W * dw and H * dh < 2^31 (checked by the entry point)
                if (splat)
                    atomicMin(img + ((int)(((unsigned)(int)v * (unsigned)dh) / (unsigned)H) * dw +
                                     (int)(((unsigned)(int)u * (unsigned)dw) / (unsigned)W)), key);   // result unused: returnless
                if constexpr (kSplat) {
                    TexelBox b = {0, 0, 0, 0};
                    if (splat) {
                        int j0, j1, i0, i1;
                        splat_range(u, krx / cz, sx, dw, j0, j1);
                        splat_range(v, kry / cz, sy, dh, i0, i1);
                        b = texel_box(j0, j1, i0, i1);
                    }
                    offer_box(b, key, lane, dw, img);              // every lane of the wave: no early exit above
                }
            }
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

// scratch -> the two uint16 frames of a labelled call: low half = label, high half = millimetres, all ones (nothing
// offered) = 0 in both
__global__ __launch_bounds__(256) void render_labels_narrow_kernel(const uint32_t *__restrict__ scratch, int64_t total,
                                                                    uint16_t *__restrict__ labels, uint16_t *__restrict__ depth)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint32_t s = scratch[i];
    const bool empty = s == kRdEmpty;
    labels[i] = empty ? 0 : (uint16_t)(s & 0xffffu);
    if (depth) depth[i] = empty ? 0 : (uint16_t)(s >> 16);
}

// ---------------------------------------------------------------------------------------------------------------------
// Depth frames rendered from a triangle mesh.  One thread owns one triangle: its nine vertex doubles stay in registers
// across the frames of the block's frame tile (blockIdx.y, poses wave-uniform).  Per frame the three vertices are
// transformed (camera_point) and the screen triangle -- kClip: the one or two triangles of the polygon the near plane
// leaves -- goes through raster_tri: its texel box clipped to the frame, the box's texels tested with the header's edge
// functions, one returnless atomicMin per covered texel.  scratch, out and the narrowing kernel are the point renderer's.
constexpr int kRmBlock = 256;
constexpr int kRmLaneBox = 64;                                     // texels a lane walks alone; beyond: the wave path
constexpr double kRmPixelLimit = 16777216.0;                       // 2^24: |px|, |py| of a triangle that takes part

struct WorldTri { double ax, ay, az, bx, by, bz, cx, cy, cz; bool valid; };    // valid = false: draws nothing
struct CamVtx { double c0, c1, c2, px, py; };                      // a vertex in camera coordinates and on the screen
struct ScreenTri { double x0, y0, r0, x1, y1, r1, x2, y2, r2; };   // pixel position and 1 / depth of the three vertices

// Triangle tri of the launch.  The caller has validated the indices; a triangle that names a vertex outside the array is
// still never read (it, and a thread past the last triangle, load vertex 0 and are not valid)
__device__ __forceinline__ WorldTri load_tri(const double *__restrict__ vtx, int64_t n_vertices, int64_t nv_pad,
                                             const int32_t *__restrict__ faces, int64_t n_faces, int64_t tri)
{
    WorldTri w;
    w.valid = tri < n_faces;
    int64_t v0 = 0, v1 = 0, v2 = 0;
    if (w.valid) {
        v0 = faces[3 * tri], v1 = faces[3 * tri + 1], v2 = faces[3 * tri + 2];
        w.valid = v0 >= 0 && v0 < n_vertices && v1 >= 0 && v1 < n_vertices && v2 >= 0 && v2 < n_vertices;
        if (!w.valid) v0 = v1 = v2 = 0;
    }
    w.ax = vtx[v0], w.ay = vtx[nv_pad + v0], w.az = vtx[2 * nv_pad + v0];
    w.bx = vtx[v1], w.by = vtx[nv_pad + v1], w.bz = vtx[2 * nv_pad + v1];
    w.cx = vtx[v2], w.cy = vtx[nv_pad + v2], w.cz = vtx[2 * nv_pad + v2];
    return w;
}

// World point -> camera coordinates c and screen position in pixels (pixel centres at integers).  c: camera_pixel's fma
// chains, so c2 is the depth the visibility test compares; px, py: plain products and sums in the header's order.
__device__ __forceinline__ CamVtx camera_point(const double *__restrict__ P, const CameraK &K, double x, double y, double z)
{
    CamVtx v;
    v.c0 = fma(P[3], 1.0, fma(P[2], z, fma(P[1], y, fma(P[0], x, 0.0))));
    v.c1 = fma(P[7], 1.0, fma(P[6], z, fma(P[5], y, fma(P[4], x, 0.0))));
    v.c2 = fma(P[11], 1.0, fma(P[10], z, fma(P[9], y, fma(P[8], x, 0.0))));
    v.px = __dadd_rn(__dadd_rn(__dmul_rn(K.k[0], v.c0), __dmul_rn(K.k[1], v.c1)), __dmul_rn(K.k[2], v.c2)) / v.c2;
    v.py = __dadd_rn(__dadd_rn(__dmul_rn(K.k[3], v.c0), __dmul_rn(K.k[4], v.c1)), __dmul_rn(K.k[5], v.c2)) / v.c2;
    return v;
}

__device__ __forceinline__ bool in_pixel_range(const ScreenTri &t)   // on the doubles: NaN fails
{
    return fabs(t.x0) < kRmPixelLimit && fabs(t.x1) < kRmPixelLimit && fabs(t.x2) < kRmPixelLimit &&
           fabs(t.y0) < kRmPixelLimit && fabs(t.y1) < kRmPixelLimit && fabs(t.y2) < kRmPixelLimit;
}

// One texel against one triangle: the header's coverage test and depth; splats when covered and in range
__device__ __forceinline__ void mesh_texel(const ScreenTri &t, int i, int j, double sx, double sy, int dw,
                                           uint32_t *__restrict__ img)
{
    const double X = __dsub_rn(__dmul_rn((double)j + 0.5, sx), 0.5), Y = __dsub_rn(__dmul_rn((double)i + 0.5, sy), 0.5);
    const double ax = t.x0 - X, ay = t.y0 - Y, bx = t.x1 - X, by = t.y1 - Y, cx = t.x2 - X, cy = t.y2 - Y;
    const double e0 = __dsub_rn(__dmul_rn(bx, cy), __dmul_rn(cx, by));
    const double e1 = __dsub_rn(__dmul_rn(cx, ay), __dmul_rn(ax, cy));
    const double e2 = __dsub_rn(__dmul_rn(ax, by), __dmul_rn(bx, ay));
    const double S = __dadd_rn(__dadd_rn(e0, e1), e2);
    const bool covered = (S != 0.0) && ((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0));
    if (!covered) return;
    const double z = S / __dadd_rn(__dadd_rn(__dmul_rn(e0, t.r0), __dmul_rn(e1, t.r1)), __dmul_rn(e2, t.r2));
    const double m = rint(__dmul_rn(z, 1000.0));
    if (m >= 1.0 && m <= 65535.0) atomicMin(img + (i * dw + j), (uint32_t)m);          // result unused: returnless
}

// The box, lane walk and wave walk of one screen triangle per lane.  A box of at most kRmLaneBox texels is walked by the
// lane that owns the triangle; a larger one (a triangle near the camera can cover a frame) by the whole wave: ballot,
// broadcast of the triangle, 64 lanes stride over the box.  Every lane of the wave comes here (takes = false: it has
// nothing to draw): the wave walk needs them all at its ballot.
__device__ __forceinline__ void raster_tri(const ScreenTri &t, bool takes, int lane, double sx, double sy, int H, int W,
                                           int dh, int dw, uint32_t *__restrict__ img)
{
    TexelBox b = {0, 0, 0, 0};
    // two vertices at one position: e0 + e1 + e2 is exactly 0 at every texel (one e is x * y - x * y, the other two
    // are each other's negatives), so nothing is covered
    const bool flat = (t.x0 == t.x1 && t.y0 == t.y1) || (t.x1 == t.x2 && t.y1 == t.y2) || (t.x0 == t.x2 && t.y0 == t.y2);
    if (takes && !flat) {
        const double xlo = fmin(t.x0, fmin(t.x1, t.x2)), xhi = fmax(t.x0, fmax(t.x1, t.x2));
        const double ylo = fmin(t.y0, fmin(t.y1, t.y2)), yhi = fmax(t.y0, fmax(t.y1, t.y2));
        int j0, j1, i0, i1;
        texel_range(xlo, xhi, sx, dw, j0, j1);
        texel_range(ylo, yhi, sy, dh, i0, i1);
        // The box must hold every texel the header's arithmetic covers.  A texel outside it lies more than a texel
        // beyond the vertices along x (or y): x_k - X has one sign for all k, the sample point is outside the
        // triangle, and the negative edge functions add up to at least |A| * sx / ex (A: twice the area, ex >= |x_k -
        // X|).  Rounding can lift an edge function to >= 0 only from above -2^-52 ex ey, so the texel can pass as
        // covered only where |A| <= 2^-51 ex ey (ex / sx); with the rounding of A itself, 2^-49 ex ey max(ex / sx, ey /
        // sy) bounds it.  Such a sliver (three distinct vertices on a line) takes the whole frame as its box.
        const double ex = fmax(fabs(xlo), fabs(xhi)) + (double)W, ey = fmax(fabs(ylo), fabs(yhi)) + (double)H;
        const double A = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.x2 - t.x0) * (t.y1 - t.y0);
        if (!(fabs(A) > 0x1p-49 * ex * ey * fmax(ex / sx, ey / sy)))
            j0 = 0, j1 = dw - 1, i0 = 0, i1 = dh - 1;
        b = texel_box(j0, j1, i0, i1);
    }
    if (b.count > 0 && b.count <= kRmLaneBox)                      // the lane's own walk, row by row
        for (int k = 0, i = b.i0, j = b.j0; k < b.count; ++k) {
            mesh_texel(t, i, j, sx, sy, dw, img);
            if (++j == b.j0 + b.bw) j = b.j0, ++i;
        }
    uint64_t big = __ballot(b.count > kRmLaneBox);
    while (big) {
        const int src = __ffsll((unsigned long long)big) - 1;
        big &= big - 1;
        ScreenTri w;
        w.x0 = __shfl(t.x0, src), w.y0 = __shfl(t.y0, src), w.r0 = __shfl(t.r0, src);
        w.x1 = __shfl(t.x1, src), w.y1 = __shfl(t.y1, src), w.r1 = __shfl(t.r1, src);
        w.x2 = __shfl(t.x2, src), w.y2 = __shfl(t.y2, src), w.r2 = __shfl(t.r2, src);
        const int wj0 = __shfl(b.j0, src), wi0 = __shfl(b.i0, src), wbw = __shfl(b.bw, src), wcount = __shfl(b.count, src);
        for (unsigned k = lane; k < (unsigned)wcount; k += kWave)   // unsigned: wcount + 63 may pass 2^31
            mesh_texel(w, wi0 + (int)(k / (unsigned)wbw), wj0 + (int)(k % (unsigned)wbw), sx, sy, dw, img);
    }
}

// The clipped polygon: up to four screen vertices in named registers (no indexed array: that would live in scratch
// memory).  emit: the next vertex goes into the first free slot; a polygon never has a fifth
struct Polygon {
    double x0, y0, r0, x1, y1, r1, x2, y2, r2, x3, y3, r3;
    int n;
    __device__ __forceinline__ void emit(double x, double y, double r)
    {
        x0 = n == 0 ? x : x0, y0 = n == 0 ? y : y0, r0 = n == 0 ? r : r0;
        x1 = n == 1 ? x : x1, y1 = n == 1 ? y : y1, r1 = n == 1 ? r : r1;
        x2 = n == 2 ? x : x2, y2 = n == 2 ? y : y2, r2 = n == 2 ? r : r2;
        x3 = n == 3 ? x : x3, y3 = n == 3 ? y : y3, r3 = n == 3 ? r : r3;
        ++n;
    }
};

// Edge a -> b of the header's polygon walk: a itself when it is inside, and the cut point when the edge crosses the near
// plane, computed from the inside vertex towards the outside one whichever way the edge is walked
__device__ __forceinline__ void clip_edge(const CamVtx &a, bool a_in, const CamVtx &b, bool b_in, const CameraK &K, double zn,
                                          double rn, Polygon &q)
{
    if (a_in) q.emit(a.px, a.py, 1.0 / a.c2);
    if (a_in != b_in) {
        const double p0 = a_in ? a.c0 : b.c0, p1 = a_in ? a.c1 : b.c1, p2 = a_in ? a.c2 : b.c2;
        const double o0 = a_in ? b.c0 : a.c0, o1 = a_in ? b.c1 : a.c1, o2 = a_in ? b.c2 : a.c2;
        const double t = __dsub_rn(p2, zn) / __dsub_rn(p2, o2);
        const double i0 = __dadd_rn(p0, __dmul_rn(t, __dsub_rn(o0, p0)));
        const double i1 = __dadd_rn(p1, __dmul_rn(t, __dsub_rn(o1, p1)));
        const double x = __dadd_rn(__dadd_rn(__dmul_rn(K.k[0], i0), __dmul_rn(K.k[1], i1)), __dmul_rn(K.k[2], zn)) / zn;
        const double y = __dadd_rn(__dadd_rn(__dmul_rn(K.k[3], i0), __dmul_rn(K.k[4], i1)), __dmul_rn(K.k[5], zn)) / zn;
        q.emit(x, y, rn);
    }
}

__device__ __forceinline__ bool finite3(const CamVtx &v) { return isfinite(v.c0) && isfinite(v.c1) && isfinite(v.c2); }

// kClip = false (bff_render_mesh_depth_u16): a triangle that reaches the camera plane is dropped.  kClip = true
// (bff_render_mesh_depth_clip_u16): it is cut at c2 = zn into a polygon of up to four screen vertices, and the fan's one
// or two triangles are drawn; a clipped wall beside the camera usually covers the frame, so the wave walk is the common
// case there.
template <bool kClip>
__global__ __launch_bounds__(kRmBlock) void render_mesh_kernel(
    const double *__restrict__ vtx, int64_t n_vertices, int64_t nv_pad, const int32_t *__restrict__ faces, int64_t n_faces,
    const double *__restrict__ inv_pose, CameraK K, int n_frames, int frames_per_block, int H, int W, int dh, int dw,
    double zn, uint32_t *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63;
    const int f0 = blockIdx.y * frames_per_block;
    const int f1 = min(n_frames, f0 + frames_per_block);
    const int64_t plane = (int64_t)dh * dw;
    const double sx = (double)W / (double)dw, sy = (double)H / (double)dh;
    const WorldTri w = load_tri(vtx, n_vertices, nv_pad, faces, n_faces, (int64_t)blockIdx.x * kRmBlock + threadIdx.x);

    for (int f = f0; f < f1; ++f) {                                // wave-uniform
        const double *P = inv_pose + 16 * (int64_t)f;
        uint32_t *img = scratch + (int64_t)f * plane;
        const CamVtx a = camera_point(P, K, w.ax, w.ay, w.az), b = camera_point(P, K, w.bx, w.by, w.bz),
                     c = camera_point(P, K, w.cx, w.cy, w.cz);
        if constexpr (!kClip) {
            const ScreenTri t = {a.px, a.py, 1.0 / a.c2, b.px, b.py, 1.0 / b.c2, c.px, c.py, 1.0 / c.c2};
            // comparisons on the doubles: NaN fails; a triangle that crosses the camera plane is dropped, not clipped
            const bool takes = w.valid && a.c2 > 0.0 && b.c2 > 0.0 && c.c2 > 0.0 && in_pixel_range(t);
            raster_tri(t, takes, lane, sx, sy, H, W, dh, dw, img);
        } else {
            const bool part = w.valid && finite3(a) && finite3(b) && finite3(c);
            const bool a_in = part && a.c2 >= zn, b_in = part && b.c2 >= zn, c_in = part && c.c2 >= zn;
            const double rn = 1.0 / zn;
            Polygon q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0};      // 0, 3 or 4 vertices, in the
            clip_edge(a, a_in, b, b_in, K, zn, rn, q);                                        // header's emission order
            clip_edge(b, b_in, c, c_in, K, zn, rn, q);
            clip_edge(c, c_in, a, a_in, K, zn, rn, q);
            // the fan (q0, q1, q2), (q0, q2, q3); the second pass only where a lane of the wave has a quadrilateral
            for (int pass = 0; pass < 2; ++pass) {                 // wave-uniform: every lane reaches raster_tri's ballot
                if (pass == 1 && !__any(q.n == 4)) break;
                const ScreenTri t = {q.x0, q.y0, q.r0, pass ? q.x2 : q.x1, pass ? q.y2 : q.y1, pass ? q.r2 : q.r1,
                                     pass ? q.x3 : q.x2, pass ? q.y3 : q.y2, pass ? q.r3 : q.r2};
                const bool takes = (pass ? q.n == 4 : q.n >= 3) && in_pixel_range(t);
                raster_tri(t, takes, lane, sx, sy, H, W, dh, dw, img);
            }
        }
    }
}

}  // namespace bff

using namespace bff;

// blocks of a narrowing kernel: 256 threads of per_thread texels
static int64_t narrow_blocks(int64_t total, int per_thread) { return ceil_div(ceil_div(total, per_thread), 256); }

// the scratch of a depth call -> its uint16 frames
static int narrow_frames(const uint32_t *scratch_u32, int64_t total, uint16_t *out_u16, hipStream_t st, const char *what)
{
    const int vec_ok = (reinterpret_cast<uintptr_t>(scratch_u32) % 16 == 0) && (reinterpret_cast<uintptr_t>(out_u16) % 8 == 0);
    render_depth_narrow_kernel<<<(unsigned)narrow_blocks(total, 4), 256, 0, st>>>(scratch_u32, total, vec_ok, out_u16);
    return launched(what);
}

// What a render call launches with, once render_setup has let it through
struct RenderSetup {
    bool launch;                                                     // false: the call has returned what it returns
    hipStream_t st;
    int64_t total;                                                   // texels of the call
    CameraK K;
    int frames_per_block;
};

// The part every render entry point shares, in the order their callers rely on: the caller's size check, the image and
// frame limits, the caller's own checks (`own_checks`, a callable that returns BFF_OK or has failed), the early returns --
// no frames: nothing; nothing to draw: the outputs zeroed -- the null-pointer check, the all-ones fill of the scratch, the
// copy of K and the frame tile (0 = chosen here: >= ~4096 blocks in flight over gx blocks per tile, tiles of up to 8 frames).
template <typename Checks>
static int render_setup(const char *what, bool sizes_ok, int32_t n_frames, int32_t height, int32_t width, int32_t depth_h,
                        int32_t depth_w, Checks own_checks, bool nothing_to_draw, bool inputs_ok, const double *cam_intr_host,
                        int64_t gx, int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *out_u16, uint16_t *out2_u16,
                        void *stream, RenderSetup &s)
{
    s.launch = false;
    BFF_REQUIRE(sizes_ok && n_frames >= 0 && frames_per_block >= 0, "%s: bad sizes", what);
    BFF_REQUIRE(height > 0 && width > 0 && depth_h > 0 && depth_w > 0, "%s: bad image size", what);
    BFF_LIMIT((int64_t)height * width < (1ll << 31), "%s: image larger than 2^31 pixels", what);
    BFF_LIMIT((int64_t)depth_h * depth_w < (1ll << 31), "%s: depth frame larger than 2^31 texels", what);
    BFF_LIMIT((int64_t)height * depth_h < (1ll << 31) && (int64_t)width * depth_w < (1ll << 31),
              "%s: pixel x texel products beyond 2^31 (height * depth_h, width * depth_w)", what);
    BFF_LIMIT(n_frames <= 65535, "%s: too many frames", what);
    s.total = (int64_t)n_frames * depth_h * depth_w;
    int rc = own_checks();
    if (rc != BFF_OK || n_frames == 0) return rc;
    BFF_REQUIRE(out_u16, "%s: null pointer", what);
    s.st = as_stream(stream);
    if (nothing_to_draw) {                                           // every texel is "no depth" (and background)
        hipError_t e = hipMemsetAsync(out_u16, 0, sizeof(uint16_t) * (size_t)s.total, s.st);
        if (e == hipSuccess && out2_u16) e = hipMemsetAsync(out2_u16, 0, sizeof(uint16_t) * (size_t)s.total, s.st);
        if (e != hipSuccess) return fail((int)e, "%s: memset: %s", what, hipGetErrorString(e));
        return BFF_OK;
    }
    BFF_REQUIRE(inputs_ok && cam_intr_host && scratch_u32, "%s: null pointer", what);
    hipError_t e = hipMemsetAsync(scratch_u32, 0xff, sizeof(uint32_t) * (size_t)s.total, s.st);
    if (e != hipSuccess) return fail((int)e, "%s: memset: %s", what, hipGetErrorString(e));
    for (int i = 0; i < 9; ++i) s.K.k[i] = cam_intr_host[i];
    s.frames_per_block = frames_per_block;
    if (frames_per_block == 0) {
        const int64_t fpb = (int64_t)n_frames * gx / 4096;
        s.frames_per_block = fpb < 1 ? 1 : (fpb > kRdCullGroup ? kRdCullGroup : (int)fpb);
    }
    s.launch = true;
    return BFF_OK;
}

// The three point entry points: the checks, one of the four z-buffer kernels, one of the two narrowing kernels.  labels:
// out_u16 takes the labels and depth_u16 (optional) the depth; else out_u16 takes the depth
static int render_points(const char *what, bool labels, bool splat, double splat_radius, const double *xyz, int64_t n_points,
                         int64_t n_pad, const uint16_t *lab, const double *inv_pose, const double *cam_intr_host,
                         int32_t n_frames, int32_t height, int32_t width, int32_t depth_h, int32_t depth_w,
                         int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *out_u16, uint16_t *depth_u16,
                         const double *tile_bounds, void *stream)
{
    const int64_t gx = ceil_div(n_points, kRdPtsPerBlock);
    const int64_t n_narrow = narrow_blocks((int64_t)n_frames * depth_h * depth_w, labels ? 1 : 4);
    auto own_checks = [&]() {
        BFF_LIMIT(gx < (1ll << 31) && n_narrow < (1ll << 31), "%s: too many points / texels for one launch", what);
        // the comparisons fail on NaN; checked before the early returns, as the sizes are (K: where the caller gave one)
        if (labels)
            BFF_REQUIRE(splat_radius >= 0.0 && std::isfinite(splat_radius), "%s: splat_radius must be finite and >= 0", what);
        else
            BFF_REQUIRE(!splat || (splat_radius > 0.0 && std::isfinite(splat_radius)), "%s: splat_radius must be finite and > 0", what);
        BFF_REQUIRE(!splat || !cam_intr_host || (cam_intr_host[0] > 0.0 && std::isfinite(cam_intr_host[0]) && cam_intr_host[4] > 0.0 &&
                                                 std::isfinite(cam_intr_host[4])), "%s: K00 and K11 must be finite and > 0", what);
        return (int)BFF_OK;
    };
    RenderSetup s;
    int rc = render_setup(what, n_points >= 0 && n_pad >= n_points, n_frames, height, width, depth_h, depth_w, own_checks,
                          n_points == 0, xyz && inv_pose && (lab || !labels), cam_intr_host, gx, frames_per_block, scratch_u32,
                          out_u16, depth_u16, stream, s);
    if (rc != BFF_OK || !s.launch) return rc;
    // the culling table's tiles are the sweep's (bff_point_tile_bounds): they must be this kernel's waves
    BFF_REQUIRE(!tile_bounds || bff_point_tile_size() == kRdPPT * kWave, "%s: tile_bounds holds tiles of %d points, the "
                "renderer's waves own %d", what, bff_point_tile_size(), kRdPPT * kWave);
    const auto kernel = labels ? (splat ? point_zbuffer_kernel<true, true> : point_zbuffer_kernel<false, true>)
                               : (splat ? point_zbuffer_kernel<true, false> : point_zbuffer_kernel<false, false>);
    dim3 grid((unsigned)gx, (unsigned)ceil_div(n_frames, s.frames_per_block));
    kernel<<<grid, kRdBlock, 0, s.st>>>(xyz, n_points, n_pad, lab, inv_pose, s.K, n_frames, s.frames_per_block, height, width,
                                        depth_h, depth_w, splat ? splat_radius : 0.0, scratch_u32, tile_bounds);
    rc = launched(what);
    if (rc != BFF_OK) return rc;
    if (!labels) return narrow_frames(scratch_u32, s.total, out_u16, s.st, what);
    render_labels_narrow_kernel<<<(unsigned)n_narrow, 256, 0, s.st>>>(scratch_u32, s.total, out_u16, depth_u16);
    return launched(what);
}

extern "C" int bff_render_depth_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                                    const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width,
                                    int32_t depth_h, int32_t depth_w, int32_t frames_per_block, uint32_t *scratch_u32,
                                    uint16_t *out_u16, const double *tile_bounds, void *stream)
{
    return render_points("bff_render_depth_u16", false, false, 0.0, xyz, n_points, n_pad, nullptr, inv_pose, cam_intr_host,
                         n_frames, height, width, depth_h, depth_w, frames_per_block, scratch_u32, out_u16, nullptr, tile_bounds,
                         stream);
}

extern "C" int bff_render_splat_depth_u16(const double *xyz, int64_t n_points, int64_t n_pad, const double *inv_pose,
                                          const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width,
                                          int32_t depth_h, int32_t depth_w, double splat_radius, int32_t frames_per_block,
                                          uint32_t *scratch_u32, uint16_t *out_u16, const double *tile_bounds, void *stream)
{
    return render_points("bff_render_splat_depth_u16", false, true, splat_radius, xyz, n_points, n_pad, nullptr, inv_pose,
                         cam_intr_host, n_frames, height, width, depth_h, depth_w, frames_per_block, scratch_u32, out_u16, nullptr,
                         tile_bounds, stream);
}

extern "C" int bff_render_labels_u16(const double *xyz, int64_t n_points, int64_t n_pad, const uint16_t *lab,
                                     const double *inv_pose, const double *cam_intr_host, int32_t n_frames, int32_t height,
                                     int32_t width, int32_t depth_h, int32_t depth_w, double splat_radius,
                                     int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *labels_u16,
                                     uint16_t *depth_u16, const double *tile_bounds, void *stream)
{
    return render_points("bff_render_labels_u16", true, splat_radius > 0.0, splat_radius, xyz, n_points, n_pad, lab, inv_pose,
                         cam_intr_host, n_frames, height, width, depth_h, depth_w, frames_per_block, scratch_u32, labels_u16,
                         depth_u16, tile_bounds, stream);
}

extern "C" int bff_splat_lane_box(void) { return kRsLaneBox; }

extern "C" int bff_mesh_lane_box(void) { return kRmLaneBox; }

// both mesh entry points: the checks, one of the two kernels, the narrowing
static int render_mesh(const char *what, bool clip, double near_clip, const double *vertices, int64_t n_vertices,
                       int64_t nv_pad, const int32_t *faces, int64_t n_faces, const double *inv_pose,
                       const double *cam_intr_host, int32_t n_frames, int32_t height, int32_t width, int32_t depth_h,
                       int32_t depth_w, int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *out_u16, void *stream)
{
    const int64_t gx = ceil_div(n_faces, kRmBlock);                  // < 2^23
    auto own_checks = [&]() {
        BFF_LIMIT(n_faces < (1ll << 31), "%s: 2^31 triangles or more", what);
        BFF_LIMIT(narrow_blocks((int64_t)n_frames * depth_h * depth_w, 4) < (1ll << 31), "%s: too many texels for one launch", what);
        return (int)BFF_OK;
    };
    RenderSetup s;
    int rc = render_setup(what, n_vertices >= 0 && nv_pad >= n_vertices && n_faces >= 0, n_frames, height, width, depth_h,
                          depth_w, own_checks, n_faces == 0 || n_vertices == 0, vertices && faces && inv_pose, cam_intr_host, gx,
                          frames_per_block, scratch_u32, out_u16, nullptr, stream, s);
    if (rc != BFF_OK || !s.launch) return rc;
    const auto kernel = clip ? render_mesh_kernel<true> : render_mesh_kernel<false>;
    dim3 grid((unsigned)gx, (unsigned)ceil_div(n_frames, s.frames_per_block));
    kernel<<<grid, kRmBlock, 0, s.st>>>(vertices, n_vertices, nv_pad, faces, n_faces, inv_pose, s.K, n_frames, s.frames_per_block,
                                        height, width, depth_h, depth_w, near_clip, scratch_u32);
    rc = launched(what);
    if (rc != BFF_OK) return rc;
    return narrow_frames(scratch_u32, s.total, out_u16, s.st, what);
}

extern "C" int bff_render_mesh_depth_u16(const double *vertices, int64_t n_vertices, int64_t nv_pad, const int32_t *faces,
                                         int64_t n_faces, const double *inv_pose, const double *cam_intr_host,
                                         int32_t n_frames, int32_t height, int32_t width, int32_t depth_h, int32_t depth_w,
                                         int32_t frames_per_block, uint32_t *scratch_u32, uint16_t *out_u16, void *stream)
{
    return render_mesh("bff_render_mesh_depth_u16", false, 0.0, vertices, n_vertices, nv_pad, faces, n_faces, inv_pose,
                       cam_intr_host, n_frames, height, width, depth_h, depth_w, frames_per_block, scratch_u32, out_u16, stream);
}

extern "C" int bff_render_mesh_depth_clip_u16(const double *vertices, int64_t n_vertices, int64_t nv_pad, const int32_t *faces,
                                              int64_t n_faces, const double *inv_pose, const double *cam_intr_host,
                                              int32_t n_frames, int32_t height, int32_t width, int32_t depth_h,
                                              int32_t depth_w, double near_clip, int32_t frames_per_block,
                                              uint32_t *scratch_u32, uint16_t *out_u16, void *stream)
{
    // the comparisons fail on NaN
    BFF_REQUIRE(near_clip > 0.0 && near_clip < 65.535, "bff_render_mesh_depth_clip_u16: near_clip must lie in (0, 65.535) metres");
    return render_mesh("bff_render_mesh_depth_clip_u16", true, near_clip, vertices, n_vertices, nv_pad, faces, n_faces,
                       inv_pose, cam_intr_host, n_frames, height, width, depth_h, depth_w, frames_per_block, scratch_u32,
                       out_u16, stream);
}
