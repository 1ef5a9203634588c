// Per-point camera geometry as device functions: the arithmetic contract of bff_project_views (include/bff_hip.h) and the
// exact frustum test of a point tile, stated once for the sweep kernels (project.hip, visibility.hip, diag.hip) and the
// renderers (render_depth.hip, render_labels.hip).
#pragma once

#include "common.h"

namespace bff {

struct CameraK { double k[9]; };          // row-major intrinsics, passed as a kernel argument

inline CameraK camera_k(const double *cam_intr_host)    // from the caller's nine doubles; null: zeros (no geometry is run)
{
    CameraK K{};
    for (int i = 0; i < 9 && cam_intr_host; ++i) K.k[i] = cam_intr_host[i];
    return K;
}

// World point -> camera z and rounded pixel.  c_i: k-ascending fma chain of inv_pose row i with (x, y, z, 1) from +0.0;
// p_i: fma chain of K row i with c; u = rint(p_0 / c_2), v = rint(p_1 / c_2) (IEEE division, half to even).  P: the
// frame's 16 doubles, wave-uniform.
__host__ __device__ __forceinline__ void camera_pixel(const double *__restrict__ P, const CameraK &K, double x, double y, double z,
                                             double &cz, double &u, double &v)
{
    const double cx = fma(P[3], 1.0, fma(P[2], z, fma(P[1], y, fma(P[0], x, 0.0))));
    const double cy = fma(P[7], 1.0, fma(P[6], z, fma(P[5], y, fma(P[4], x, 0.0))));
    cz = fma(P[11], 1.0, fma(P[10], z, fma(P[9], y, fma(P[8], x, 0.0))));
    const double p0 = fma(K.k[2], cz, fma(K.k[1], cy, fma(K.k[0], cx, 0.0)));
    const double p1 = fma(K.k[5], cz, fma(K.k[4], cy, fma(K.k[3], cx, 0.0)));
    u = rint(p0 / cz);
    v = rint(p1 / cz);
}

// 0 <= u < W and 0 <= v < H on the doubles: NaN, inf and values beyond any integer range fail
__host__ __device__ __forceinline__ bool pixel_in_bounds(double u, double v, double dW, double dH)
{
    return (u >= 0.0) && (u < dW) && (v >= 0.0) && (v < dH);
}

// Frustum culling of one wave's point tile against the <= 8 frames [g0, g1), all at once: lane = 8 * frame + corner of the
// tile's box bb = (xmin, ymin, zmin, xmax, ymax, zmax).  Bit 8 k of the result: frame g0 + k cannot hold an in-bounds pixel
// of any point inside the box.  A point can only be visible if its pixel is in bounds, i.e. (exact arithmetic) it lies in
// the double cone  {L_i >= 0 for all i, c_z > 0}  u  {L_i <= 0 for all i, c_z < 0}  with
//   L_1 = p_0 + (1/2 + m) c_z,  L_2 = (W - 1/2 + m) c_z - p_0,  L_3 = p_1 + (1/2 + m) c_z,  L_4 = (H - 1/2 + m) c_z - p_1
// (the two image borders in u and in v, widened by m = 0.01 pixel; the reference has no z > 0 test, hence both cones).
// Each L_i is an affine function of the world point, so its value anywhere in the box is a convex combination of the 8
// corner values: if some L_i < -delta at every corner the box misses the front cone, if some L_j > +delta at every corner
// it misses the back cone; a frame is skipped only when both hold.  delta = 1e-6 and m exceed the float64 rounding of these
// forms (~1e-11) by orders of magnitude; NaN / inf corner values compare false and keep the frame.  Exact: a skipped frame
// has no in-bounds point in this wave.  Must be called by all 64 lanes.
__device__ __forceinline__ uint64_t cull_frames(const double *__restrict__ bb, const double *__restrict__ inv_pose,
                                                const CameraK &K, int g0, int g1, int lane, double dW, double dH)
{
    const int corner = lane & 7, fk = lane >> 3;
    const double bx = (corner & 1) ? bb[3] : bb[0], by = (corner & 2) ? bb[4] : bb[1], bz = (corner & 4) ? bb[5] : bb[2];
    double l1 = 0.0, l2 = 0.0, l3 = 0.0, l4 = 0.0;
    if (g0 + fk < g1) {
        const double *P = inv_pose + 16 * (int64_t)(g0 + fk);
        const double cx = fma(P[2], bz, fma(P[1], by, P[0] * bx)) + P[3];
        const double cy = fma(P[6], bz, fma(P[5], by, P[4] * bx)) + P[7];
        const double cz = fma(P[10], bz, fma(P[9], by, P[8] * bx)) + P[11];
        const double p0 = fma(K.k[2], cz, fma(K.k[1], cy, K.k[0] * cx));
        const double p1 = fma(K.k[5], cz, fma(K.k[4], cy, K.k[3] * cx));
        constexpr double m = 0.01;
        l1 = fma(0.5 + m, cz, p0);
        l2 = fma(dW - 0.5 + m, cz, -p0);
        l3 = fma(0.5 + m, cz, p1);
        l4 = fma(dH - 0.5 + m, cz, -p1);
    }
    constexpr double delta = 1e-6;
    auto all8 = [](uint64_t b) {                           // bit 8 k of the result = all 8 bits of byte k set
        b &= b >> 1; b &= b >> 2; b &= b >> 4;
        return b & 0x0101010101010101ull;
    };
    const uint64_t neg = all8(__ballot(l1 < -delta)) | all8(__ballot(l2 < -delta)) |
                         all8(__ballot(l3 < -delta)) | all8(__ballot(l4 < -delta));
    const uint64_t pos = all8(__ballot(l1 > delta)) | all8(__ballot(l2 > delta)) |
                         all8(__ballot(l3 > delta)) | all8(__ballot(l4 > delta));
    return neg & pos;
}

}  // namespace bff
