"""The visibility table (bff_visibility_table, include/bff_hip.h) restated in NumPy, and the small case its test runs on.

Host only.  For depth slot s, sorted point word w and lane l the table says whether point 64 w + l passes the sweep's
test in the slot's frame, and at which pixel:

  camera point   c_i = fma(P[i][3], 1, fma(P[i][2], z, fma(P[i][1], y, fma(P[i][0], x, +0.0))))    (k ascending)
  pixel          p_i = fma(K[i][2], c_2, fma(K[i][1], c_1, fma(K[i][0], c_0, +0.0))),  u = rint(p_0 / c_2), v = rint(p_1 / c_2)
  in bounds      0 <= u < W and 0 <= v < H, compared on the doubles (NaN fails; there is no c_2 > 0 test)
  depth          the float32 (H, W) image: the sensor frame as float32 / 1000, resized with io.resize_bilinear_f32's
                 arithmetic (float32 2-tap passes, horizontal then vertical; taps of io._axis_taps), restated below
  visible        in bounds, depth != 0 and |c_2 - (double)depth| < thresh

fma is libm's, element by element: NumPy has none, and a * b + c rounds twice."""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma = np.frompyfunc(_libm.fma, 3, 1)


def fma(a, b, c):
    return _fma(a, b, c).astype(np.float64)


def project(xyz, inv_pose, k33):
    """xyz f64 [n][3], inv_pose f64 [16] or [4][4], k33 f64 [3][3] -> (c_2, u, v) as doubles (u, v may be NaN / inf)."""
    P, K = np.asarray(inv_pose, np.float64).reshape(4, 4), np.asarray(k33, np.float64)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    zero, one = np.zeros_like(x), np.ones_like(x)
    c = [fma(P[i, 3], one, fma(P[i, 2], z, fma(P[i, 1], y, fma(P[i, 0], x, zero)))) for i in range(3)]
    p = [fma(K[i, 2], c[2], fma(K[i, 1], c[1], fma(K[i, 0], c[0], zero))) for i in range(2)]
    with np.errstate(all="ignore"):
        return c[2], np.rint(p[0] / c[2]), np.rint(p[1] / c[2])


def axis_taps(n_dst, n_src, x_axis):
    """(i0, i1, a) of one axis: f = (float32)((d + 0.5) * (1 / (n_dst / n_src)) - 0.5), i0 = floor(f), a = f - i0 in
    float32; x: border columns are copied (a = 0), y: the fraction stays and the two indices are clamped."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i0 = np.floor(f).astype(np.int64)
    a = (f - i0.astype(np.float32)).astype(np.float32)
    if x_axis:
        lo, hi = i0 < 0, i0 >= n_src - 1
        a[lo | hi] = 0.0
        i0 = np.where(lo, 0, np.where(hi, n_src - 1, i0))
        return i0, np.minimum(i0 + 1, n_src - 1), a
    return np.clip(i0, 0, n_src - 1), np.clip(i0 + 1, 0, n_src - 1), a


def resized_depth(raw, height, width):
    """uint16 [hs][ws] millimetres -> float32 [height][width] metres."""
    t = raw.astype(np.float32) / np.float32(1000)
    x0, x1, ax = axis_taps(width, raw.shape[1], True)
    y0, y1, ay = axis_taps(height, raw.shape[0], False)
    one = np.float32(1)
    rows = t[:, x0] * (one - ax) + t[:, x1] * ax
    return rows[y0] * (one - ay)[:, None] + rows[y1] * ay[:, None]


def stride_words(n_points):
    """Words per slot: those of whole 1024-point sweep blocks."""
    return (n_points + 1023) // 1024 * 16


def frame_visibility(xyz, inv_pose, k33, depth, thresh):
    """One frame -> (visible bool [n], u int64 [n], v int64 [n], why dict of bool [n]); depth float32 [H][W]."""
    h, w = depth.shape
    cz, u, v = project(xyz, inv_pose, k33)
    inb = (u >= 0.0) & (u < float(w)) & (v >= 0.0) & (v < float(h))
    ui, vi = np.where(inb, u, 0).astype(np.int64), np.where(inb, v, 0).astype(np.int64)
    d = depth[vi, ui]
    with np.errstate(all="ignore"):
        near = np.abs(cz - d.astype(np.float64)) < thresh
    vis = inb & (d != 0) & near
    return vis, ui, vi, dict(in_bounds=inb, zero_depth=inb & (d == 0), behind=inb & (cz < 0))


def table(xyz, poses, k33, depths, thresh):
    """xyz f64 [n][3], poses f64 [S][16], depths float32 [S][H][W] -> (vis_mask uint64 [S][stride], vis_off uint32
    [S][stride], vis_pix uint32 [pairs])."""
    n, n_slots = xyz.shape[0], len(poses)
    stride = stride_words(n)
    bits = np.zeros((n_slots, stride * 64), bool)
    pix = []
    for s in range(n_slots):
        vis, u, v, _why = frame_visibility(xyz, poses[s], k33, depths[s], thresh)
        bits[s, :n] = vis
        pix.append((u[vis] | (v[vis] << 16)).astype(np.uint32))          # ascending point order = (word, lane) order
    mask = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n_slots, stride)
    counts = bits.reshape(n_slots, stride, 64).sum(axis=2).reshape(-1)
    off = (np.cumsum(counts) - counts).astype(np.uint32).reshape(n_slots, stride)
    return mask, off, np.concatenate(pix) if pix else np.zeros(0, np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# The case: 1500 points (two sweep blocks, neither 64 nor 1024 divides it), six depth slots of 24 x 32 pixels over
# 12 x 16-texel sensor frames.
N_POINTS = 1500
H, W, HS, WS = 24, 32, 12, 16
K = np.array([[20.0, 0.0, 15.5], [0.0, 20.0, 11.5], [0.0, 0.0, 1.0]])
THRESH = 0.08
N_SLOTS = 6
PLANE_Z = 2.0
ZERO_TEXELS = (slice(4, 8), slice(4, 9))          # sensor texels of slot 0 without a reading
SLOT_NO_DEPTH, SLOT_AWAY = 3, 4                   # frames that see nothing: no reading at all / every point out of bounds


def _pose(yaw=0.0, pos=(0.0, 0.0, 0.0)):
    """World -> camera for a camera at `pos` turned by `yaw` about its y axis."""
    c, s = np.cos(yaw), np.sin(yaw)
    pose = np.eye(4)
    pose[:3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    pose[:3, 3] = pos
    return np.linalg.inv(pose).reshape(16)


def _sensor_frame(xyz, inv_pose):
    """uint16 [HS][WS]: per texel the smallest rint(1000 c_2) of the in-bounds points in front of the camera."""
    cz, u, v = project(xyz, inv_pose, K)
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (cz > 0)
    tex = (v[ok].astype(np.int64) * HS // H) * WS + u[ok].astype(np.int64) * WS // W
    mm = np.minimum(np.rint(cz[ok] * 1000.0), 65535).astype(np.int64)
    order = np.argsort(-mm, kind="stable")
    out = np.zeros(HS * WS, np.int64)
    out[tex[order]] = mm[order]
    return out.astype(np.uint16).reshape(HS, WS)


def build_case(seed=7):
    """-> dict(xyz f64 [N][3], poses f64 [S][16], raw uint16 [S][HS][WS], depth float32 [S][H][W])."""
    rng = np.random.default_rng(seed)
    # a plane at z = PLANE_Z with one point at the centre of every pixel of slot 0's image (borders included) and a rim of
    # points just outside it; a box of points around it; points behind camera 0; NaN points
    uu, vv = np.meshgrid(np.arange(-2, W + 2), np.arange(-2, H + 2))
    grid = np.stack([(uu.ravel() - K[0, 2]) / K[0, 0] * PLANE_Z, (vv.ravel() - K[1, 2]) / K[1, 1] * PLANE_Z,
                     np.full(uu.size, PLANE_Z)], axis=1)
    n_box = N_POINTS - grid.shape[0] - 100 - 5
    box = rng.uniform([-2.0, -1.5, 0.5], [2.0, 1.5, 4.0], (n_box, 3))
    behind = rng.uniform([-1.0, -1.0, -3.0], [1.0, 1.0, -0.01], (100, 3))
    xyz = np.concatenate([grid, box, behind, np.full((5, 3), np.nan)])
    xyz[-3, 1:] = 0.5                              # NaN in one coordinate only
    xyz = xyz[rng.permutation(N_POINTS)]
    assert xyz.shape == (N_POINTS, 3)
    poses = np.stack([_pose(), _pose(0.0, (0.3, -0.2, -0.5)), _pose(0.35, (-0.4, 0.1, 0.2)), _pose(-0.2, (0.2, 0.0, 0.1)),
                      _pose(0.0, (1000.0, 0.0, 0.0)), _pose(0.1, (0.0, 0.3, -1.0))])
    raw = np.stack([_sensor_frame(xyz, p) for p in poses])
    raw[0] = int(PLANE_Z * 1000)
    raw[0][ZERO_TEXELS] = 0
    raw[SLOT_NO_DEPTH] = 0
    raw[SLOT_AWAY] = 1500                          # a reading everywhere: only the bounds keep this frame empty
    depth = np.stack([resized_depth(r, H, W) for r in raw])
    return dict(xyz=xyz, poses=poses, raw=raw, depth=depth)
