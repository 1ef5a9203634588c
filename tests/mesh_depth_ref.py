"""NumPy statement of bff_render_mesh_depth_u16 (include/bff_hip.h), and of a scene whose depth frames are rasterised
from its triangle mesh.  TEST INFRASTRUCTURE ONLY.

Camera points come from oracle/geom_fma (k-ascending fma chains from +0.0); everything after them is the header's
float64 arithmetic in the order written -- NumPy neither fuses nor reorders it -- evaluated by brute force: every
triangle against every texel, then np.minimum.
"""
import copy

import numpy as np

from oracle import geom_fma

EMPTY = np.uint32(0xFFFFFFFF)
PIXEL_LIMIT = 2.0 ** 24


def screen_vertices(vertices, inv_pose, k33):
    """One frame: (px, py, c2) of every vertex."""
    k = np.asarray(k33, np.float64)
    pts, _, _ = geom_fma.view(np.asarray(vertices, np.float64), np.asarray(inv_pose, np.float64).reshape(4, 4), k,
                              np.zeros((1, 1), np.float32))
    c0, c1, c2 = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        px = ((k[0, 0] * c0 + k[0, 1] * c1) + k[0, 2] * c2) / c2
        py = ((k[1, 0] * c0 + k[1, 1] * c1) + k[1, 2] * c2) / c2
    return px, py, c2


def sample_points(height, width, depth_h, depth_w):
    """-> (X (depth_w,), Y (depth_h,)): the pixel position of every texel's sample point."""
    return (np.arange(depth_w) + 0.5) * (width / depth_w) - 0.5, (np.arange(depth_h) + 0.5) * (height / depth_h) - 0.5


def taking_part(px, py, c2, faces):
    with np.errstate(all="ignore"):
        ok = (c2 > 0) & (np.abs(px) < PIXEL_LIMIT) & (np.abs(py) < PIXEL_LIMIT)
    return ok[faces].all(axis=1)


def render_mesh_frame(px, py, c2, faces, X, Y, chunk=128, covered=None):
    """One frame from its screen vertices: uint16 (len(Y), len(X)).  covered (optional list): receives the number of
    triangles that cover each texel (whatever their depth)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    faces = faces[taking_part(px, py, c2, faces)]
    xx, yy = np.meshgrid(X, Y)
    xx, yy = xx.reshape(1, -1), yy.reshape(1, -1)
    buf = np.full(xx.shape[1], float(EMPTY))
    cnt = np.zeros(xx.shape[1], np.int64)
    with np.errstate(all="ignore"):
        r = 1.0 / c2
        for t0 in range(0, faces.shape[0], chunk):
            f = faces[t0:t0 + chunk]
            col = lambda a, k: a[f[:, k]].reshape(-1, 1)
            ax, ay, bx, by, cx, cy = (col(px, 0) - xx, col(py, 0) - yy, col(px, 1) - xx, col(py, 1) - yy,
                                      col(px, 2) - xx, col(py, 2) - yy)
            e0 = bx * cy - cx * by
            e1 = cx * ay - ax * cy
            e2 = ax * by - bx * ay
            s = (e0 + e1) + e2
            cov = (s != 0) & (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)))
            z = s / ((e0 * col(r, 0) + e1 * col(r, 1)) + e2 * col(r, 2))
            m = np.rint(z * 1000.0)
            take = cov & (m >= 1) & (m <= 65535)
            buf = np.minimum(buf, np.where(take, m, float(EMPTY)).min(axis=0))
            cnt += cov.sum(axis=0)
    if covered is not None:
        covered.append(cnt.reshape(len(Y), len(X)))
    return np.where(buf == float(EMPTY), 0, buf).astype(np.uint16).reshape(len(Y), len(X))


def render_mesh_ref(vertices, faces, inv_poses, k33, height, width, depth_h, depth_w, covered=None):
    """uint16 [F][depth_h][depth_w] millimetres, 0 = no triangle."""
    vertices = np.asarray(vertices, np.float64)[:, :3]
    inv_poses = np.asarray(inv_poses, np.float64).reshape(-1, 16)
    X, Y = sample_points(height, width, depth_h, depth_w)
    out = np.zeros((inv_poses.shape[0], depth_h, depth_w), np.uint16)
    for f, inv in enumerate(inv_poses):
        out[f] = render_mesh_frame(*screen_vertices(vertices, inv, k33), faces, X, Y, covered=covered)
    return out


def rendered_size(height, width, stride):
    return -(-height // stride), -(-width // stride)


def scene_mesh(scene):
    """(vertices, faces) of a scene: its own mesh vertices, or the rows of its cloud."""
    v = scene.mesh_vertices if getattr(scene, "mesh_vertices", None) is not None else scene.points
    return np.asarray(v, np.float64)[:, :3], np.asarray(scene.faces)


def scene_with_rendered_depth(scene, stride):
    """A copy of `scene` whose float32 (H, W) depth images are what the reference would read had the frames rasterised
    from the scene's mesh been its depth PNGs (P:431-436): astype(float32) / 1000, then the bilinear resize."""
    from beyond_fixed_forms_amd.io import resize_bilinear_f32
    h, w = scene.height, scene.width
    dh, dw = rendered_size(h, w, stride)
    ids = list(scene.poses)
    inv = np.stack([np.linalg.inv(np.asarray(scene.poses[f], np.float64)) for f in ids])
    vertices, faces = scene_mesh(scene)
    frames = render_mesh_ref(vertices, faces, inv, np.asarray(scene.cam_intr, np.float64)[:3, :3], h, w, dh, dw)
    out = copy.copy(scene)
    out.depths = {f: resize_bilinear_f32(frames[k].astype(np.float32) / np.float32(1000), w, h) for k, f in enumerate(ids)}
    out.depths_raw = None
    return out


def grid_faces(rows, cols, base=0):
    """Two triangles per cell of a rows x cols vertex grid stored row-major from index `base`."""
    i, j = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    c = (i * cols + j).reshape(-1) + base
    return np.concatenate([np.stack([c, c + cols, c + cols + 1], 1), np.stack([c, c + cols + 1, c + 1], 1)])


def tilted_plane(height=96, width=128, n=90):
    """The issue's plane: through (0, 0, 3), tilted 30 degrees about the camera's x axis, a 90 x 90 vertex grid
    -> (vertices, faces, K, (a, b)) with vertex (i, j) = (b_j, a_i cos 30, 3 + a_i sin 30)."""
    a, b = np.linspace(-3, 5, n), np.linspace(-9, 9, n)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    aa, bb = np.meshgrid(a, b, indexing="ij")
    vertices = np.stack([bb, aa * c, 3 + aa * s], -1).reshape(-1, 3)
    k33 = np.array([[0.9 * width, 0, width / 2 - 0.5], [0, 0.9 * width, height / 2 - 0.5], [0, 0, 1.0]])
    return vertices, grid_faces(n, n), k33, (a, b)


def two_plane_mesh_scene(**kw):
    """render_depth_ref.two_plane_scene with both planes triangulated: the faces index the cloud (one vertex per pixel
    centre on the far plane, then on the near plane's rectangle)."""
    import render_depth_ref as rd
    scene, far_px, n_far = rd.two_plane_scene(**kw)
    near = kw.get("near", (16, 20, 32, 44))
    scene.faces = np.concatenate([grid_faces(scene.height, scene.width),
                                  grid_faces(near[2] - near[0], near[3] - near[1], base=n_far)])
    return scene, far_px, n_far


def write_mesh(root, scene):
    """scene_mesh_dir/<scene_id>.npz of a scene (root / "mesh")."""
    (root / "mesh").mkdir(parents=True, exist_ok=True)
    arrays = dict(faces=np.asarray(scene.faces))
    if getattr(scene, "mesh_vertices", None) is not None:
        arrays["vertices"] = np.asarray(scene.mesh_vertices)
    np.savez(root / "mesh" / f"{scene.scene_id}.npz", **arrays)
