"""Mesh depth clipped at a near plane, the parts that need no GPU: the NumPy statement of bff_render_mesh_depth_clip_u16
(tests/mesh_clip_ref.py) against the analytic depth of a box room seen from inside, against the unclipped frames of the
generated scene, and on triangles worked by hand; the config key; the header and the binding table."""
import functools
import os
import re

import numpy as np
import pytest

import mesh_clip_ref as mc
import mesh_depth_ref as md

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4).reshape(1, 16)


# ------------------------------------------------------------------ the box room against the analytic ray / box depth
@functools.lru_cache(maxsize=None)
def room_frames(stride, zn):
    """zn None: today's rule (mesh_depth_ref).  Computed once, shared, never written to."""
    vertices, faces, inv = mc.box_room()
    size = md.rendered_size(mc.ROOM_H, mc.ROOM_W, stride)
    frames = md.render_mesh_ref(vertices, faces, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, *size) if zn is None else \
        mc.render_clip_ref(vertices, faces, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, *size, zn)
    frames.setflags(write=False)
    return frames


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("camera", range(len(mc.ROOM_CAMERAS)))
def test_box_room_equals_the_analytic_depth(camera, stride):
    """A closed room seen from inside has depth in every texel.  z is correct to far below a micrometre, so the rounded
    millimetres can differ from the analytic value only at a tie: the bound is 1 (observed: 0).  At zn = 0.25 the walls
    nearer than zn are cut away: texels within 1 mm of zn are left out, nearer ones hold nothing."""
    size = md.rendered_size(mc.ROOM_H, mc.ROOM_W, stride)
    z = mc.room_depth(camera, *size)
    exp = np.rint(1000.0 * z)
    got = room_frames(stride, 0.05)[camera].astype(np.float64)
    assert z.min() > 0.051 and (got != 0).all()
    print(f"camera {camera} stride {stride} zn 0.05: largest difference {np.abs(got - exp).max()} mm")
    assert (np.abs(got - exp) <= 1).all()
    zn = 0.25
    got = room_frames(stride, zn)[camera].astype(np.float64)
    beyond, nearer = z >= zn + 1e-3, z < zn - 1e-3
    print(f"camera {camera} stride {stride} zn {zn}: {int(beyond.sum())} texels beyond, {int(nearer.sum())} nearer, "
          f"{int((~beyond & ~nearer).sum())} left out, largest difference {np.abs(got - exp)[beyond].max(initial=0)} mm")
    assert (~beyond & ~nearer).sum() <= 48
    assert (np.abs(got - exp)[beyond] <= 1).all() and (got[nearer] == 0).all()


@pytest.mark.parametrize("stride", [1, 4])
def test_box_room_is_what_the_feature_is_for(stride):
    """Today's rule drops the walls that reach behind the camera: on the four cameras that stand off centre at least half
    of the texels hold nothing (at stride 1: 2330, 3071, 2602 and 3072 of 3072)."""
    dropped = room_frames(stride, None)
    zeros = [int((f == 0).sum()) for f in dropped]
    print(f"stride {stride}: zero texels per camera {zeros} of {dropped[0].size}")
    assert all(2 * z >= dropped[0].size for z in zeros[:mc.ROOM_OFF_CENTRE])
    if stride == 1:
        assert zeros[:mc.ROOM_OFF_CENTRE] == [2330, 3071, 2602, 3072]
    for zn in (0.05, 0.25):                                              # a wall that is not clipped keeps its bytes
        clipped = room_frames(stride, zn)
        keep = (dropped != 0) & (clipped != 0)
        assert np.array_equal(clipped[keep], dropped[keep])


# ------------------------------------------------------------------ the generated scene
@pytest.mark.parametrize("stride,zeros", [(2, 5718), (4, 1425)])
def test_tiny_scene_has_depth_everywhere(stride, zeros):
    import render_depth_ref as rd
    from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh
    scene = rd.without_depth(make_scene("tiny", seed=74))
    vertices, faces = make_scene_mesh(seed=74)
    inv = np.stack([np.linalg.inv(np.asarray(scene.poses[f], np.float64)) for f in scene.poses])
    k33 = np.asarray(scene.cam_intr, np.float64)[:3, :3]
    h, w = scene.height, scene.width
    size = md.rendered_size(h, w, stride)
    assert faces.shape[0] == 112 and inv.shape[0] == 6 and (h, w) == (120, 160)
    dropped = md.render_mesh_ref(vertices, faces, inv, k33, h, w, *size)
    clipped = mc.render_clip_ref(vertices, faces, inv, k33, h, w, *size, 0.05)
    assert int((dropped == 0).sum()) == zeros
    assert (clipped != 0).all()
    assert np.array_equal(clipped[dropped != 0], dropped[dropped != 0])


# ------------------------------------------------------------------ hand cases
def hand_frame(vertices, faces, fans=None):
    return mc.render_clip_ref(vertices, faces, EYE, mc.HAND_K, mc.HAND_H, mc.HAND_W, mc.HAND_H, mc.HAND_W, mc.HAND_ZN, fans)[0]


def rays():
    return mc.texel_rays(mc.HAND_K, mc.HAND_H, mc.HAND_W, mc.HAND_H, mc.HAND_W)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", [n for n in mc.HAND if n != "nan vertex"])
def test_hand_triangle_against_its_rays(name, flip):
    """One triangle at the identity pose against rays cast in camera coordinates: a texel whose ray meets the triangle
    beyond zn holds that depth (to 1 mm: a tie of the rounding), one whose ray misses it or meets it nearer holds 0."""
    vertices, faces = mc.hand_triangle(name, flip)
    fans = []
    got = hand_frame(vertices, faces, fans)
    z, w = mc.ray_triangle(vertices, rays())
    inside, outside = (w > 1e-9) & (z > mc.HAND_ZN + 1e-6), ~(w >= -1e-9) | ~(z >= mc.HAND_ZN - 1e-6)
    assert (~inside & ~outside).sum() <= 16                              # texels on an edge or on the cut: either way
    assert (got[inside] != 0).all() and (got[outside] == 0).all()
    assert (np.abs(got[inside].astype(np.float64) - np.rint(1000.0 * z[inside])) <= 1).all()
    assert inside.any() == (name in mc.HAND_DRAWS)
    n_fan = {"one inside": 1, "two inside": 2, "on plane, one in, one out": 2, "on plane, others inside": 1,
             "on plane, others outside": 1, "all nearer": 0, "all behind": 0, "wholly beyond": 1, "shared edge a": 2,
             "shared edge b": 2}[name]
    assert len(fans[0]["faces"]) == n_fan


@pytest.mark.parametrize("flip", [False, True])
def test_hand_special_cases(flip):
    # a vertex with c2 == zn exactly: t = 0, the cut point is the vertex itself, and that fan triangle draws nothing
    vertices, faces = mc.hand_triangle("on plane, one in, one out", flip)
    fans = []
    got = hand_frame(vertices, faces, fans)
    fan = fans[0]
    assert mc.camera_points(vertices, EYE, mc.HAND_K)[0, 2] == mc.HAND_ZN
    onplane = [c for c in fan["cuts"] if c[1] == 0]
    assert len(onplane) == 1 and (onplane[0][3], onplane[0][4]) == (fan["px"][0], fan["py"][0])
    boxes = [mc.box_texels(fan, t, mc.HAND_H, mc.HAND_W, mc.HAND_H, mc.HAND_W) for t in range(2)]
    assert sorted(boxes)[0] == 0 and sorted(boxes)[1] > 0 and got.any()
    # ... and with the two others nearer than zn all three polygon vertices are that vertex
    assert not hand_frame(*mc.hand_triangle("on plane, others outside", flip)).any()
    # nearer than zn, behind the camera, a NaN vertex: nothing
    for name in ("all nearer", "all behind", "nan vertex"):
        fans = []
        assert not hand_frame(*mc.hand_triangle(name, flip), fans).any() and len(fans[0]["faces"]) == 0
    # wholly at or beyond zn: today's arithmetic, today's bytes
    for name in ("wholly beyond", "on plane, others inside"):
        vertices, faces = mc.hand_triangle(name, flip)
        old = md.render_mesh_ref(vertices, faces, EYE, mc.HAND_K, mc.HAND_H, mc.HAND_W, mc.HAND_H, mc.HAND_W)[0]
        assert old.any() and np.array_equal(hand_frame(vertices, faces), old)
    # today's rule drops the straddlers
    for name in ("one inside", "two inside"):
        vertices, faces = mc.hand_triangle(name, flip)
        assert not md.render_mesh_ref(vertices, faces, EYE, mc.HAND_K, mc.HAND_H, mc.HAND_W, mc.HAND_H, mc.HAND_W).any()


@pytest.mark.parametrize("flip", [False, True])
def test_shared_straddling_edge_has_no_crack(flip):
    """Two triangles over one edge that crosses the near plane, walked in opposite directions: the cut point is computed
    from the inside vertex both times, so it is the same bits, and no texel inside the union stays empty."""
    va, _ = mc.hand_triangle("shared edge a")
    vb, _ = mc.hand_triangle("shared edge b")
    vertices = np.concatenate([va, vb[2:]])                              # a0 = b1 (inside), a1 = b0 (outside)
    assert np.array_equal(va[0], vb[1]) and np.array_equal(va[1], vb[0])
    faces = np.array([[0, 1, 2], [1, 0, 3]])
    if flip:
        faces = faces[:, [0, 2, 1]]
    fans = []
    got = hand_frame(vertices, faces, fans)
    shared = [c for c in fans[0]["cuts"] if (c[1], c[2]) == (0, 1)]
    assert len(shared) == 2 and shared[0][0] != shared[1][0]
    assert shared[0][3].hex() == shared[1][3].hex() and shared[0][4].hex() == shared[1][4].hex()
    r = rays()
    za, wa = mc.ray_triangle(va, r)
    zb, wb = mc.ray_triangle(vb, r)
    # inside the union: inside one of the two, the shared edge included (the other triangle's rim), beyond zn
    union = ((wa >= -1e-12) & (za > mc.HAND_ZN + 1e-6)) | ((wb >= -1e-12) & (zb > mc.HAND_ZN + 1e-6))
    on_edge = ((np.abs(wa) <= 1e-12) | (np.abs(wb) <= 1e-12)) & union
    print(f"{int(union.sum())} texels inside the union, {int(on_edge.sum())} of them within 1e-12 of an edge")
    assert union.sum() > 1000 and (got[union] != 0).all()


def test_hand_mesh_holds_every_case():
    vertices, faces = mc.hand_mesh()
    assert faces.shape == (2 * len(mc.HAND), 3)
    names = list(mc.HAND)
    a, b = faces[names.index("shared edge a")], faces[names.index("shared edge b")]
    assert (a[0], a[1]) == (b[1], b[0])
    for k, name in enumerate(names):
        assert np.array_equal(vertices[faces[k]], np.array(mc.HAND[name]), equal_nan=True)
        assert np.array_equal(faces[k + len(names)], faces[k][[0, 2, 1]])
    fans = []
    got = hand_frame(vertices, faces, fans)
    parts = [hand_frame(*mc.hand_triangle(n, flip)) for n in names for flip in (False, True)]
    lowest = np.where(np.stack(parts) == 0, 65536, np.stack(parts).astype(np.int64)).min(axis=0)
    assert np.array_equal(got, np.where(lowest == 65536, 0, lowest).astype(np.uint16))   # a minimum over the triangles


# ------------------------------------------------------------------ config key
def test_config_key():
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    from beyond_fixed_forms_amd.scene import mesh_near_clip
    assert DEFAULTS["mesh_near_clip"] == 0.0 and isinstance(DEFAULTS["mesh_near_clip"], float)
    assert mesh_near_clip(Config()) == 0.0 and mesh_near_clip(Config.with_defaults()) == 0.0
    assert mesh_near_clip(Config(mesh_near_clip=None)) == 0.0 and mesh_near_clip(Config(mesh_near_clip=0)) == 0.0
    assert mesh_near_clip(Config.with_defaults(depth_from_mesh=2)) == 0.0
    assert mesh_near_clip(Config.with_defaults(depth_from_cloud=8, mesh_near_clip=0.0)) == 0.0
    for v in (0.05, np.float64(0.25), np.float32(0.5), 1, np.int64(2), 65.53):
        got = mesh_near_clip(Config.with_defaults(depth_from_mesh=4, mesh_near_clip=v))
        assert isinstance(got, float) and got == float(v)
    for bad in (True, False, "0.05", [0.05], float("nan"), -0.05, -1, 65.535, 70, float("inf")):
        with pytest.raises(ValueError, match="mesh_near_clip"):
            mesh_near_clip(Config.with_defaults(depth_from_mesh=4, mesh_near_clip=bad))
    for cfg in (Config(mesh_near_clip=0.05), Config.with_defaults(mesh_near_clip=0.05),
                Config.with_defaults(depth_from_cloud=8, mesh_near_clip=0.05)):
        with pytest.raises(ValueError, match="depth_from_mesh"):
            mesh_near_clip(cfg)


def test_key_without_the_mesh_key_raises_before_any_upload():
    """prepare_scene and prepare_geometry on a device that would take the upload: the error comes first, as for the
    two-keys error."""
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.scene import prepare_geometry, prepare_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=74)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height, mesh_near_clip=0.05)
    with pytest.raises(ValueError, match="depth_from_mesh"):
        prepare_scene(scene, cfg, device="cpu")
    with pytest.raises(ValueError, match="depth_from_mesh"):
        prepare_geometry(scene, cfg, [scene.mask_2d], device="cpu")
    with pytest.raises(ValueError, match="both"):
        prepare_scene(scene, Config.with_defaults(width_2d=scene.width, height_2d=scene.height, depth_from_mesh=2,
                                                  depth_from_cloud=8, mesh_near_clip=0.05), device="cpu")


# ------------------------------------------------------------------ header and binding
def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 13
    m = re.search(r"int bff_render_mesh_depth_clip_u16\(([^;]*)\);", header)
    assert m, "bff_render_mesh_depth_clip_u16 is not declared"
    kinds, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        kinds.append(_lib._P if "*" in arg else {"int64_t": _lib._L, "int32_t": _lib._I, "double": _lib._D,
                                                 "float": _lib._F}[arg.split()[0]])
    assert kinds == _lib.SIGNATURES["bff_render_mesh_depth_clip_u16"] and len(kinds) == 17
    old = list(_lib.SIGNATURES["bff_render_mesh_depth_u16"])
    at = names.index("near_clip")
    assert names[at + 1] == "frames_per_block" and kinds[:at] + kinds[at + 1:] == old and kinds[at] is _lib._D
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION
    fn = lib.bff_render_mesh_depth_clip_u16                             # argument checks run on the host, before any launch
    N = None
    # (vertices, n_vertices, nv_pad, faces, n_faces, inv_pose, K, n_frames, H, W, dh, dw, near_clip, frames_per_block, ...)
    assert fn(N, 0, 0, N, 0, N, N, 0, 50, 70, 7, 9, 0.05, 0, N, N, N) == 0      # no frames: nothing to do
    for bad in (0.0, -0.05, 65.535, 70.0, float("nan"), float("inf"), -float("inf")):
        assert fn(N, 0, 0, N, 0, N, N, 0, 50, 70, 7, 9, bad, 0, N, N, N) == -1 and b"near_clip" in lib.bff_last_error()
    assert fn(N, 0, 0, N, 0, N, N, 0, 50, 70, 7, 9, 65.53, 0, N, N, N) == 0
    # the old entry point's checks, limits and early returns
    assert fn(N, -1, 0, N, 0, N, N, 0, 1, 1, 1, 1, 0.05, 0, N, N, N) == -1
    assert fn(N, 5, 4, N, 0, N, N, 0, 1, 1, 1, 1, 0.05, 0, N, N, N) == -1
    assert fn(N, 0, 0, N, 0, N, N, 0, 50, 70, 0, 5, 0.05, 0, N, N, N) == -1
    assert fn(N, 0, 0, N, 0, N, N, 0, 50, 70, 7, 9, 0.05, -1, N, N, N) == -1
    assert fn(N, 0, 0, N, 0, N, N, 0, 65536, 65536, 4, 4, 0.05, 0, N, N, N) == -2
    assert fn(N, 0, 0, N, 0, N, N, 70000, 4, 4, 4, 4, 0.05, 0, N, N, N) == -2
    assert fn(N, 0, 0, N, 1 << 31, N, N, 0, 4, 4, 4, 4, 0.05, 0, N, N, N) == -2 and b"triangles" in lib.bff_last_error()
    assert fn(N, 5, 1024, N, 2, N, N, 1, 50, 70, 7, 9, 0.05, 0, N, N, N) == -1 and b"null pointer" in lib.bff_last_error()
    assert b"bff_render_mesh_depth_clip_u16" in lib.bff_last_error()
    old_fn = lib.bff_render_mesh_depth_u16
    assert old_fn(N, 5, 1024, N, 2, N, N, 1, 50, 70, 7, 9, 0, N, N, N) == -1
    assert b"bff_render_mesh_depth_u16: null pointer" in lib.bff_last_error()
