"""Depth rendered from the cloud with a surfel footprint per point, the parts that need no GPU: the NumPy statement of
bff_render_splat_depth_u16 pinned on a case worked by hand, the visibility table that motivates it, the config key, the
loaders on a scene directory without depth/, and the binding table."""
import functools
import os
import re

import numpy as np
import pytest

import mesh_depth_ref as md
import render_depth_ref as rd
import splat_depth_ref as sd
from oracle import geom_fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4).reshape(1, 16)


@functools.lru_cache(maxsize=None)
def two_planes():
    scene, _, _ = rd.two_plane_scene()
    k33 = scene.cam_intr[:3, :3]
    plain = rd.render_depth_ref(scene.points, EYE, k33, 48, 64, 48, 64)[0]
    plain.setflags(write=False)
    return scene.points, k33, plain


def test_reference_two_planes_by_hand():
    """fx = fy = 64, stride 1 (sample point of texel (i, j) = pixel (j, i)), a near plane z = 1 over the pixels v 16..31,
    u 20..43 in front of a far plane z = 3 that fills the 48 x 64 image, one point per pixel centre.  A near point has
    Rx = Ry = 64 r, a far one 64 r / 3.
    r = 0.015625: Rx = 1.0 exactly on the near plane (1/3 on the far one: own texel only) -- the near rectangle grows by
                  one pixel on every side, 18 x 26 - 16 x 24 = 84 texels change from 3000 to 1000;
    r = 0.0156:   Rx = 0.9984 < 1: every point reaches its own sample point only -- the plain frame;
    r = 0.03:     Rx = 1.92 (0.64 on the far plane): the same frame as with 0.015625."""
    xyz, k33, plain = two_planes()
    exp = np.full((48, 64), 3000, np.uint16)
    exp[16:32, 20:44] = 1000
    assert np.array_equal(plain, exp)
    exp[15:33, 19:45] = 1000
    assert 64 * 0.015625 == 1.0
    boxes = []
    got = sd.render_splat_ref(xyz, EYE, k33, 48, 64, 48, 64, 0.015625, boxes)[0]
    assert got.dtype == np.uint16 and np.array_equal(got, exp) and int((got != plain).sum()) == 84
    assert (boxes[0][:48 * 64] == 1).all() and (boxes[0][48 * 64:] == 9).all()     # far: own sample point; near: 3 x 3
    assert np.array_equal(sd.render_splat_ref(xyz, EYE, k33, 48, 64, 48, 64, 0.0156)[0], plain)
    assert np.array_equal(sd.render_splat_ref(xyz, EYE, k33, 48, 64, 48, 64, 0.03)[0], exp)


def plane_visibility(n, radius, stride):
    """test_mesh_depth_host.test_visibility_table's measurement for the tilted plane with n x n vertices as a cloud
    -> (counted, seen through the plain point frame, seen through the splat frame, the splat frame)."""
    from beyond_fixed_forms_amd.io import resize_bilinear_f32
    h, w = 96, 128
    vertices, _, k33, _ = md.tilted_plane(n=n)
    px, py, _ = md.screen_vertices(vertices, EYE, k33)
    u, v = np.rint(px), np.rint(py)
    counted = (u >= stride) & (u < w - stride) & (v >= stride) & (v < h - stride)
    dh, dw = md.rendered_size(h, w, stride)
    frames = (rd.render_depth_ref(vertices, EYE, k33, h, w, dh, dw)[0],
              sd.render_splat_ref(vertices, EYE, k33, h, w, dh, dw, radius)[0])
    seen = []
    for frame in frames:
        depth = resize_bilinear_f32(frame.astype(np.float32) / np.float32(1000), w, h)
        seen.append(int((geom_fma.view(vertices, np.eye(4), k33, depth, 0.08)[2] & counted).sum()))
    return int(counted.sum()), seen[0], seen[1], frames[1]


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_visibility_table(stride):
    """The tilted plane as a cloud through the reference's visibility test (P:51-70) after the bilinear resize of the
    frames; counted as in test_mesh_depth_host.test_visibility_table.  A cloud of 180 x 180 points with r = 0.06 m (about
    the spacing of its points: 0.045 x 0.10 m): the splat frames see every counted vertex at every stride, where the plain
    z-buffer sees 10 of 2236 at stride 2.  Counts with this statement -- stride: counted, plain, splat, empty texels --
    1: 2314, 2314, 2314, 40;  2: 2236, 10, 2236, 4;  4: 2058, 2004, 2058, 0;  8: 1690, 1690, 1690, 0.
    The empty texels: at strides 2 to 8 all in the frame's first or last column (a surface within a radius of the border
    gets no help from points outside the image); at stride 1 20 of the 40 lie on the frame's edge, 2 beside its upper
    corners, and 18 inside, in rows 76 to 83, where the plane is nearest and its points project farther apart than their
    footprints reach -- no counted vertex looks one of them up.
    The shipped plane (90 x 90 points, spacing 0.09 x 0.20 m) with r = 0.1 m: splat 564 / 556 / 492 / 406 where the plain
    frames see 564 / 0 / 6 / 406."""
    n, plain, splat, frame = plane_visibility(180, 0.06, stride)
    empty = np.argwhere(frame == 0)
    print(f"n 180, r 0.06, stride {stride}: counted {n}, plain {plain}, splat {splat}, empty texels {len(empty)}")
    assert n > 0 and splat == n
    assert (n, plain, len(empty)) == {1: (2314, 2314, 40), 2: (2236, 10, 4), 4: (2058, 2004, 0), 8: (1690, 1690, 0)}[stride]
    at_border = np.isin(empty[:, 1], (0, frame.shape[1] - 1)) | np.isin(empty[:, 0], (0, frame.shape[0] - 1))
    inner = empty[~at_border]
    assert at_border.all() if stride > 1 else (len(inner) == 20 and ((inner[:, 0] >= 76) | (inner[:, 0] == 1)).all())
    n, plain, splat, _ = plane_visibility(90, 0.1, stride)
    print(f"n 90, r 0.1, stride {stride}: counted {n}, plain {plain}, splat {splat}")
    assert (n, plain, splat) == {1: (564, 564, 564), 2: (556, 0, 556), 4: (506, 6, 492), 8: (422, 406, 406)}[stride]


def test_too_large_a_radius_costs_visibility():
    """Flat squares bias the minimum towards the camera on a tilted surface: the shipped plane with r = 0.15 m (its
    points are 0.09 m apart along the tilt) at stride 1 loses more than half of the 564 counted vertices that r = 0.1
    and the plain frame both see.  This statement sees 244 (228 at r = 0.151, 166 at r = 0.16: the count falls steeply
    here; the issue's draft reported 212 at 0.15)."""
    n, plain, splat, _ = plane_visibility(90, 0.15, 1)
    print(f"n 90, r 0.15, stride 1: counted {n}, plain {plain}, splat {splat}")
    assert (n, plain) == (564, 564) and splat < n / 2
    assert splat == 244


def test_splat_frame_is_never_larger_than_the_plain_frame():
    vertices, _, k33, _ = md.tilted_plane()
    for stride in (1, 4):
        dh, dw = md.rendered_size(96, 128, stride)
        plain = rd.render_depth_ref(vertices, EYE, k33, 96, 128, dh, dw)[0]
        splat = sd.render_splat_ref(vertices, EYE, k33, 96, 128, dh, dw, 0.1)[0]
        assert ((splat[plain != 0] != 0) & (splat[plain != 0] <= plain[plain != 0])).all() and (splat != plain).any()


# ------------------------------------------------------------------ config key
def test_config_key():
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    from beyond_fixed_forms_amd.scene import cloud_splat_radius, rendered_depth_stride
    assert DEFAULTS["cloud_splat_radius"] == 0.0 and isinstance(DEFAULTS["cloud_splat_radius"], float)
    assert cloud_splat_radius(Config()) == 0.0 and cloud_splat_radius(Config.with_defaults()) == 0.0
    assert cloud_splat_radius(Config(cloud_splat_radius=None)) == 0.0 and cloud_splat_radius(Config(cloud_splat_radius=0)) == 0.0
    assert cloud_splat_radius(Config.with_defaults(depth_from_cloud=2)) == 0.0
    assert cloud_splat_radius(Config.with_defaults(depth_from_mesh=8, cloud_splat_radius=0.0)) == 0.0
    for v in (0.02, np.float64(0.25), np.float32(0.5), 1, np.int64(2), 1e6):
        got = cloud_splat_radius(Config.with_defaults(depth_from_cloud=4, cloud_splat_radius=v))
        assert isinstance(got, float) and got == float(v)
    for bad in (True, False, "0.02", [0.02], float("nan"), -0.02, -1, float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="cloud_splat_radius"):
            cloud_splat_radius(Config.with_defaults(depth_from_cloud=4, cloud_splat_radius=bad))
    for cfg in (Config(cloud_splat_radius=0.02), Config.with_defaults(cloud_splat_radius=0.02),
                Config.with_defaults(depth_from_mesh=8, cloud_splat_radius=0.02)):
        with pytest.raises(ValueError, match="depth_from_cloud"):
            cloud_splat_radius(cfg)
    # both depth keys together with the radius: the radius itself is in order, the two keys are the error
    both = Config.with_defaults(depth_from_mesh=4, depth_from_cloud=8, cloud_splat_radius=0.02)
    assert cloud_splat_radius(both) == 0.02
    with pytest.raises(ValueError, match="both"):
        rendered_depth_stride(both)


def test_key_without_the_cloud_key_raises_before_any_upload():
    """prepare_scene and prepare_geometry on a device that would take the upload: the error comes first, as for the
    two-keys error."""
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.scene import prepare_geometry, prepare_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=74)
    size = dict(width_2d=scene.width, height_2d=scene.height)
    for cfg in (Config.with_defaults(cloud_splat_radius=0.02, **size),
                Config.with_defaults(depth_from_mesh=2, cloud_splat_radius=0.02, **size)):
        with pytest.raises(ValueError, match="depth_from_cloud"):
            prepare_scene(scene, cfg, device="cpu")
        with pytest.raises(ValueError, match="depth_from_cloud"):
            prepare_geometry(scene, cfg, [scene.mask_2d], device="cpu")
    with pytest.raises(ValueError, match="cloud_splat_radius"):
        prepare_scene(scene, Config.with_defaults(depth_from_cloud=8, cloud_splat_radius=-1.0, **size), device="cpu")
    with pytest.raises(ValueError, match="both"):
        prepare_scene(scene, Config.with_defaults(depth_from_mesh=2, depth_from_cloud=8, cloud_splat_radius=0.02, **size),
                      device="cpu")


def test_loaders_still_read_nothing_under_depth(tmp_path):
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.io import load_scene, load_scene_classes
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=3, n_points=500)
    rd.write_scene_without_depth(tmp_path, scene, {"table": scene.mask_2d, "chair": scene.mask_2d[:2]})
    assert not (tmp_path / "2d" / scene.scene_id / "depth").exists()
    on = Config.with_defaults(depth_from_cloud=4, cloud_splat_radius=0.03, width_2d=scene.width, height_2d=scene.height,
                              scene_2d_dir=str(tmp_path / "2d"), scene_npy_dir=str(tmp_path / "npy"),
                              mask_2d_dir=str(tmp_path / "m2d"))
    from beyond_fixed_forms_amd.scene import cloud_splat_radius
    assert cloud_splat_radius(on) == 0.03
    for on_device in (False, True):
        got = load_scene(on, "table", scene.scene_id, depth_on_device=on_device)
        both = load_scene_classes(on, ["table", "chair"], scene.scene_id, depth_on_device=on_device)
        for s in (got, both.scene):
            assert s.depths == {} and not s.depths_raw and s.depth_staged is None
            assert list(s.poses) == list(scene.poses) and np.array_equal(s.points, scene.points)
        assert list(both.masks) == ["table", "chair"] and len(got.mask_2d) == len(scene.mask_2d)


# ------------------------------------------------------------------ header and binding
def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 14
    m = re.search(r"int bff_render_splat_depth_u16\(([^;]*)\);", header)
    assert m, "bff_render_splat_depth_u16 is not declared"
    kinds, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        kinds.append(_lib._P if "*" in arg else {"int64_t": _lib._L, "int32_t": _lib._I, "double": _lib._D,
                                                 "float": _lib._F}[arg.split()[0]])
    assert kinds == _lib.SIGNATURES["bff_render_splat_depth_u16"] and len(kinds) == 16
    old = list(_lib.SIGNATURES["bff_render_depth_u16"])
    at = names.index("splat_radius")
    assert names[at + 1] == "frames_per_block" and kinds[:at] + kinds[at + 1:] == old and kinds[at] is _lib._D
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION
    assert _lib.PLAIN["bff_splat_lane_box"] == (_lib.c_int32, []) and lib.bff_splat_lane_box() >= 1
    fn = lib.bff_render_splat_depth_u16                                 # argument checks run on the host, before any launch
    N = None
    # (xyz, n_points, n_pad, inv_pose, K, n_frames, H, W, dh, dw, splat_radius, frames_per_block, scratch, out, tile_bounds, stream)
    assert fn(N, 0, 0, N, N, 0, 50, 70, 7, 9, 0.02, 0, N, N, N, N) == 0         # no frames: nothing to do
    for bad in (0.0, -0.02, float("nan"), float("inf"), -float("inf")):
        assert fn(N, 0, 0, N, N, 0, 50, 70, 7, 9, bad, 0, N, N, N, N) == -1 and b"splat_radius" in lib.bff_last_error()
    k9 = lambda k00, k11: (_lib.c_double * 9)(k00, 0.0, 34.5, 0.0, k11, 24.5, 0.0, 0.0, 1.0)
    assert fn(N, 0, 0, N, k9(64.0, 64.0), 0, 50, 70, 7, 9, 0.02, 0, N, N, N, N) == 0
    for k00, k11 in ((0.0, 64.0), (-64.0, 64.0), (64.0, 0.0), (float("nan"), 64.0), (64.0, float("inf"))):
        assert fn(N, 0, 0, N, k9(k00, k11), 0, 50, 70, 7, 9, 0.02, 0, N, N, N, N) == -1 and b"K00" in lib.bff_last_error()
    # bff_render_depth_u16's checks, limits and early returns
    assert fn(N, -1, 0, N, N, 0, 1, 1, 1, 1, 0.02, 0, N, N, N, N) == -1
    assert fn(N, 5, 4, N, N, 0, 1, 1, 1, 1, 0.02, 0, N, N, N, N) == -1          # n_pad < n_points
    assert fn(N, 0, 0, N, N, 0, 50, 70, 0, 5, 0.02, 0, N, N, N, N) == -1
    assert fn(N, 0, 0, N, N, 0, 50, 70, 7, 9, 0.02, -1, N, N, N, N) == -1       # frame tile
    assert fn(N, 0, 0, N, N, 0, 65536, 65536, 4, 4, 0.02, 0, N, N, N, N) == -2
    assert fn(N, 0, 0, N, N, 0, 4, 4, 65536, 65536, 0.02, 0, N, N, N, N) == -2
    assert fn(N, 0, 0, N, N, 0, 65536, 4, 65536, 4, 0.02, 0, N, N, N, N) == -2  # height * depth_h
    assert fn(N, 0, 0, N, N, 70000, 4, 4, 4, 4, 0.02, 0, N, N, N, N) == -2
    assert fn(N, 5, 1024, N, N, 1, 50, 70, 7, 9, 0.02, 0, N, N, N, N) == -1 and b"null pointer" in lib.bff_last_error()
    # the plain entry point goes through the same checks and still names itself
    assert lib.bff_render_depth_u16(N, 5, 1024, N, N, 1, 50, 70, 7, 9, 0, N, N, N, N) == -1 \
        and b"bff_render_depth_u16: null pointer" in lib.bff_last_error()
