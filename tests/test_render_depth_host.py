"""Depth rendered from the cloud, the parts that need no GPU: the NumPy reference of bff_render_depth_u16 pinned on
cases worked by hand, the config key, the loaders on a scene directory without depth/, and the binding table."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import render_depth_ref as rd
from oracle import projection_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_three_points_by_hand():
    """K = [[100, 0, 50], [0, 100, 40], [0, 0, 1]], camera at the origin, image 80 x 100, frames 20 x 25.
    A (0, 0, 2):          u = 50, v = 40, 2000 mm -> texel (40 * 20 // 80, 50 * 25 // 100) = (10, 12)
    B (0.02, 0.01, 1.5):  u = rint(51.33) = 51, v = rint(40.67) = 41, 1500 mm -> texel (10, 12) too: the nearer one stays
    C (-1, 0, 2):         u = 0, v = 40, 2000 mm -> texel (10, 0)."""
    k33 = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1]])
    xyz = np.array([[0, 0, 2.0], [0.02, 0.01, 1.5], [-1.0, 0, 2.0]])
    counts = []
    got = rd.render_depth_ref(xyz, np.eye(4).reshape(1, 16), k33, 80, 100, 20, 25, counts)
    exp = np.zeros((1, 20, 25), np.uint16)
    exp[0, 10, 12] = 1500
    exp[0, 10, 0] = 2000
    assert got.dtype == np.uint16 and np.array_equal(got, exp)
    assert counts[0][10, 12] == 2 and counts[0][10, 0] == 1 and counts[0].sum() == 3
    # behind the camera, nearer than half a millimetre, farther than 65.535 m, outside the image, NaN: none splats
    bad = np.array([[0, 0, -2.0], [0, 0, 0.0], [0, 0, 0.0004], [0, 0, 65.5356], [-1.02, 0, 2.0], [np.nan, 0, 2.0]])
    assert not rd.render_depth_ref(bad, np.eye(4).reshape(1, 16), k33, 80, 100, 20, 25).any()
    # the ends of the range: rint(0.6) = 1 and rint(65535.4) = 65535 are kept; half a millimetre rounds to even
    # (0.0005 * 1000.0 == 0.5, 0.0025 * 1000.0 == 2.5 and 65.5355 * 1000.0 == 65535.5 exactly in float64)
    edge = np.array([[0, 0, 0.0006], [-30.0, 0, 65.5354], [0.0001, 0, 0.0005], [-0.0005, 0, 0.0025], [30.0, 0, 65.5355]])
    got = rd.render_depth_ref(edge, np.eye(4).reshape(1, 16), k33, 80, 100, 20, 25)
    assert 0.0005 * 1000.0 == 0.5 and 0.0025 * 1000.0 == 2.5 and 65.5355 * 1000.0 == 65535.5
    assert got[0, 10, 12] == 1 and got[0, 10, 1] == 65535            # u = 50 and u = rint(4.22) = 4
    assert got[0, 10, 17] == 0                                        # u = 70: rint(0.5) = 0 does not splat
    assert got[0, 10, 7] == 2                                         # u = 30: rint(2.5) = 2
    assert got[0, 10, 23] == 0 and np.count_nonzero(got) == 3         # u = rint(95.78) = 96: rint(65535.5) = 65536 is too far


@pytest.mark.parametrize("stride", [1, 4])
def test_reference_two_planes_by_hand(stride):
    """A near plane in front of a far one: inside the near plane's silhouette the frame holds the near depth, outside
    the far one; every texel is covered (one point per pixel)."""
    scene, _, _ = rd.two_plane_scene()
    h, w = scene.height, scene.width
    dh, dw = rd.rendered_size(h, w, stride)
    got = rd.render_depth_ref(scene.points, np.eye(4).reshape(1, 16), scene.cam_intr[:3, :3], h, w, dh, dw)[0]
    exp = np.full((dh, dw), 3000, np.uint16)
    exp[16 // stride:32 // stride, 20 // stride:44 // stride] = 1000      # the rectangle's edges are multiples of 4
    assert np.array_equal(got, exp)
    # through the reference's scene loop (min_aggragated_masks = 1, no point filter): the row of the one full-image mask
    # holds the near points and the far points outside the silhouette -- at stride 1 exactly those
    from beyond_fixed_forms_amd.config import Config
    cfg = Config.with_defaults(width_2d=w, height_2d=h, min_aggragated_masks=1, if_detected_ratio_threshold=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = pref.project_scene_ref(rd.scene_with_rendered_depth(scene, stride), cfg)
    assert out["ins"].shape[0] == 1
    row = out["ins"][0].numpy()
    exp_row, sure = rd.hand_row(stride)
    assert np.array_equal(row[sure], exp_row[sure])
    if stride == 1:
        assert sure.all()




def test_config_key():
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    from beyond_fixed_forms_amd.scene import depth_from_cloud_stride, rendered_depth_size
    assert DEFAULTS["depth_from_cloud"] == 0
    assert depth_from_cloud_stride(Config()) == 0                          # the reference's config file has no such key
    assert depth_from_cloud_stride(Config.with_defaults()) == 0
    assert depth_from_cloud_stride(Config(depth_from_cloud=None)) == 0
    assert depth_from_cloud_stride(Config.with_defaults(depth_from_cloud=8)) == 8
    assert depth_from_cloud_stride(Config(depth_from_cloud=np.int64(2))) == 2
    for bad in (-1, "8", 2.0, True):
        with pytest.raises(ValueError):
            depth_from_cloud_stride(Config(depth_from_cloud=bad))
    assert rendered_depth_size(968, 1296, 8) == (121, 162) and rendered_depth_size(50, 70, 16) == (4, 5)
    assert rendered_depth_size(50, 70, 1) == (50, 70) and rd.rendered_size(50, 70, 8) == rendered_depth_size(50, 70, 8)




def test_loaders_without_depth_folder(tmp_path):
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.io import load_scene, load_scene_classes
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=3, n_points=500)
    rd.write_scene_without_depth(tmp_path, scene, {"table": scene.mask_2d, "chair": scene.mask_2d[:2]})
    assert not (tmp_path / "2d" / scene.scene_id / "depth").exists()
    dirs = dict(width_2d=scene.width, height_2d=scene.height, scene_2d_dir=str(tmp_path / "2d"),
                scene_npy_dir=str(tmp_path / "npy"), mask_2d_dir=str(tmp_path / "m2d"))
    on = Config.with_defaults(depth_from_cloud=8, **dirs)
    for on_device in (False, True):
        got = load_scene(on, "table", scene.scene_id, depth_on_device=on_device)
        assert got.depths == {} and not got.depths_raw and got.depth_staged is None
        assert list(got.poses) == list(scene.poses) and np.array_equal(got.points, scene.points)
        assert len(got.mask_2d) == len(scene.mask_2d) and sorted(got.color_files) == sorted(scene.color_files)
        both = load_scene_classes(on, ["table", "chair"], scene.scene_id, depth_on_device=on_device)
        assert both.scene.depths == {} and not both.scene.depths_raw and list(both.masks) == ["table", "chair"]
        assert list(both.scene.poses) == list(scene.poses)
    # key off (absent or 0): the missing depth file is the error it has always been -- the decoder's own: PIL's
    # FileNotFoundError naming the file, or, where cv2 is installed, the AttributeError of `None.astype` after cv2.imread
    try:
        import cv2  # noqa: F401
        kind = AttributeError
    except ImportError:
        kind = FileNotFoundError
    for off in (Config.with_defaults(**dirs), Config.with_defaults(depth_from_cloud=0, **dirs)):
        with pytest.raises(kind) as e1:
            load_scene(off, "table", scene.scene_id)
        with pytest.raises(kind) as e2:
            load_scene_classes(off, ["table"], scene.scene_id)
        if kind is FileNotFoundError:
            first = scene.mask_2d[0]["frame_id"][:-4]
            for e in (e1, e2):
                assert os.path.join(scene.scene_id, "depth", f"{first}.png") in str(e.value.filename)
        with pytest.raises(FileNotFoundError):                           # the native batch decoder's path (PIL decides)
            load_scene(off, "table", scene.scene_id, depth_on_device=True)


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    m = re.search(r"int bff_render_depth_u16\(([^;]*)\);", header)
    assert m, "bff_render_depth_u16 is not declared"
    kinds = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        kinds.append(_lib._P if "*" in arg else {"int64_t": _lib._L, "int32_t": _lib._I, "double": _lib._D,
                                                 "float": _lib._F}[arg.split()[0]])
    assert kinds == _lib.SIGNATURES["bff_render_depth_u16"]
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 10
    lib = _lib.load()                                                    # argument checks run on the host, before any launch
    assert lib.bff_render_depth_u16(None, -1, 0, None, None, 0, 1, 1, 1, 1, 0, None, None, None, None) == -1
    assert lib.bff_render_depth_u16(None, 0, 0, None, None, 0, 50, 70, 0, 5, 0, None, None, None, None) == -1
    assert lib.bff_render_depth_u16(None, 0, 0, None, None, 0, 65536, 65536, 4, 4, 0, None, None, None, None) == -2
    assert lib.bff_render_depth_u16(None, 0, 0, None, None, 0, 4, 4, 65536, 65536, 0, None, None, None, None) == -2
    assert lib.bff_render_depth_u16(None, 0, 0, None, None, 70000, 4, 4, 4, 4, 0, None, None, None, None) == -2
    assert lib.bff_render_depth_u16(None, 0, 0, None, None, 0, 50, 70, 7, 9, 0, None, None, None, None) == 0    # no frames
    assert lib.bff_render_depth_u16(None, 0, 0, None, None, 0, 50, 70, 7, 9, -1, None, None, None, None) == -1  # frame tile
    assert lib.bff_render_depth_u16(None, 5, 1024, None, None, 1, 50, 70, 7, 9, 0, None, None, None, None) == -1 \
        and b"null pointer" in lib.bff_last_error()
