"""Depth frames rasterised from a triangle mesh (bff_render_mesh_depth_u16) on the GPU: the kernel against its NumPy
statement (tests/mesh_depth_ref.py), byte for byte, and scenes without depth frames against the oracle fed with the
frames the reference would have read had the rasterised frames been its depth PNGs.  Everything is compared for equality."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

import mesh_depth_ref as md
import render_depth_ref as rd
from oracle import projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, F = 50, 70, 5
K33 = np.array([[64.0, 0.0, 34.5], [0.0, 64.0, 24.5], [0.0, 0.0, 1.0]])
SIZES = [(50, 70), (25, 35), (13, 18), (7, 9)]
ROWS, COLS = 24, 32


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def at_pixel(u, v, z):
    """A vertex (camera 0 = world coordinates) that projects to pixel (u, v) at depth z."""
    return [(u - K33[0, 2]) * z / 64.0, (v - K33[1, 2]) * z / 64.0, z]


# hand triangles, as pixel positions and depths in frame 0 (the identity pose)
HAND = {
    "winding a": [(12, 8, 2.0), (20, 8, 2.0), (12, 16, 2.2)],
    "winding b": [(40, 8, 2.0), (40, 16, 2.2), (48, 8, 2.0)],
    "collinear": [(5.25, 5.25, 2.0), (15.25, 15.25, 2.0), (25.25, 25.25, 2.0)],       # three distinct vertices on a line
    "nan vertex": [(30, 30, 2.0), (36, 30, 2.0), (np.nan, 36, 2.0)],
    "behind": [(30, 30, -2.0), (36, 30, -2.0), (30, 36, -2.5)],
    "straddling": [(30, 40, 2.0), (36, 40, 2.0), (33, 44, -0.5)],
    "partly outside": [(60, 40, 1.5), (90, 44, 1.5), (62, 70, 1.6)],
    "wholly outside": [(100, 10, 2.0), (120, 10, 2.0), (110, 30, 2.0)],
    "whole frame": [(-200, -100, 6.0), (300, -100, 6.0), (35, 400, 6.5)],              # behind the field: the wave path
    "lane box": [(10.3, 10.3, 1.9), (14.6, 10.4, 1.9), (12.0, 14.6, 1.9)],             # 8 x 8 texels at (50, 70): the lane's
    "lane box + 1": [(30.3, 10.3, 1.9), (31.6, 10.4, 1.9), (31.0, 19.6, 1.9)],         # 5 x 13 = 65 texels: the wave's
    "near over far a": [(50, 20, 2.5), (64, 20, 2.5), (57, 34, 2.5)],
    "near over far b": [(52, 22, 1.2), (62, 22, 1.2), (57, 30, 1.2)],
}


@functools.lru_cache(maxsize=None)
def mesh():
    """-> (vertices (V, 3), faces (T, 3), inverse poses (F, 16), index of the first hand triangle): a 24 x 32-vertex wavy
    height field that fills the image of camera 0 and a little more, the hand triangles (and one that names a vertex
    twice), 5 poses of which the first is the identity; the faces in random order."""
    rng = np.random.default_rng(11)
    i, j = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    z = 3.0 + 0.25 * np.sin(0.9 * i) + 0.2 * np.cos(0.7 * j)
    u, v = -5 + 80 * j / (COLS - 1), -5 + 60 * i / (ROWS - 1)
    field = np.stack([(u - K33[0, 2]) * z / 64.0, (v - K33[1, 2]) * z / 64.0, z], -1).reshape(-1, 3)
    hand = np.array([at_pixel(*p) for tri in HAND.values() for p in tri])
    hand[np.isnan(hand).any(1)] = [np.nan, 0.1, 2.0]
    n0 = field.shape[0]
    hand_faces = np.arange(n0, n0 + hand.shape[0]).reshape(-1, 3)
    twice = np.array([[n0, n0, n0 + 1], [n0 + 3, n0 + 4, n0 + 3]])       # a repeated index
    faces = np.concatenate([md.grid_faces(ROWS, COLS), hand_faces, twice])
    inv = np.zeros((F, 16))
    inv[0] = np.eye(4).reshape(-1)
    for f in range(1, F):
        a, b = rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2)
        pose = np.eye(4)
        pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ \
            np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        pose[:3, 3] = rng.uniform(-0.6, 0.6, 3)
        inv[f] = np.linalg.inv(pose).reshape(-1)
    order = rng.permutation(faces.shape[0])
    return np.concatenate([field, hand]), faces[order], inv, np.argsort(order)[2 * (ROWS - 1) * (COLS - 1):]


@functools.lru_cache(maxsize=None)
def reference(dh, dw):
    vertices, faces, inv, _ = mesh()
    covered = []
    return md.render_mesh_ref(vertices, faces, inv, K33, H, W, dh, dw, covered), np.stack(covered)


def hand_frame(name, dh=H, dw=W):
    """Frame 0 of one hand triangle alone."""
    vertices, faces, inv, hand_at = mesh()
    k = list(HAND).index(name)
    return md.render_mesh_ref(vertices, faces[hand_at[k]:hand_at[k] + 1], inv[:1], K33, H, W, dh, dw)[0]


def box_texels(name, dh=H, dw=W):
    """Texels of the clipped box the header documents for a hand triangle in frame 0 (bff_mesh_lane_box)."""
    p = np.array(HAND[name])
    out = 1
    for lo, hi, s, n in ((p[:, 0].min(), p[:, 0].max(), W / dw, dw), (p[:, 1].min(), p[:, 1].max(), H / dh, dh)):
        first = max(np.floor((lo + 0.5) / s - 0.5) - 1, 0)
        last = min(np.ceil((hi + 0.5) / s - 0.5) + 1, n - 1)
        out *= int(max(last - first + 1, 0))
    return out


def test_hand_triangles_are_what_they_claim(lib):
    """On the reference, frame 0: what each hand triangle is there for."""
    for name in ("winding a", "winding b", "partly outside", "whole frame", "lane box", "lane box + 1", "near over far a"):
        assert hand_frame(name).any(), name
    for name in ("collinear", "nan vertex", "behind", "straddling", "wholly outside"):
        assert not hand_frame(name).any(), name
    assert (hand_frame("whole frame") != 0).all() and (hand_frame("whole frame", 7, 9) != 0).all()
    lane = lib.load().bff_mesh_lane_box()
    assert box_texels("lane box") == lane == 64 and box_texels("lane box + 1") == lane + 1
    assert box_texels("whole frame") == H * W and box_texels("wholly outside") == 0 and 0 < box_texels("partly outside") < H * W
    ref, covered = reference(H, W)
    near, far = hand_frame("near over far b"), hand_frame("near over far a")
    both = (near != 0) & (far != 0)
    assert both.any() and (ref[0][both] == near[both]).all() and (near[both] < far[both]).all()
    assert (ref != 0).all(axis=(1, 2)).any() and (covered >= 3).any()     # the whole-frame triangle leaves no hole in frame 0
    for dh, dw in SIZES:
        r, c = reference(dh, dw)
        assert ((c == 0) <= (r == 0)).all() and (c >= 2).any()          # contested texels at every size


def render(lib, dh, dw, faces=None, vertices=None, **kw):
    v, f, inv, _ = mesh()
    v = v if vertices is None else vertices
    f = f if faces is None else faces
    n_pad = (v.shape[0] + 255) // 256 * 256
    soa = np.zeros((3, n_pad))
    soa[:, :v.shape[0]] = v.T
    soa[:, v.shape[0]:] = np.array([[0.0], [0.0], [0.5]])       # padding that would draw 500 mm at the image centre if read
    out = lib.render_mesh_depth(torch.from_numpy(soa).to(DEV), v.shape[0], torch.from_numpy(f.astype(np.int32)).to(DEV),
                                torch.from_numpy(inv).to(DEV), K33, H, W, dh, dw, **kw)
    assert out.dtype == torch.int16 and tuple(out.shape) == (F, dh, dw)
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("tile", [0, 1, 3, 8])
@pytest.mark.parametrize("dh,dw", SIZES)
def test_kernel_equals_reference(lib, dh, dw, tile):
    ref, _ = reference(dh, dw)
    got = render(lib, dh, dw, frames_per_block=tile)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:10]
    assert render(lib, dh, dw, frames_per_block=tile).tobytes() == got.tobytes()          # the same bytes on every run


@pytest.mark.parametrize("dh,dw", SIZES[:2])
def test_face_order_does_not_matter(lib, dh, dw):
    """Random order (the fixture's) and the launch order of scene.mesh_for_render (sorted by smallest vertex)."""
    from beyond_fixed_forms_amd.scene import mesh_for_render
    _, faces, _, _ = mesh()
    ref, _ = reference(dh, dw)
    dev_faces = torch.from_numpy(faces.astype(np.int32)).to(DEV)
    _, _, ordered = mesh_for_render(dev_faces, None, 0, vertices=torch.zeros(1, device=DEV), n_vertices=1)
    ordered = ordered.cpu().numpy()
    assert (np.diff(ordered.min(1)) >= 0).all() and not np.array_equal(ordered, faces)
    assert sorted(map(tuple, ordered.tolist())) == sorted(map(tuple, faces.tolist()))
    assert np.array_equal(render(lib, dh, dw, faces=ordered), ref)
    assert np.array_equal(render(lib, dh, dw, faces=faces[::-1].copy()), ref)


def test_scratch_smaller_than_the_frames(lib):
    """A scratch that holds 2 of the 5 frames: three runs (2, 2, 1), the same bytes; and frame by frame."""
    ref, _ = reference(13, 18)
    assert np.array_equal(render(lib, 13, 18, scratch_texels=2 * 13 * 18 + 5), ref)
    assert np.array_equal(render(lib, 13, 18, scratch_texels=1, frames_per_block=8), ref)


def test_empty_inputs_return_cleanly(lib):
    v, f, inv, _ = mesh()
    soa = torch.zeros((3, 1024), dtype=torch.float64, device=DEV)
    faces = torch.from_numpy(f.astype(np.int32)).to(DEV)
    none = lib.render_mesh_depth(soa, 1000, faces, torch.zeros((0, 16), dtype=torch.float64, device=DEV), K33, H, W, 7, 9)
    assert tuple(none.shape) == (0, 7, 9)
    out = lib.render_mesh_depth(soa, 1000, faces[:0], torch.from_numpy(inv).to(DEV), K33, H, W, 7, 9)    # no triangle
    torch.cuda.synchronize()
    assert tuple(out.shape) == (F, 7, 9) and int(out.count_nonzero()) == 0
    with pytest.raises(ValueError):
        lib.render_mesh_depth(soa, 1000, faces.long(), torch.from_numpy(inv).to(DEV), K33, H, W, 7, 9)


@pytest.mark.parametrize("sort_points", [True, False])
def test_own_vertices_and_cloud_indices_give_the_same_frames(lib, sort_points, monkeypatch):
    """The same mesh given with its own vertices and as faces into the cloud (whose rows are those vertices): the same
    frames, with the cloud Morton-sorted on the device (the faces are remapped through the permutation) and left as it is;
    prepared by scene.py and by ingest.py."""
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.ingest import prepare_geometry_fast
    from beyond_fixed_forms_amd.scene import prepare_geometry
    from beyond_fixed_forms_amd.synthetic import SceneInputs
    vertices, faces, inv, _ = mesh()
    ok = ~np.isnan(vertices).any(1)                                      # the cloud's Morton sort takes finite points
    vertices = vertices[ok]
    faces = (np.cumsum(ok) - 1)[faces[ok[faces].all(1)]]
    poses = {str(k): np.linalg.inv(inv[k].reshape(4, 4)) for k in range(F)}
    cam = np.eye(4)
    cam[:3, :3] = K33
    masks = [{"frame_id": f"{k}.jpg", "segmented_frame_masks": [], "confidences": torch.zeros(0, dtype=torch.float16),
              "labels": []} for k in range(F)]
    cloud = np.concatenate([vertices, np.zeros_like(vertices)], 1)
    other = np.random.default_rng(3).uniform(-1, 1, (300, 6))            # a cloud that is not the mesh's vertices
    scenes = [SceneInputs("s", cloud, cam, poses, {}, masks, [], height=H, width=W, faces=faces),
              SceneInputs("s", other, cam, poses, {}, masks, [], height=H, width=W, faces=faces, mesh_vertices=vertices)]
    cfg = Config.with_defaults(width_2d=W, height_2d=H, depth_from_mesh=2)
    ref = md.render_mesh_ref(vertices, faces, np.stack([np.linalg.inv(poses[str(k)]) for k in range(F)]), K33, H, W, 25, 35)
    monkeypatch.setenv("BFF_DEPTH_TILES", "0")                           # the resident frames stay row-major: read them back
    for scene in scenes:
        geoms = [prepare_geometry(scene, cfg, [masks], DEV, with_viewed=False, sort_points=sort_points)]
        if sort_points:
            geoms.append(prepare_geometry_fast(scene, cfg, [masks], DEV, with_viewed=False))
        for g in geoms:
            assert (g.unsort is not None) == sort_points and g.depth_raw is not None and g.depth is None
            assert np.array_equal(g.depth_raw.cpu().numpy().view(np.uint16), ref)


# ------------------------------------------------------------------ scenes without depth frames against the oracle
FILTERS = {"ratio": {}, "occurrence": dict(if_occurance_threshold=True), "none": dict(if_detected_ratio_threshold=False)}
SEED = 74


def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


@functools.lru_cache(maxsize=None)
def generated():
    """A small generated scene without depth frames whose mesh (the room and the cuboids, its own vertices) is independent
    of the cloud."""
    from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh
    scene = rd.without_depth(make_scene("tiny", seed=SEED))
    scene.mesh_vertices, scene.faces = make_scene_mesh(seed=SEED)
    return scene


@functools.lru_cache(maxsize=None)
def two_planes():
    return md.two_plane_mesh_scene()[0]


SCENES = {"generated": (generated, {}), "two planes": (two_planes, dict(min_aggragated_masks=1))}


@functools.lru_cache(maxsize=None)
def with_depth(which, stride):
    return md.scene_with_rendered_depth(SCENES[which][0](), stride)


@functools.lru_cache(maxsize=None)
def expected(which, stride, filt):
    ref_scene = with_depth(which, stride)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pref.project_scene_ref(ref_scene, cfg_for(ref_scene, **SCENES[which][1], **FILTERS[filt]))
    assert exp["ins"].dim() == 2 and exp["ins"].shape[0] >= 1 and len(exp["final_class"]) >= 1     # the oracle keeps an instance
    return exp


def same(got, exp):
    assert got["ins"].dtype == exp["ins"].dtype and tuple(got["ins"].shape) == tuple(exp["ins"].shape)
    assert torch.equal(got["ins"].cpu(), exp["ins"].cpu())
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"].cpu())
    assert list(got["final_class"]) == list(exp["final_class"])


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("which", list(SCENES))
def test_scene_equals_oracle(lib, which, stride, filt):
    """project_scene on a scene that has a mesh and no depth frames: the one-call path behind prepare_scene_fast, and
    debug_out=True behind prepare_scene.  Two planes: the faces index the cloud; generated: the mesh has its own vertices."""
    from beyond_fixed_forms_amd.projection import project_scene
    scene = SCENES[which][0]()
    assert scene.depths == {} and scene.depths_raw is None
    cfg = cfg_for(scene, depth_from_mesh=stride, **SCENES[which][1], **FILTERS[filt])
    exp = expected(which, stride, filt)
    same(project_scene(scene, cfg, DEV), exp)
    same(project_scene(scene, cfg, DEV, debug_out=True), exp)


def test_two_planes_by_hand(lib):
    """A near plane in front of a far one, both triangulated, and a full-image mask at stride 1: the row holds the near
    points and exactly the far points outside the near plane's silhouette."""
    from beyond_fixed_forms_amd.projection import project_scene
    scene = two_planes()
    got = project_scene(scene, cfg_for(scene, depth_from_mesh=1, min_aggragated_masks=1, if_detected_ratio_threshold=False), DEV)
    exp_row, sure = rd.hand_row(1)
    assert got["ins"].shape[0] == 1 and sure.all() and np.array_equal(got["ins"][0].cpu().numpy(), exp_row)


def test_both_keys_and_bad_faces_raise(lib):
    from beyond_fixed_forms_amd.ingest import prepare_scene_fast
    from beyond_fixed_forms_amd.scene import prepare_scene
    import copy
    scene = generated()
    for prep in (prepare_scene, prepare_scene_fast):
        with pytest.raises(ValueError, match="both"):
            prep(scene, cfg_for(scene, depth_from_mesh=2, depth_from_cloud=8), device=DEV)
        bad = copy.copy(scene)
        bad.faces = scene.faces.copy()
        bad.faces[5, 1] = scene.mesh_vertices.shape[0]
        with pytest.raises(ValueError, match="outside"):
            prep(bad, cfg_for(scene, depth_from_mesh=2), device=DEV)
        bad.faces = None
        with pytest.raises(ValueError):
            prep(bad, cfg_for(scene, depth_from_mesh=2), device=DEV)


@pytest.mark.parametrize("debug_out", [False, True])
def test_two_classes_render_once(lib, debug_out, monkeypatch):
    """project_scene_classes: depth lives in the shared geometry, so the mesh is rasterised once per scene; every class
    equals its single-class run and the oracle."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes
    from beyond_fixed_forms_amd.synthetic import class_scene
    stride = 2
    scene, ref_scene = generated(), with_depth("generated", stride)
    cfg = cfg_for(scene, depth_from_mesh=stride)
    masks = {"table": scene.mask_2d,
             "chair": [dict(fr, labels=["chair"] * len(fr["labels"])) for fr in scene.mask_2d[1:]]}
    calls = []
    real = _lib.render_mesh_depth
    monkeypatch.setattr(_lib, "render_mesh_depth", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(_lib, "render_depth", lambda *a, **k: pytest.fail("the point renderer ran"))
    got = project_scene_classes(scene, masks, cfg, DEV, debug_out=debug_out)
    assert len(calls) == 1
    for c, m in masks.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp = pref.project_scene_ref(class_scene(ref_scene, m), cfg_for(ref_scene))
        assert len(exp["final_class"]) >= 1
        same(got[c], exp)
        same(got[c], project_scene(class_scene(scene, m), cfg, DEV, debug_out=debug_out))


# ------------------------------------------------------------------ the stage script on a tree without depth/
def test_stage_script_without_depth_folder(tmp_path):
    from beyond_fixed_forms_amd.synthetic import class_scene
    stride = 2
    scene, ref_scene = generated(), with_depth("generated", stride)
    masks = {"table": scene.mask_2d,
             "chair": [dict(fr, labels=["chair"] * len(fr["labels"])) for fr in scene.mask_2d[1:]]}
    rd.write_scene_without_depth(tmp_path, scene, masks)
    md.write_mesh(tmp_path, scene)
    assert not (tmp_path / "2d" / scene.scene_id / "depth").exists()
    cfg = cfg_for(scene, depth_from_mesh=stride, scene_2d_dir=str(tmp_path / "2d"), scene_npy_dir=str(tmp_path / "npy"),
                  mask_2d_dir=str(tmp_path / "m2d"), mask_3d_dir=str(tmp_path / "m3d"), scene_mesh_dir=str(tmp_path / "mesh"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    argv = [sys.executable, os.path.join(ROOT, "tools", "projection_2d_to_3d.py"), "--config", str(tmp_path / "config.yaml"),
            "--cls", "table", "--cls", "chair"]                          # several classes: the scene is read and rendered once
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for cls in masks:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp = pref.project_scene_ref(class_scene(ref_scene, masks[cls]), cfg)
        got = torch.load(tmp_path / "m3d" / cls / f"{scene.scene_id}.pth", map_location="cpu", weights_only=False)
        assert len(exp["final_class"]) >= 1
        same(got, exp)
