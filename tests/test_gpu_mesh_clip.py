"""Mesh depth clipped at a near plane (bff_render_mesh_depth_clip_u16) on the GPU: the kernel against its NumPy statement
(tests/mesh_clip_ref.py), byte for byte, and scenes without depth frames with the config key `mesh_near_clip` against
the oracle fed with the clipped frames.  Everything is compared for equality."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

import mesh_clip_ref as mc
import mesh_depth_ref as md
import render_depth_ref as rd
from oracle import projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def render(lib, vertices, faces, inv, k33, h, w, dh, dw, **kw):
    n_pad = (vertices.shape[0] + 255) // 256 * 256
    soa = np.zeros((3, n_pad))
    soa[:, :vertices.shape[0]] = vertices.T
    soa[:, vertices.shape[0]:] = np.array([[0.0], [0.0], [0.6]])       # padding that would draw 600 mm at the image centre if read
    out = lib.render_mesh_depth(torch.from_numpy(soa).to(DEV), vertices.shape[0],
                                torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV),
                                torch.from_numpy(np.array(inv)).to(DEV), k33, h, w, dh, dw, **kw)
    assert out.dtype == torch.int16 and tuple(out.shape) == (inv.shape[0], dh, dw)
    return out.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------ the box room
ROOM_SIZES = [(48, 64), (12, 16), (7, 9)]


@functools.lru_cache(maxsize=None)
def room_reference(dh, dw, zn):
    vertices, faces, inv = mc.box_room()
    fans = []
    frames = mc.render_clip_ref(vertices, faces, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, dh, dw, zn, fans)
    frames.setflags(write=False)
    return frames, fans


@pytest.mark.parametrize("zn", [0.05, 0.25])
@pytest.mark.parametrize("tile", [0, 1, 3, 8])
@pytest.mark.parametrize("dh,dw", ROOM_SIZES)
def test_kernel_equals_reference_in_the_box_room(lib, dh, dw, tile, zn):
    vertices, faces, inv = mc.box_room()
    ref, _ = room_reference(dh, dw, zn)
    got = render(lib, vertices, faces, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, dh, dw, frames_per_block=tile, near_clip=zn)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:10]
    again = render(lib, vertices, faces, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, dh, dw, frames_per_block=tile, near_clip=zn)
    assert again.tobytes() == got.tobytes()                              # the same bytes on every run
    if zn == 0.05:
        assert (got != 0).all()                                         # a closed room seen from inside


def test_clipped_triangles_take_both_walks(lib):
    """From the reference's texel boxes: fan triangles of clipped polygons are walked by their lane (at most
    bff_mesh_lane_box() texels) at the coarse size and by the wave at the fine one; quadrilaterals occur."""
    lane = lib.load().bff_mesh_lane_box()
    for zn in (0.05, 0.25):
        counts = {}
        for dh, dw in ROOM_SIZES:
            _, fans = room_reference(dh, dw, zn)
            boxes = [mc.box_texels(fan, t, mc.ROOM_H, mc.ROOM_W, dh, dw) for fan in fans for t in np.flatnonzero(fan["cut"])]
            counts[dh, dw] = (sum(0 < b <= lane for b in boxes), sum(b > lane for b in boxes))
            sources = [np.bincount(fan["source"][fan["cut"]]) for fan in fans if fan["cut"].any()]
            assert any((s == 2).any() for s in sources) and any((s == 1).any() for s in sources)
        print(f"zn {zn}: (lane walks, wave walks) of clipped fan triangles per size {counts}")
        assert counts[7, 9][0] > 0 and counts[48, 64][1] > 0
        assert counts[7, 9][1] == 0 and 7 * 9 <= lane


# ------------------------------------------------------------------ the hand cases as one mesh
HAND_SIZES = [(50, 70), (13, 18)]


@functools.lru_cache(maxsize=None)
def hand_poses():
    """The identity, at which the cases are what their names say, and three poses near it."""
    rng = np.random.default_rng(5)
    inv = [np.eye(4).reshape(-1)]
    for _ in range(3):
        a, b = rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2)
        pose = np.eye(4)
        pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ \
            np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        pose[:3, 3] = rng.uniform(-0.3, 0.3, 3)
        inv.append(np.linalg.inv(pose).reshape(-1))
    return np.stack(inv)


@functools.lru_cache(maxsize=None)
def hand_reference(dh, dw):
    vertices, faces = mc.hand_mesh()
    ref = mc.render_clip_ref(vertices, faces, hand_poses(), mc.HAND_K, mc.HAND_H, mc.HAND_W, dh, dw, mc.HAND_ZN)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("dh,dw", HAND_SIZES)
def test_hand_cases_in_any_face_order(lib, dh, dw):
    from beyond_fixed_forms_amd.scene import mesh_for_render
    vertices, faces = mc.hand_mesh()
    ref = hand_reference(dh, dw)
    assert ref[0].any() and (ref[0] == 0).any()
    args = (hand_poses(), mc.HAND_K, mc.HAND_H, mc.HAND_W, dh, dw)
    shuffled = faces[np.random.default_rng(7).permutation(faces.shape[0])]
    assert not np.array_equal(shuffled, faces)
    assert np.array_equal(render(lib, vertices, shuffled, *args, near_clip=mc.HAND_ZN), ref)
    _, _, ordered = mesh_for_render(torch.from_numpy(shuffled.astype(np.int32)).to(DEV), None, 0,
                                    vertices=torch.zeros(1, device=DEV), n_vertices=1)
    ordered = ordered.cpu().numpy()
    assert (np.diff(ordered.min(1)) >= 0).all() and sorted(map(tuple, ordered.tolist())) == sorted(map(tuple, faces.tolist()))
    assert np.array_equal(render(lib, vertices, ordered, *args, near_clip=mc.HAND_ZN), ref)
    assert np.array_equal(render(lib, vertices, faces, *args, near_clip=mc.HAND_ZN, frames_per_block=3), ref)


# ------------------------------------------------------------------ a mesh that never comes nearer than zn
H, W, F = 50, 70, 5
K33 = np.array([[64.0, 0.0, 34.5], [0.0, 64.0, 24.5], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def far_field():
    """A 24 x 32-vertex wavy height field at z of about 3 that fills the image of camera 0 and a little more; 5 poses within
    0.6 m of the origin, the first the identity; the faces in random order."""
    rng = np.random.default_rng(11)
    rows, cols = 24, 32
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = 3.0 + 0.25 * np.sin(0.9 * i) + 0.2 * np.cos(0.7 * j)
    u, v = -5 + 80 * j / (cols - 1), -5 + 60 * i / (rows - 1)
    field = np.stack([(u - K33[0, 2]) * z / 64.0, (v - K33[1, 2]) * z / 64.0, z], -1).reshape(-1, 3)
    inv = np.zeros((F, 16))
    inv[0] = np.eye(4).reshape(-1)
    for f in range(1, F):
        a, b = rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2)
        pose = np.eye(4)
        pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ \
            np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        pose[:3, 3] = rng.uniform(-0.6, 0.6, 3)
        inv[f] = np.linalg.inv(pose).reshape(-1)
    faces = md.grid_faces(rows, cols)
    return field, faces[rng.permutation(faces.shape[0])], inv


@pytest.mark.parametrize("dh,dw", [(50, 70), (13, 18)])
def test_mesh_beyond_the_plane_gives_the_old_bytes(lib, dh, dw, monkeypatch):
    vertices, faces, inv = far_field()
    for k in range(F):
        assert mc.camera_points(vertices, inv[k], K33)[:, 2].min() > 1.0
    names = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    old = render(lib, vertices, faces, inv, K33, H, W, dh, dw)
    assert old.any() and names == ["bff_render_mesh_depth_u16"]
    assert render(lib, vertices, faces, inv, K33, H, W, dh, dw, near_clip=0.0).tobytes() == old.tobytes()
    assert names == ["bff_render_mesh_depth_u16"] * 2
    for zn in (0.05, 1.0):
        assert render(lib, vertices, faces, inv, K33, H, W, dh, dw, near_clip=zn).tobytes() == old.tobytes()
    assert names[2:] == ["bff_render_mesh_depth_clip_u16"] * 2
    # a scratch that holds 2 of the 5 frames: three runs, the same bytes
    assert render(lib, vertices, faces, inv, K33, H, W, dh, dw, near_clip=0.05, scratch_texels=2 * dh * dw + 5).tobytes() == \
        old.tobytes()
    assert names[4:] == ["bff_render_mesh_depth_clip_u16"] * 3


def test_bad_arguments_and_empty_inputs(lib):
    vertices, faces, inv = mc.box_room()
    for bad in (float("nan"), -0.05, 70.0):
        with pytest.raises(RuntimeError, match="near_clip"):
            render(lib, vertices, faces, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, 7, 9, near_clip=bad)
    soa = torch.zeros((3, 256), dtype=torch.float64, device=DEV)
    soa[2] = 0.6                                                        # every vertex slot would draw if it were read
    dev_faces = torch.from_numpy(faces.astype(np.int32)).to(DEV)
    dev_inv = torch.from_numpy(np.array(inv)).to(DEV)
    none = lib.render_mesh_depth(soa, 8, dev_faces, dev_inv[:0], mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, 7, 9, near_clip=0.05)
    assert tuple(none.shape) == (0, 7, 9)
    with pytest.raises(RuntimeError, match="near_clip"):                # checked before the early return, as the sizes are
        lib.render_mesh_depth(soa, 8, dev_faces, dev_inv[:0], mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, 7, 9, near_clip=70.0)
    for kw in (dict(faces=dev_faces[:0], n=8), dict(faces=dev_faces, n=0)):          # no triangle; no vertex
        out = lib.render_mesh_depth(soa, kw["n"], kw["faces"], dev_inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, 7, 9, near_clip=0.05)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (len(inv), 7, 9) and int(out.count_nonzero()) == 0
    with pytest.raises(ValueError):
        lib.render_mesh_depth(soa, 8, dev_faces.long(), dev_inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, 7, 9, near_clip=0.05)
    # the padding beyond n_vertices is never read as a vertex: a triangle that names it is not drawn
    ref, _ = room_reference(7, 9, 0.05)
    beyond = np.concatenate([faces, [[8, 9, 10]]])
    assert np.array_equal(render(lib, vertices, beyond, inv, mc.ROOM_K, mc.ROOM_H, mc.ROOM_W, 7, 9, near_clip=0.05), ref)


# ------------------------------------------------------------------ scenes without depth frames against the oracle
FILTERS = {"ratio": {}, "occurrence": dict(if_occurance_threshold=True), "none": dict(if_detected_ratio_threshold=False)}
SEED = 74
ZN = 0.05


def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


@functools.lru_cache(maxsize=None)
def generated():
    """The generated scene without depth frames; its mesh is the room and the cuboids, one cell per face: every wall
    reaches behind some camera."""
    from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh
    scene = rd.without_depth(make_scene("tiny", seed=SEED))
    scene.mesh_vertices, scene.faces = make_scene_mesh(seed=SEED)
    return scene


@functools.lru_cache(maxsize=None)
def clipped_frames(stride):
    scene = generated()
    inv = np.stack([np.linalg.inv(np.asarray(scene.poses[f], np.float64)) for f in scene.poses])
    frames = mc.render_clip_ref(*md.scene_mesh(scene), inv, np.asarray(scene.cam_intr, np.float64)[:3, :3], scene.height,
                                scene.width, *md.rendered_size(scene.height, scene.width, stride), ZN)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def with_depth(stride):
    return mc.scene_with_rendered_depth(generated(), stride, ZN)


@functools.lru_cache(maxsize=None)
def expected(stride, filt):
    ref_scene = with_depth(stride)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pref.project_scene_ref(ref_scene, cfg_for(ref_scene, **FILTERS[filt]))
    assert exp["ins"].dim() == 2 and exp["ins"].shape[0] >= 1 and len(exp["final_class"]) >= 1     # the oracle keeps an instance
    return exp


def same(got, exp):
    assert got["ins"].dtype == exp["ins"].dtype and tuple(got["ins"].shape) == tuple(exp["ins"].shape)
    assert torch.equal(got["ins"].cpu(), exp["ins"].cpu())
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"].cpu())
    assert list(got["final_class"]) == list(exp["final_class"])


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("stride", [1, 2, 4])
def test_scene_equals_oracle(lib, stride, filt):
    """project_scene with depth_from_mesh and mesh_near_clip: the one-call path behind prepare_scene_fast, and
    debug_out=True behind prepare_scene."""
    from beyond_fixed_forms_amd.projection import project_scene
    scene = generated()
    assert scene.depths == {} and scene.depths_raw is None and (clipped_frames(stride) != 0).all()
    cfg = cfg_for(scene, depth_from_mesh=stride, mesh_near_clip=ZN, **FILTERS[filt])
    exp = expected(stride, filt)
    same(project_scene(scene, cfg, DEV), exp)
    same(project_scene(scene, cfg, DEV, debug_out=True), exp)


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_resident_frames_are_the_clipped_frames(lib, stride, monkeypatch):
    from beyond_fixed_forms_amd.ingest import prepare_geometry_fast
    from beyond_fixed_forms_amd.scene import prepare_geometry
    scene = generated()
    cfg = cfg_for(scene, depth_from_mesh=stride, mesh_near_clip=ZN)
    monkeypatch.setenv("BFF_DEPTH_TILES", "0")                           # the resident frames stay row-major: read them back
    ids = list(scene.poses)
    for prep in (prepare_geometry, prepare_geometry_fast):
        g = prep(scene, cfg, [scene.mask_2d], DEV, with_viewed=False)
        assert g.depth_raw is not None and g.depth is None
        got = g.depth_raw.cpu().numpy().view(np.uint16)
        order = [ids.index(f) for f in g.frame_ids]
        assert np.array_equal(got, clipped_frames(stride)[order])
        dropped = prep(scene, cfg_for(scene, depth_from_mesh=stride), [scene.mask_2d], DEV, with_viewed=False)
        assert (dropped.depth_raw == 0).any() and not (g.depth_raw == 0).any()      # the key is what changes the frames


def test_key_without_the_mesh_key_raises(lib):
    from beyond_fixed_forms_amd.ingest import prepare_geometry_fast, prepare_scene_fast
    from beyond_fixed_forms_amd.scene import prepare_geometry, prepare_scene
    scene = generated()
    for cfg in (cfg_for(scene, mesh_near_clip=ZN), cfg_for(scene, depth_from_cloud=8, mesh_near_clip=ZN)):
        for prep in (prepare_scene, prepare_scene_fast):
            with pytest.raises(ValueError, match="depth_from_mesh"):
                prep(scene, cfg, device=DEV)
        for prep in (prepare_geometry, prepare_geometry_fast):
            with pytest.raises(ValueError, match="depth_from_mesh"):
                prep(scene, cfg, [scene.mask_2d], DEV, with_viewed=False)
    with pytest.raises(ValueError, match="mesh_near_clip"):
        prepare_scene_fast(scene, cfg_for(scene, depth_from_mesh=2, mesh_near_clip=70), device=DEV)


@pytest.mark.parametrize("debug_out", [False, True])
def test_two_classes_render_once(lib, debug_out, monkeypatch):
    """project_scene_classes: depth lives in the shared geometry, so the mesh is rasterised once per scene, clipped; every
    class equals its single-class run and the oracle."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes
    from beyond_fixed_forms_amd.synthetic import class_scene
    stride = 2
    scene, ref_scene = generated(), with_depth(stride)
    cfg = cfg_for(scene, depth_from_mesh=stride, mesh_near_clip=ZN)
    masks = {"table": scene.mask_2d,
             "chair": [dict(fr, labels=["chair"] * len(fr["labels"])) for fr in scene.mask_2d[1:]]}
    calls = []
    real = _lib.render_mesh_depth
    monkeypatch.setattr(_lib, "render_mesh_depth", lambda *a, **k: (calls.append(k.get("near_clip")), real(*a, **k))[1])
    got = project_scene_classes(scene, masks, cfg, DEV, debug_out=debug_out)
    assert calls == [ZN]
    for c, m in masks.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp = pref.project_scene_ref(class_scene(ref_scene, m), cfg_for(ref_scene))
        assert len(exp["final_class"]) >= 1
        same(got[c], exp)
        same(got[c], project_scene(class_scene(scene, m), cfg, DEV, debug_out=debug_out))


# ------------------------------------------------------------------ the stage script on a tree without depth/
def test_stage_script_with_the_key_in_the_yaml(tmp_path):
    from beyond_fixed_forms_amd.synthetic import class_scene
    stride = 2
    scene, ref_scene = generated(), with_depth(stride)
    masks = {"table": scene.mask_2d}
    rd.write_scene_without_depth(tmp_path, scene, masks)
    md.write_mesh(tmp_path, scene)
    assert not (tmp_path / "2d" / scene.scene_id / "depth").exists()
    cfg = cfg_for(scene, depth_from_mesh=stride, mesh_near_clip=ZN, scene_2d_dir=str(tmp_path / "2d"),
                  scene_npy_dir=str(tmp_path / "npy"), mask_2d_dir=str(tmp_path / "m2d"), mask_3d_dir=str(tmp_path / "m3d"),
                  scene_mesh_dir=str(tmp_path / "mesh"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    assert yaml.safe_load((tmp_path / "config.yaml").read_text())["mesh_near_clip"] == ZN
    argv = [sys.executable, os.path.join(ROOT, "tools", "projection_2d_to_3d.py"), "--config", str(tmp_path / "config.yaml"),
            "--cls", "table"]
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pref.project_scene_ref(class_scene(ref_scene, masks["table"]), cfg)
        dropped = pref.project_scene_ref(class_scene(md.scene_with_rendered_depth(scene, stride), masks["table"]), cfg)
    got = torch.load(tmp_path / "m3d" / "table" / f"{scene.scene_id}.pth", map_location="cpu", weights_only=False)
    assert len(exp["final_class"]) >= 1
    same(got, exp)
    print("clipped and dropped frames give", "the same" if torch.equal(exp["ins"], dropped["ins"]) else "different", "instances")
