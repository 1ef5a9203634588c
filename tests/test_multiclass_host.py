"""Multi-class projection, host side (no GPU): argv of the projection CLI, the scene / frame unions of a multi-class
run, and the per-class tables built against one shared scene geometry -- equal to the single-class tables."""
import os

import numpy as np
import pytest
import torch


def test_projection_argv_one_and_several_classes():
    from beyond_fixed_forms_amd import cli
    p = cli._projection_parser()
    assert p.parse_args(["--config", "c.yaml", "--cls", "table"]).cls == ["table"]
    assert p.parse_args(["--config", "c.yaml", "--cls", "a", "--cls", "b c", "--cls", "d"]).cls == ["a", "b c", "d"]
    with pytest.raises(SystemExit):
        p.parse_args(["--config", "c.yaml"])


def test_refinement_argv_unchanged():
    from beyond_fixed_forms_amd import cli
    p = cli._parser("refinement")
    assert p.parse_args(["--config", "c.yaml", "--cls", "table"]).cls == "table"
    assert p.parse_args(["--config", "c.yaml", "--cls", "a", "--cls", "b"]).cls == "b"     # a single class, as before


def test_class_scene_union(tmp_path):
    from beyond_fixed_forms_amd.cli import class_scenes
    listing = {"a": ["scene0002_00", "scene0000_00"], "b": ["scene0001_00", "scene0002_00"], "c": ["scene0003_00"]}
    for c, ids in listing.items():
        (tmp_path / c).mkdir()
        for s in ids:
            (tmp_path / c / f"{s}.pth").write_bytes(b"")
        (tmp_path / c / "scene0009_01.pth").write_bytes(b"")          # not a *_00 scene (P:363)
    ids, per = class_scenes(str(tmp_path), ["b", "a", "c"])
    assert ids == ["scene0000_00", "scene0001_00", "scene0002_00", "scene0003_00"]
    assert per == [["a"], ["b"], ["b", "a"], ["c"]]                   # command-line order inside a scene


def test_frame_union():
    from beyond_fixed_forms_amd.scene import frame_union
    fr = lambda f: {"frame_id": f"{f}.jpg"}
    assert frame_union([[fr(3), fr(1)], [fr(1), fr(7)], []], ["0", "3", "10"]) == ["3", "1", "7", "0", "10"]
    assert frame_union([], []) == []


def _classes(scene):
    """Derived classes + the edge cases: > 32 masks on one frame, a frame outside the viewed set, an empty list,
    classes sharing frames."""
    from beyond_fixed_forms_amd.synthetic import derive_classes
    masks = derive_classes(scene, k=3, fraction=0.5, seed=3)
    f0 = scene.mask_2d[0]
    big = dict(f0, segmented_frame_masks=list(f0["segmented_frame_masks"]) * 9,
               confidences=torch.cat([f0["confidences"]] * 9), labels=["many"] * (9 * len(f0["labels"])))
    masks["many"] = [big] + scene.mask_2d[1:2]
    masks["off view"] = [dict(scene.mask_2d[1], frame_id="5.jpg")]      # frame 5 is a pose of its own, never viewed
    masks["empty"] = []
    masks["shared"] = scene.mask_2d[:2]
    return masks


def _tiny_scene():
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=5)
    scene.poses["5"] = scene.poses["10"] @ np.diag([1.0, 1.0, 1.0, 1.0])
    scene.depths["5"] = scene.depths["10"] * np.float32(0.5)
    return scene


def test_class_tables_equal_single_class_tables():
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.scene import prepare_class, prepare_geometry, prepare_scene
    from beyond_fixed_forms_amd.synthetic import class_scene
    scene = _tiny_scene()
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
    masks = _classes(scene)
    geom = prepare_geometry(scene, cfg, list(masks.values()), device="cpu", with_viewed=True)
    assert geom.viewed is None                            # counted on the GPU only
    assert geom.frame_ids[:len(dict.fromkeys(fr["frame_id"] for m in masks.values() for fr in m))][-1] == "5"
    assert any(len(fr["segmented_frame_masks"]) > 32 for fr in masks["many"])
    for cls, m in masks.items():
        ds = prepare_class(geom, m, cfg)
        ref = prepare_scene(class_scene(scene, m), cfg, device="cpu", with_viewed=False)
        assert ds.geometry is geom and ds.xyz is geom.xyz
        assert torch.equal(ds.xyz, ref.xyz) and torch.equal(ds.unsort, ref.unsort) and torch.equal(ds.perm, ref.perm)
        for k in ("n_frames", "n_mask_frames", "word_bits", "n_rows", "labels", "n_label_ids", "n_points", "nw"):
            assert getattr(ds, k) == getattr(ref, k), (cls, k)
        for k in ("inv_pose", "frame_mask", "frame_rowbase", "frame_nmask", "frame_flags", "run_start", "run_end",
                  "mask_run_offs", "view_mask_offs", "label_id", "conf"):
            a, b = getattr(ds, k), getattr(ref, k)
            assert a.dtype == b.dtype and torch.equal(a, b), (cls, k)
        assert ds.word_bits == (64 if cls == "many" else 32)
        assert not ds.frame_flags.any()
        # each depth_index names the same depth frame in the shared slots as in the class's own scene
        for f in range(ds.n_frames):
            assert torch.equal(geom.depth[int(ds.depth_index[f])], ref.depth[int(ref.depth_index[f])]), (cls, f)
    assert prepare_class(geom, [], cfg).n_rows == 0


def test_geometry_slots_cover_the_viewed_frames():
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.scene import prepare_geometry, viewed_frame_ids
    scene = _tiny_scene()
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
    masks = _classes(scene)
    geom = prepare_geometry(scene, cfg, list(masks.values()), device="cpu", with_viewed=True)
    viewed = viewed_frame_ids(scene.color_files, cfg.downsample_ratio)
    assert geom.n_viewed == len(viewed) and set(viewed) <= set(geom.frame_ids)
    assert len(set(geom.frame_ids)) == len(geom.frame_ids) == geom.depth.shape[0] == geom.inv_pose_host.shape[0]
    for k, f in enumerate(geom.frame_ids):
        assert np.array_equal(geom.inv_pose_host[k].reshape(4, 4), np.linalg.inv(scene.poses[f]))
        assert np.array_equal(geom.depth[k].numpy(), scene.depths[f].reshape(-1))
    plain = prepare_geometry(scene, cfg, list(masks.values()), device="cpu", with_viewed=False)
    assert plain.n_viewed == 0 and "5" in plain.frame_ids and set(plain.frame_ids) <= set(geom.frame_ids)


def test_hand_written_scene_against_hand_written_tables():
    """tests/hand_scene_case.py: the tables of a five-point scene with two mask lists, through prepare_scene (with and
    without the viewed frames) and through prepare_geometry + prepare_class, against tables written out by hand."""
    import hand_scene_case as case
    from beyond_fixed_forms_amd.scene import prepare_class, prepare_geometry, prepare_scene
    cfg = case.config()
    m32, m64 = case.masks()
    case.check_tables(prepare_scene(case.scene(m32), cfg, device="cpu"), "scene m32", None)
    case.check_tables(prepare_scene(case.scene(m32), cfg, device="cpu", with_viewed=False), "scene m32 without viewed", None)
    case.check_tables(prepare_scene(case.scene(m64), cfg, device="cpu"), "scene m64", None)
    geom = prepare_geometry(case.scene([]), cfg, [m32, m64], device="cpu")
    assert geom.viewed is None                            # counted on the GPU only
    case.check_tables(prepare_class(geom, m32, cfg), "class m32", geom)
    case.check_tables(prepare_class(geom, m64, cfg), "class m64", geom)
