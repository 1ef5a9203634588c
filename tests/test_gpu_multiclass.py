"""Multi-class projection on the GPU: the viewed-count sweep (bff_count_viewed) against the oracle and the fused sweep,
every class of project_scene_classes / project_classes_stream bit-identical to its own single-class run, and the
projection CLI with several --cls against single-class runs."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

from oracle import projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    return _lib.load()


def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


def same(got: dict, exp: dict):
    """Bit-identical masks (the empty form included), identical conf values and dtype, identical labels."""
    assert got["ins"].dtype == exp["ins"].dtype and tuple(got["ins"].shape) == tuple(exp["ins"].shape)
    assert torch.equal(got["ins"].cpu(), exp["ins"].cpu())
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"].cpu())
    assert list(got["final_class"]) == list(exp["final_class"])


def tiny_scene(seed=5, shape="tiny"):
    """A scene with one extra pose ("5") that no viewed frame is (downsample_ratio 10 keeps 0, 10, 20, ...)."""
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene(shape, seed=seed)
    scene.poses["5"] = scene.poses["10"].copy()
    scene.depths["5"] = scene.depths["10"] * np.float32(0.5)
    return scene


def edge_classes(scene, k=4, seed=3):
    """K >= 4 derived classes + > 32 masks on one frame, a mask frame outside the viewed set, an empty list, and two
    classes that share frames."""
    from beyond_fixed_forms_amd.synthetic import derive_classes
    masks = derive_classes(scene, k=k, fraction=0.5, seed=seed)
    f0 = scene.mask_2d[0]
    masks["many"] = [dict(f0, segmented_frame_masks=list(f0["segmented_frame_masks"]) * 9,
                          confidences=torch.cat([f0["confidences"]] * 9), labels=["many"] * (9 * len(f0["labels"])))] + \
        scene.mask_2d[1:3]
    masks["off view"] = [dict(scene.mask_2d[1], frame_id="5.jpg")] + scene.mask_2d[2:4]
    masks["empty"] = []
    masks["shared a"] = scene.mask_2d[:3]
    masks["shared b"] = [dict(fr, labels=["shared b"] * len(fr["labels"])) for fr in scene.mask_2d[1:4]]
    return masks


def sorted_to_caller(geom, viewed):
    return viewed[geom.unsort.long()] if geom.unsort is not None else viewed


# ------------------------------------------------------------------ the viewed-count sweep
@pytest.mark.parametrize("shape", ["tiny", "c1"])
def test_viewed_counts_match_oracle(lib, shape):
    from beyond_fixed_forms_amd.ingest import prepare_geometry_fast
    from beyond_fixed_forms_amd.scene import prepare_geometry
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene(shape, seed=21)
    cfg = cfg_for(scene)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _exp, dbg = pref.project_scene_ref(scene, cfg, return_debug=True)
    want = dbg["viewed_counts"].numpy().astype(np.int32)
    for geom in (prepare_geometry(scene, cfg, [scene.mask_2d], device=DEV),
                 prepare_geometry_fast(scene, cfg, [scene.mask_2d], device=DEV),
                 prepare_geometry(scene, cfg, [], device=DEV, sort_points=False)):
        torch.cuda.synchronize()
        assert np.array_equal(sorted_to_caller(geom, geom.viewed).cpu().numpy(), want)


def _count(geom, cfg, color_files, fpb):
    """bff_count_viewed over the viewed frames with a given frame tile."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.scene import viewed_frame_ids
    idx = np.array([geom.slot[f] for f in viewed_frame_ids(color_files, cfg.downsample_ratio)])
    out = torch.zeros(geom.n_points, dtype=torch.int32, device=DEV)
    _lib.count_viewed(geom.xyz, geom.n_points, torch.from_numpy(np.ascontiguousarray(geom.inv_pose_host[idx])).to(DEV),
                      geom.cam_intr, geom.sweep_depth, torch.from_numpy(idx.astype(np.int32)).to(DEV), geom.height,
                      geom.width, 0.08, out, tile_bounds=geom.tile_bounds, depth_size=geom.depth_size, frames_per_block=fpb)
    return out


@pytest.mark.parametrize("form", ["f32", "tiles_f32", "tiles_u16", "rows_u16", "resize_pass"])
def test_viewed_counts_match_fused_sweep_c2(lib, form):
    """A c2-sized cloud and image (200 k points, 968 x 1296): the counts equal the fused sweep's own viewed output in
    every depth form, and do not depend on the frame tile."""
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_geometry, prepare_scene
    from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth
    scene = make_scene("c2", seed=2, n_views=40, device=DEV)
    if form != "f32":
        scene = with_sensor_depth(scene)
    cfg = cfg_for(scene)
    env = {"tiles_f32": "f32", "tiles_u16": "u16", "rows_u16": "0"}.get(form)
    old = os.environ.get("BFF_DEPTH_TILES")
    try:
        if env is not None:
            os.environ["BFF_DEPTH_TILES"] = env
        resident = False if form == "resize_pass" else None
        ds = prepare_scene(scene, cfg, device=DEV, raw_depth_resident=resident)
        geom = prepare_geometry(scene, cfg, [scene.mask_2d], device=DEV, raw_depth_resident=resident)
    finally:
        if old is None:
            os.environ.pop("BFF_DEPTH_TILES", None)
        else:
            os.environ["BFF_DEPTH_TILES"] = old
    if form == "resize_pass":
        assert geom.depth_raw is None and geom.depth is not None
    elif form != "f32":
        assert geom.depth_raw is not None and (geom.depth_size is None) == (form == "rows_u16")
    ref = run_projection(ds, cfg, debug_out=True).debug["viewed_counts"]
    assert int(ref.max()) > 0
    assert torch.equal(sorted_to_caller(geom, geom.viewed), ref)
    for fpb in (1, 3, 8, 32):
        assert torch.equal(_count(geom, cfg, scene.color_files, fpb), geom.viewed), fpb


# ------------------------------------------------------------------ parity per class
def _expected(scene, masks, cfg, **kw):
    from beyond_fixed_forms_amd.projection import project_scene
    from beyond_fixed_forms_amd.synthetic import class_scene
    return {c: project_scene(class_scene(scene, m), cfg, DEV, **kw) for c, m in masks.items()}


@pytest.mark.parametrize("filt", ["ratio", "occurrence", "none"])
@pytest.mark.parametrize("debug_out", [False, True])
def test_classes_equal_single_class_runs(lib, filt, debug_out):
    from beyond_fixed_forms_amd.projection import project_scene_classes
    scene = tiny_scene()
    over = {"ratio": {}, "occurrence": dict(if_occurance_threshold=True),
            "none": dict(if_detected_ratio_threshold=False)}[filt]
    cfg = cfg_for(scene, **over)
    masks = edge_classes(scene)
    assert len(masks) >= 8 and any(len(fr["segmented_frame_masks"]) > 32 for fr in masks["many"])
    exp = _expected(scene, masks, cfg, debug_out=debug_out)
    got = project_scene_classes(scene, masks, cfg, DEV, debug_out=debug_out)
    assert list(got) == list(masks)
    for c in masks:
        same(got[c], exp[c])
    assert got["empty"]["final_class"] == []


def test_classes_c1_and_results(lib):
    """A c1 scene, derived classes (about 15 % of the frames each): results, groups and thresholds as single-class."""
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes
    from beyond_fixed_forms_amd.synthetic import class_scene, derive_classes, make_scene
    scene = make_scene("c1", seed=4, n_views=40, cut_masks=False)
    cfg = cfg_for(scene)
    masks = derive_classes(scene, k=6, fraction=0.15, seed=1)
    got = project_scene_classes(scene, masks, cfg, DEV, return_result=True)
    for c, m in masks.items():
        exp = project_scene(class_scene(scene, m), cfg, DEV, return_result=True)
        same(got[c].to_dict(), exp.to_dict())
        assert got[c].debug.get("thr") == exp.debug.get("thr") and got[c].debug["path"] == exp.debug["path"]


@pytest.mark.parametrize("how", ["resident_false", "resize_env", "tiles_u16"])
def test_classes_sensor_depth(lib, how):
    """Sensor-resolution depth: resident frames (per-point resize) and the separate resize pass, plain and native."""
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.synthetic import class_scene, with_sensor_depth
    scene = with_sensor_depth(tiny_scene(seed=8))
    cfg = cfg_for(scene)
    masks = edge_classes(scene, k=4, seed=9)
    env = {"resize_env": ("BFF_DEPTH_RESIZE_PASS", "1"), "tiles_u16": ("BFF_DEPTH_TILES", "u16")}.get(how)
    try:
        if env:
            os.environ[env[0]] = env[1]
        if how == "resident_false":
            got = project_scene_classes(scene, masks, cfg, DEV, debug_out=True, raw_depth_resident=False)
            exp = {c: run_projection(prepare_scene(class_scene(scene, m), cfg, DEV, raw_depth_resident=False), cfg,
                                     debug_out=True).to_dict() for c, m in masks.items()}
        else:
            got = project_scene_classes(scene, masks, cfg, DEV)
            exp = {c: project_scene(class_scene(scene, m), cfg, DEV) for c, m in masks.items()}
    finally:
        if env:
            os.environ.pop(env[0], None)
    for c in masks:
        same(got[c], exp[c])


def test_classes_stream_equals_project_stream(lib):
    """project_classes_stream over several scenes (classes listing different scenes) = project_stream per class."""
    from beyond_fixed_forms_amd.pipeline import project_classes_stream, project_stream
    from beyond_fixed_forms_amd.scene import SceneClasses
    from beyond_fixed_forms_amd.synthetic import class_scene
    scenes = [tiny_scene(seed=30 + s) for s in range(3)]
    cfg = cfg_for(scenes[0])
    per = [edge_classes(sc, k=4, seed=s) for s, sc in enumerate(scenes)]
    items = [(SceneClasses(sc, per[s]), [c for c in per[s] if not (s == 1 and c == "empty")]) for s, sc in enumerate(scenes)]
    got = {}
    project_classes_stream(items, cfg, DEV, lambda k, c, _s, res: got.__setitem__((k, c), res.to_dict()))
    assert list(got) == [(k, c) for k, (_s, cl) in enumerate(items) for c in cl]
    for cls in per[0]:
        ks = [k for k, (_s, cl) in enumerate(items) if cls in cl]
        exp = {}
        project_stream([class_scene(scenes[k], per[k][cls]) for k in ks], cfg, DEV,
                       lambda i, _s, res: exp.__setitem__(ks[i], res.to_dict()), with_stage1=False)
        for k in ks:
            same(got[(k, cls)], exp[k])


# ------------------------------------------------------------------ CLI
def _load_dir(d):
    out = {}
    for cls in sorted(os.listdir(d)):
        for f in sorted(os.listdir(os.path.join(d, cls))):
            out[(cls, f)] = torch.load(os.path.join(d, cls, f), map_location="cpu", weights_only=False)
    return out


def _run(tmp_path, classes, env):
    args = [sys.executable, os.path.join(ROOT, "tools", "projection_2d_to_3d.py"), "--config", str(tmp_path / "config.yaml")]
    for c in classes:
        args += ["--cls", c]
    r = subprocess.run(args, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_cli_several_classes(tmp_path):
    import shutil
    from beyond_fixed_forms_amd.synthetic import class_scene, derive_classes
    from test_gpu_cli import write_scene
    scenes = [tiny_scene(seed=70 + k) for k in range(3)]
    listing = {"a": [0, 1], "b chair": [1, 2], "c": [0, 1, 2]}
    for k, sc in enumerate(scenes):
        sc.scene_id = f"scene{70 + k:04d}_00"
        masks = derive_classes(sc, k=3, fraction=0.6, seed=k)
        for (cls, ks), m in zip(listing.items(), masks.values()):
            if k in ks:
                write_scene(tmp_path, class_scene(sc, [dict(fr, labels=[cls] * len(fr["labels"])) for fr in m]), cls)
    cfg = cfg_for(scenes[0], scene_2d_dir=str(tmp_path / "2d"), scene_npy_dir=str(tmp_path / "npy"),
                  mask_2d_dir=str(tmp_path / "m2d"), mask_3d_dir=str(tmp_path / "m3d"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BFF_GPUS"):
        env.pop(k, None)
    classes = list(listing)

    def take(tag):
        out = _load_dir(tmp_path / "m3d")
        ck = {c: yaml.safe_load((tmp_path / "checkpoints" / f"projection_2d_to_3d_checkpoint_{c}.yaml").read_text())
              for c in classes}
        shutil.move(tmp_path / "m3d", tmp_path / f"m3d_{tag}")
        shutil.move(tmp_path / "checkpoints", tmp_path / f"ck_{tag}")
        return out, ck

    log = _run(tmp_path, classes, env)
    for k, sc in enumerate(scenes):
        for c in classes:
            assert (f"Working on {sc.scene_id} class {c}" in log) == (k in listing[c])
    multi, ck_multi = take("multi")
    for c in classes:
        _run(tmp_path, [c], env)
    single, ck_single = take("single")
    assert sorted(multi) == sorted(single) and len(multi) == sum(len(v) for v in listing.values())
    for key in single:
        same(multi[key], single[key])
    assert ck_multi == ck_single and ck_multi["c"] == {sc.scene_id: True for sc in scenes}
    env2 = dict(env, BFF_GPUS="2", BFF_REHEARSE_ON_ONE_GPU="1", BFF_DEPTH_ON_DEVICE="1")
    _run(tmp_path, classes, env2)
    two, ck_two = take("two")
    assert sorted(two) == sorted(single)
    for key in single:
        same(two[key], single[key])
    assert ck_two == ck_single
