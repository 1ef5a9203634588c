"""Depth frames rendered from the cloud (bff_render_depth_u16) on the GPU: the kernel against its NumPy statement
(tests/render_depth_ref.py), texel for texel, and scenes without depth frames against the oracle fed with the frames the
reference would have read had the rendered frames been its depth PNGs.  Everything is compared for equality."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

import render_depth_ref as rd
from oracle import geom_fma, projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, N_PAD, F = 3000, 3072, 9
K33 = np.array([[64.0, 0.0, 34.5], [0.0, 64.0, 24.5], [0.0, 0.0, 1.0]])
CASES = [(50, 70, 1), (50, 70, 8), (50, 70, 16), (48, 64, 4)]            # (height, width, stride)


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def at_pixel(u, v, z):
    """A point (camera 0 = world coordinates) that projects to pixel (u, v) at depth z."""
    return [(u - K33[0, 2]) * z / 64.0, (v - K33[1, 2]) * z / 64.0, z]


@functools.lru_cache(maxsize=None)
def cloud():
    """3000 points, two full blocks and a ragged tail: a stack of 2000 points on one pixel with distinct depths (tight
    point tiles, which the frustum test culls in the frames that do not see them), ties, the crafted edge cases, and
    random points sorted along x; 9 poses, the first the identity, the last full of NaN."""
    rng = np.random.default_rng(7)
    stack = np.array([at_pixel(10, 10, 1.0 + 0.001 * i) for i in rng.permutation(2000)])        # 1000 .. 2999 mm, shuffled
    ties = np.array([at_pixel(20, 20, 2.0)] * 50 + [at_pixel(21, 20, 2.0)] * 10)                  # equal depths in a texel
    ulp = 2.0 ** -53                                                                               # of x in [0.5, 1)
    crafted = np.array([
        [0.1, 0.1, -1.0], [0.0, 0.0, 0.0], [0.2, 0.1, -0.0],                                        # c2 <= 0
        at_pixel(30, 5, 0.0004), at_pixel(31, 5, 0.0005), at_pixel(32, 5, 0.0006), at_pixel(33, 5, 0.0015),  # around 1/2 mm
        at_pixel(40, 5, 65.535), at_pixel(40, 30, 65.5354), at_pixel(5, 30, 65.5355), at_pixel(5, 40, 65.536),
        # u = width - 0.5 = 69.5 exactly (64 * 35 / 64 + 34.5) and one ulp of the pixel coordinate to either side
        [35.0 / 64 - 2 * ulp, 0.0, 1.0], [35.0 / 64, 0.0, 1.0], [35.0 / 64 + 2 * ulp, 0.0, 1.0],
        # the same around u = 63.5 for the 64-pixel image
        [29.0 / 64 - 2 * ulp, 0.1, 1.0], [29.0 / 64, 0.1, 1.0], [29.0 / 64 + 2 * ulp, 0.1, 1.0],
        [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, np.inf], [0.0, 0.0, np.nan], [-np.inf, 0.0, 2.0],
        [1e300, 0.0, 1.0], [0.0, 0.0, 1e-320],
    ])
    n_rand = N - len(stack) - len(ties) - len(crafted)
    rnd = np.stack([rng.uniform(-6, 6, n_rand), rng.uniform(-2, 2, n_rand), rng.uniform(0.8, 5, n_rand)], 1)
    rnd = rnd[np.argsort(rnd[:, 0])]
    xyz = np.concatenate([stack, ties, crafted, rnd])
    assert xyz.shape == (N, 3)
    inv = np.zeros((F, 16))
    inv[0] = np.eye(4).reshape(-1)
    for f in range(1, F - 1):
        a = rng.uniform(-1.2, 1.2)
        pose = np.eye(4)
        pose[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        pose[:3, 3] = rng.uniform(-1, 1, 3)
        inv[f] = np.linalg.inv(pose).reshape(-1)
    inv[F - 1] = np.nan
    soa = np.empty((3, N_PAD))
    soa[:, :N] = xyz.T
    soa[:, N:] = np.array([[0.0], [0.0], [0.5]])             # padding that would splat 500 mm at the image centre if read
    return xyz, inv, soa, len(stack) + len(ties)


@functools.lru_cache(maxsize=None)
def reference(h, w, stride):
    xyz, inv, _, _ = cloud()
    dh, dw = rd.rendered_size(h, w, stride)
    counts = []
    return rd.render_depth_ref(xyz, inv, K33, h, w, dh, dw, counts), np.stack(counts)


def test_crafted_points_are_what_they_claim():
    """On the reference: the half-pixel points straddle the image border, the range ends straddle 1 and 65535 mm."""
    xyz, inv, _, c0 = cloud()
    pts, pix, _ = geom_fma.view(xyz, inv[0].reshape(4, 4), K33, np.zeros((1, 1), np.float32))
    assert pix[c0 + 11:c0 + 14, 0].tolist() == [69, 70, 70] and pix[c0 + 14:c0 + 17, 0].tolist() == [63, 64, 64]
    mm = np.rint(pts[c0 + 3:c0 + 11, 2] * 1000.0)
    assert mm.tolist() == [0, 0, 1, 2, 65535, 65535, 65536, 65536]
    assert (pix[:2000] == [10, 10]).all() and np.unique(np.rint(pts[:2000, 2] * 1000)).size == 2000
    ref, counts = reference(50, 70, 1)
    assert ref[0, 10, 10] == 1000 and counts[0, 10, 10] == 2000 and ref[0, 20, 20] == 2000 and counts[0, 20, 20] == 50
    assert ref[0, 24, 69] == 1000 and ref[0, 5, 32] == 1 and ref[0, 5, 33] == 2 and ref[0, 5, 30] == 0 and ref[0, 5, 31] == 0
    assert ref[0, 5, 40] == 65535 and ref[0, 30, 40] == 65535 and ref[0, 30, 5] == 0 and ref[0, 40, 5] == 0
    assert not ref[F - 1].any()                                          # the NaN pose sees nothing
    assert ref[0, 24, 34] != 500 and ref[0, 24, 35] != 500 and ref[0, 25, 34] != 500 and ref[0, 25, 35] != 500


def render(lib, h, w, stride, bounds, **kw):
    _, inv, soa, _ = cloud()
    dh, dw = rd.rendered_size(h, w, stride)
    xyz = torch.from_numpy(soa).to(DEV)
    tb = lib.point_tile_bounds(xyz, N) if bounds else None
    out = lib.render_depth(xyz, N, torch.from_numpy(inv).to(DEV), K33, h, w, dh, dw, tile_bounds=tb, **kw)
    assert out.dtype == torch.int16 and tuple(out.shape) == (F, dh, dw)
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("h,w,stride", CASES)
def test_kernel_equals_reference(lib, h, w, stride):
    ref, counts = reference(h, w, stride)
    assert (counts >= 2).any() and (counts == 0).any()                   # both branches: contested texels and empty ones
    assert ((ref == 0) == (counts == 0)).all()
    got = render(lib, h, w, stride, bounds=False)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:10]
    culled = render(lib, h, w, stride, bounds=True)
    assert np.array_equal(culled, ref), np.argwhere(culled != ref)[:10]  # same frames with and without the culling table
    assert render(lib, h, w, stride, bounds=True).tobytes() == culled.tobytes()    # and on every run


def test_stack_tiles_are_in_view_of_some_frames_only():
    """The first point tiles (the stack on one pixel: boxes a few centimetres wide) lie inside the image in some of the
    first eight frames and wholly outside in others, so inside one frame tile the culling decides differently per frame."""
    xyz, inv, _, _ = cloud()
    seen = [len(rd.splats(xyz[:256], inv[f], K33, 50, 70, 50, 70)[0]) for f in range(8)]
    assert any(n == 256 for n in seen) and any(n == 0 for n in seen), seen


@pytest.mark.parametrize("tile", [2, 3, 8, 9, 32])
@pytest.mark.parametrize("h,w,stride", [(50, 70, 8), (48, 64, 4)])
def test_frame_tiles_equal_reference(lib, h, w, stride, tile):
    """The 9 frames with a block visiting several of them: one full culling group of 8 and one frame over (tiles 8, 9,
    32), ragged tiles (2, 3), with and without the culling table.  The library's own choice at this size is 1."""
    ref, _ = reference(h, w, stride)
    for bounds in (False, True):
        got = render(lib, h, w, stride, bounds, frames_per_block=tile)
        assert np.array_equal(got, ref), (bounds, np.argwhere(got != ref)[:10])


def test_scratch_smaller_than_the_frames(lib):
    """A scratch that holds 4 of the 9 frames: three runs (4, 4, 1), the same frames."""
    ref, _ = reference(50, 70, 8)
    assert np.array_equal(render(lib, 50, 70, 8, True, scratch_texels=4 * 7 * 9 + 5), ref)
    assert np.array_equal(render(lib, 50, 70, 8, False, scratch_texels=1, frames_per_block=8), ref)     # frame by frame


def test_empty_inputs_return_cleanly(lib):
    _, inv, soa, _ = cloud()
    xyz = torch.from_numpy(soa).to(DEV)
    none = lib.render_depth(xyz, N, torch.zeros((0, 16), dtype=torch.float64, device=DEV), K33, 50, 70, 7, 9)
    assert tuple(none.shape) == (0, 7, 9)
    out = lib.render_depth(xyz, 0, torch.from_numpy(inv).to(DEV), K33, 50, 70, 7, 9)     # no points: "no depth" everywhere
    torch.cuda.synchronize()
    assert tuple(out.shape) == (F, 7, 9) and int(out.count_nonzero()) == 0


# ------------------------------------------------------------------ scenes without depth frames against the oracle
FILTERS = {"ratio": {}, "occurrence": dict(if_occurance_threshold=True), "none": dict(if_detected_ratio_threshold=False)}
SEED = {4: 74, 8: 70}                                                    # chosen on the CPU: the oracle keeps instances


def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


@functools.lru_cache(maxsize=None)
def tiny(stride):
    """(the scene without depth, the same scene with the depth images the reference would read)."""
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=SEED[stride])
    return rd.without_depth(scene), rd.scene_with_rendered_depth(scene, stride)


@functools.lru_cache(maxsize=None)
def expected(stride, filt):
    ref_scene = tiny(stride)[1]
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
@pytest.mark.parametrize("stride", [4, 8])
def test_scene_equals_oracle(lib, stride, filt):
    """project_scene on a scene that has no depth frames: the one-call path behind prepare_scene_fast, and debug_out=True
    behind prepare_scene."""
    from beyond_fixed_forms_amd.projection import project_scene
    scene = tiny(stride)[0]
    assert scene.depths == {} and scene.depths_raw is None
    cfg = cfg_for(scene, depth_from_cloud=stride, **FILTERS[filt])
    exp = expected(stride, filt)
    same(project_scene(scene, cfg, DEV), exp)
    same(project_scene(scene, cfg, DEV, debug_out=True), exp)


def test_key_off_still_needs_depth(lib):
    from beyond_fixed_forms_amd.projection import project_scene
    scene = tiny(4)[0]
    with pytest.raises(KeyError):
        project_scene(scene, cfg_for(scene), DEV, debug_out=True)


@pytest.mark.parametrize("form", ["f32", "u16", "0", "resize_pass"])
def test_scene_depth_layouts(lib, form, monkeypatch):
    """The rendered frames go where the PNGs' frames go: resident in either tile form or row-major, or through the
    separate scale + resize pass -- prepared by scene.py and by ingest.py."""
    from beyond_fixed_forms_amd.ingest import prepare_scene_fast
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene
    stride = 4
    scene = tiny(stride)[0]
    cfg = cfg_for(scene, depth_from_cloud=stride)
    if form == "resize_pass":
        monkeypatch.setenv("BFF_DEPTH_RESIZE_PASS", "1")
    else:
        monkeypatch.setenv("BFF_DEPTH_TILES", form)
    dh, dw = rd.rendered_size(scene.height, scene.width, stride)
    for prep in (prepare_scene, prepare_scene_fast):
        ds = prep(scene, cfg, device=DEV)
        if form == "resize_pass":
            assert ds.depth_raw is None and tuple(ds.depth.shape[1:]) == (scene.height * scene.width,)
        elif form == "0":
            assert ds.depth is None and ds.depth_size is None and tuple(ds.depth_raw.shape[1:]) == (dh, dw)
        else:
            assert ds.depth is None and ds.depth_size == (dh, dw)
            assert ds.depth_raw.dtype == (torch.float32 if form == "f32" else torch.int16)
        same(run_projection(ds, cfg).to_dict(), expected(stride, "ratio"))
        if form == "0":                                                  # the resident frames are the reference's, texel for texel
            ids = list(dict.fromkeys([fr["frame_id"][:-4] for fr in scene.mask_2d if len(fr["labels"])] +
                                     pref.viewed_frame_ids(scene.color_files, cfg.downsample_ratio)))
            inv = np.stack([np.linalg.inv(scene.poses[f]) for f in ids])
            ref = rd.render_depth_ref(scene.points, inv, scene.cam_intr[:3, :3], scene.height, scene.width, dh, dw)
            assert np.array_equal(ds.depth_raw.cpu().numpy().view(np.uint16), ref)


@pytest.mark.parametrize("debug_out", [False, True])
def test_two_classes_render_once(lib, debug_out, monkeypatch):
    """project_scene_classes: depth lives in the shared geometry, so it is rendered once per scene; every class equals
    its single-class run and the oracle."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes
    from beyond_fixed_forms_amd.synthetic import class_scene
    stride = 8
    scene, ref_scene = tiny(stride)
    cfg = cfg_for(scene, depth_from_cloud=stride)
    masks = {"table": scene.mask_2d,
             "chair": [dict(fr, labels=["chair"] * len(fr["labels"])) for fr in scene.mask_2d[1:]]}
    calls = []
    real = _lib.render_depth
    monkeypatch.setattr(_lib, "render_depth", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = project_scene_classes(scene, masks, cfg, DEV, debug_out=debug_out)
    assert len(calls) == 1
    for c, m in masks.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp = pref.project_scene_ref(class_scene(ref_scene, m), cfg_for(ref_scene))
        assert len(exp["final_class"]) >= 1
        same(got[c], exp)
        same(got[c], project_scene(class_scene(scene, m), cfg, DEV, debug_out=debug_out))


@pytest.mark.parametrize("stride", [1, 4])
def test_occlusion_by_hand(lib, stride):
    """A near plane in front of a far one and a full-image mask: the row holds the near points and exactly the far points
    outside the near plane's silhouette (at a coarser stride: away from the edge the bilinear resize blurs), and equals
    the reference's row everywhere."""
    from beyond_fixed_forms_amd.projection import project_scene
    scene, _, _ = rd.two_plane_scene()
    over = dict(min_aggragated_masks=1, if_detected_ratio_threshold=False)
    got = project_scene(scene, cfg_for(scene, depth_from_cloud=stride, **over), DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pref.project_scene_ref(rd.scene_with_rendered_depth(scene, stride), cfg_for(scene, **over))
    same(got, exp)
    assert got["ins"].shape[0] == 1
    row, (exp_row, sure) = got["ins"][0].cpu().numpy(), rd.hand_row(stride)
    assert np.array_equal(row[sure], exp_row[sure]) and (stride != 1 or sure.all())


# ------------------------------------------------------------------ the stage scripts on a tree without depth/
def test_stage_scripts_without_depth_folder(tmp_path):
    from beyond_fixed_forms_amd.labels import SCANNET200_LABELS
    from beyond_fixed_forms_amd.synthetic import class_scene, make_text_bank
    from oracle import refinement_ref as rref
    from oracle.make_golden_shared import bank_encoder
    stride = 4
    scene, ref_scene = tiny(stride)
    masks = {"table": scene.mask_2d,
             "chair": [dict(fr, labels=["chair"] * len(fr["labels"])) for fr in scene.mask_2d[1:]]}
    rd.write_scene_without_depth(tmp_path, scene, masks)
    (tmp_path / "stage1").mkdir()
    torch.save(scene.stage1, tmp_path / "stage1" / f"{scene.scene_id}.pth")
    assert not (tmp_path / "2d" / scene.scene_id / "depth").exists()
    cfg = cfg_for(scene, depth_from_cloud=stride, scene_2d_dir=str(tmp_path / "2d"), scene_npy_dir=str(tmp_path / "npy"),
                  mask_2d_dir=str(tmp_path / "m2d"), mask_3d_dir=str(tmp_path / "m3d"),
                  stage_1_results_dir=str(tmp_path / "stage1"), final_output_dir=str(tmp_path / "final"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    bank, index = make_text_bank(64, seed=5)
    torch.save({lab: bank[i].float() for i, lab in enumerate(SCANNET200_LABELS)} | {"table": bank[index["table"]].float()},
               tmp_path / "text.pt")
    env = dict(os.environ, BFF_TEXT_EMBEDDINGS=str(tmp_path / "text.pt"))

    def run(script, *classes):
        argv = [sys.executable, os.path.join(ROOT, "tools", script), "--config", str(tmp_path / "config.yaml")]
        for c in classes:
            argv += ["--cls", c]
        r = subprocess.run(argv, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]

    def oracle(cls):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return pref.project_scene_ref(class_scene(ref_scene, masks[cls]), cfg)

    def check(cls):
        exp = oracle(cls)
        got = torch.load(tmp_path / "m3d" / cls / f"{scene.scene_id}.pth", map_location="cpu", weights_only=False)
        assert len(exp["final_class"]) >= 1
        same(got, exp)
        return exp

    run("projection_2d_to_3d.py", "table")                               # one --cls: the reference's run
    exp = check("table")
    run("refinement.py", "table")
    fexp = rref.refine_class_ref([(scene.scene_id, scene.stage1, exp)], cfg, "table", bank_encoder(bank.float(), index))
    got = torch.load(tmp_path / "final" / "table" / f"{scene.scene_id}.pth", map_location="cpu", weights_only=False)
    e = fexp[scene.scene_id]
    assert torch.equal(got["ins"], e["ins"]) and torch.equal(got["conf"], e["conf"]) and got["final_class"] == e["final_class"]
    os.remove(tmp_path / "m3d" / "table" / f"{scene.scene_id}.pth")
    run("projection_2d_to_3d.py", "table", "chair")                      # several: the scene is read and rendered once
    check("table")
    check("chair")
