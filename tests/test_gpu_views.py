"""The views of 3-D instances on the device against tests/views_ref.py, element for element.

1. bff_instance_views on synthetic tables (tests/vis_table_synth.py; no geometry): word ends, one sweep block exactly,
   stride > nw, empty and full rows, a slot without a pair, rows that share all points, a row beyond the kernel's LDS
   budget, the corners of the largest image, hundreds of points on one pixel.  Outputs are pre-filled and followed by a
   guard tail: every element is overwritten, the tail is not; the counts also equal bff_cross_popcount.
2. bff_select_views on synthetic counts and boxes: pure ties, descending and ascending counts, T below and above F, the
   hand-computed crops of tests/test_views_host.py.
3. views.scene_views on the generator's c1 scene and the hand scene against the statement fed a table restated from
   oracle.projection_ref's projection and visibility: all frames, a permuted subset, slot groups forced by
   BFF_VIS_TABLE_MAX_MB, rendered depth, and a geometry whose own table is reused.
4. tools/select_views_3d.py on a small scene tree."""
import faulthandler
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch
import yaml

import hand_scene_case as hs
import views_ref as wr
import vis_table_synth as vs
from oracle import projection_ref as pref
from test_views_host import CROP_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEM_LIMIT_S = 120                # a test item that is still running by then has hung: the process ends with a traceback
FILL, TAIL = -12345, 64
NAMES = ("area", "visible", "boxes", "top", "top_visible", "crops")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(ITEM_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def to_dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def guarded(n, dtype=torch.int32):
    """n elements to be written, pre-filled, and a tail that must stay as it is."""
    return torch.full((n + TAIL,), FILL, dtype=dtype, device=DEV)


# ------------------------------------------------------------------ 1. bff_instance_views on synthetic tables
def crafted_rows(rng, k, n):
    """bool [k][n]: all ones, empty, only bits of the last (partial) word, one random row twice, then random densities."""
    last = np.zeros(n, bool)
    last[(n - 1) // 64 * 64:] = rng.random(n - (n - 1) // 64 * 64) < 0.7
    last[n - 1] = True
    twin = rng.random(n) < 0.4
    head = [np.ones(n, bool), np.zeros(n, bool), last, twin, twin.copy()]
    rest = [rng.random(n) < d for d in rng.choice([0.01, 0.1, 0.5, 0.9], size=max(0, k - len(head)))]
    return np.stack((head + rest)[:k])


def run_instance_views(lib, bits, table, n, h, w):
    """The kernel on guarded buffers -> (visible, box) as arrays, after the overwrite / tail / cross-count checks."""
    mask, off, pix = table
    k, f, nw = bits.shape[0], mask.shape[0], (n + 63) // 64
    assert mask.shape[1] == lib.visibility_words(n) >= nw
    rows = to_dev(wr.pack(bits))
    dmask, doff, dpix = to_dev(mask), to_dev(off), to_dev(pix if pix.size else np.zeros(1, np.uint32))
    visible, box = guarded(k * f), guarded(k * f * 4)
    lib.call("bff_instance_views", lib._ptr(rows), k, nw, lib._ptr(dmask), lib._ptr(doff), lib._ptr(dpix), f, mask.shape[1],
             int(pix.size), h, w, lib._ptr(visible), lib._ptr(box))
    torch.cuda.synchronize()
    assert (visible[k * f:] == FILL).all() and (box[k * f * 4:] == FILL).all(), "the guard tail was written"
    got_v, got_b = visible[:k * f].reshape(k, f), box[:k * f * 4].reshape(k, f, 4)
    exp_v, exp_b, _area = wr.instance_views(wr.pack(bits), mask, off, pix, n, h, w)
    got_b_np = got_b.cpu().numpy()
    # every element was overwritten: FILL is no count, and no coordinate of a box or of the sentinel box
    assert (got_v != FILL).all() and (got_b != FILL).all()
    assert np.array_equal(got_v.cpu().numpy(), exp_v), "visible"
    assert np.array_equal(got_b_np, exp_b), "box"
    cross = lib.cross_popcount(rows, dmask[:, :nw].contiguous())
    assert torch.equal(cross, got_v), "visible != cross_popcount(rows, vis_mask)"
    # the wrapper: the same through views.instance_views
    from beyond_fixed_forms_amd import views
    v2, b2 = views.instance_views((dmask, doff, dpix, int(pix.size)), rows, n, h, w)
    assert v2.dtype == b2.dtype == torch.int32 and torch.equal(v2, got_v) and torch.equal(b2, got_b)
    return exp_v, exp_b


KF = [(1, 1), (2, 3), (64, 17), (65, 3)]
DENSITIES = {1: [0.5], 3: [0.3, 0.0, 1.0], 17: [0.0, 1.0] + [0.02, 0.2, 0.6] * 5}


@pytest.mark.parametrize("k,f", KF)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_instance_views_on_synthetic_tables(lib, n, k, f):
    rng = np.random.default_rng(1000 * n + 10 * k + f)
    h, w = 37, 41
    table = vs.synthetic_table(n, DENSITIES[f], h, w, rng, hot_share=0.1, hot_pixels=6)
    bits = crafted_rows(rng, k, n)
    vis, box = run_instance_views(lib, bits, table, n, h, w)
    nw, stride = (n + 63) // 64, table[0].shape[1]
    assert stride - nw == {1: 15, 63: 15, 64: 15, 65: 14, 1023: 0, 1024: 0, 1025: 15, 4097: 15}[n]
    if f >= 3:
        dead = DENSITIES[f].index(0.0)
        assert not table[0][dead].any() and not vis[:, dead].any() and (box[:, dead] == [w, h, -1, -1]).all()
        full = DENSITIES[f].index(1.0)
        assert vis[0, full] == n                                     # the row of all ones in the slot that sees every point
    if k >= 2:
        assert not vis[1].any() and (box[1] == [w, h, -1, -1]).all()       # the empty row
    if k >= 64:
        assert np.array_equal(vis[3], vis[4]) and np.array_equal(box[3], box[4])     # two instances sharing all points
        if f >= 3:
            assert vis[2, DENSITIES[f].index(1.0)] == bits[2].sum() > 0 and not bits[2, :(n - 1) // 64 * 64].any()


def test_instance_views_beyond_the_lds_budget(lib):
    budget = lib.instance_views_lds_words()
    assert budget == lib.load().bff_instance_views_lds_words() and 64 <= budget <= 8192
    n = 64 * budget + 1                                              # the smallest cloud a row of which can exceed the budget
    nw = budget + 1
    rng = np.random.default_rng(5)
    h, w = 61, 67
    table = vs.synthetic_table(n, [0.3, 0.0, 1.0], h, w, rng, hot_share=0.05, hot_pixels=5)
    sparse = np.zeros((nw, 64), bool)
    sparse[np.arange(nw), rng.integers(0, 64, nw)] = True           # one bit in every word: budget + 1 non-zero words
    sparse = sparse.reshape(-1)[:n].copy()
    sparse[n - 1] = True
    fits = sparse.copy()
    fits[:64] = False                                                # exactly `budget` non-zero words: the last row that fits
    bits = np.stack([np.ones(n, bool), sparse, fits, np.zeros(n, bool), rng.random(n) < 0.001])
    words = (wr.pack(bits) != 0).sum(axis=1)
    assert words.tolist()[:4] == [budget + 1, budget + 1, budget, 0] and words[4] <= budget
    vis, _box = run_instance_views(lib, bits, table, n, h, w)
    assert vis[0, 2] == n and vis[1, 2] == sparse.sum() and vis[2, 2] == fits.sum() == sparse.sum() - 1


def test_instance_views_largest_image_and_crowded_pixel(lib):
    rng = np.random.default_rng(9)
    n, side = 1025, 32767
    table = vs.synthetic_table(n, [1.0, 0.5, 0.0], side, side, rng, hot_share=0.5, hot_pixels=4)
    u, v = (table[2] & 0xffff).astype(np.int64), (table[2] >> 16).astype(np.int64)
    assert ((u == 0) & (v == 0)).any() and ((u == side - 1) & (v == side - 1)).any()
    bits = crafted_rows(rng, 6, n)
    _vis, box = run_instance_views(lib, bits, table, n, side, side)
    assert box[0, 0].tolist() == [0, 0, side - 1, side - 1] and (box[:, 2] == [side, side, -1, -1]).all()
    # several hundred points on one pixel: 4097 points over 2 x 3 pixels
    n, h, w = 4097, 2, 3
    table = vs.synthetic_table(n, [1.0, 0.3], h, w, rng, hot_share=0.0, hot_pixels=4)
    assert np.bincount((table[2][:n] >> 16) * w + (table[2][:n] & 0xffff)).min() > 300
    vis, box = run_instance_views(lib, crafted_rows(rng, 7, n), table, n, h, w)
    assert box[0, 0].tolist() == [0, 0, w - 1, h - 1] and vis[0, 0] == n


# ------------------------------------------------------------------ 2. bff_select_views
def synthetic_counts(rng, k, f, h, w):
    """visible int32 [k][f]: all equal, strictly descending, strictly ascending, all zero, then random with many ties;
    box: a random valid box where a point is seen, the sentinel elsewhere."""
    visible = rng.integers(0, 6, (k, f)).astype(np.int32)
    kinds = [np.full(f, 7), np.arange(f, 0, -1) + 2, np.arange(f) + 1, np.zeros(f)]
    for i, row in enumerate(kinds[:k]):
        visible[i] = row
    if k > 8:
        visible[8] = rng.integers(0, 100000, f)
    u0, v0 = rng.integers(0, w, (k, f)), rng.integers(0, h, (k, f))
    box = np.stack([u0, v0, rng.integers(u0, w), rng.integers(v0, h)], axis=-1).astype(np.int32)
    box[visible == 0] = [w, h, -1, -1]
    return visible, box


def run_select_views(lib, visible, box, h, w, top_k, min_points, levels, expand):
    k, f = visible.shape
    top, tv, crops = guarded(k * top_k), guarded(k * top_k), guarded(k * top_k * levels * 4)
    dvis, dbox = to_dev(visible), to_dev(box)                       # named: they must outlive the launch
    lib.call("bff_select_views", lib._ptr(dvis), lib._ptr(dbox), k, f, h, w, top_k, min_points, levels,
             float(expand), lib._ptr(top), lib._ptr(tv), lib._ptr(crops))
    torch.cuda.synchronize()
    sizes = (k * top_k, k * top_k, k * top_k * levels * 4)
    for buf, size, what in zip((top, tv, crops), sizes, ("top", "top_visible", "crops")):
        assert (buf[size:] == FILL).all(), f"{what}: the guard tail was written"
        assert (buf[:size] != FILL).all(), f"{what}: an element was not written"
    exp = wr.select_views(visible, box, h, w, top_k, min_points, levels, expand)
    got = (top[:sizes[0]].reshape(k, top_k), tv[:sizes[1]].reshape(k, top_k), crops[:sizes[2]].reshape(k, top_k, levels, 4))
    for g, e, what in zip(got, exp, ("top", "top_visible", "crops")):
        assert np.array_equal(g.cpu().numpy(), e), what
    from beyond_fixed_forms_amd import views
    again = views.select_views(to_dev(visible), to_dev(box), h, w, top_k, min_points, levels, expand)
    for g, a in zip(got, again):
        assert a.dtype == torch.int32 and torch.equal(g, a)
    return exp


@pytest.mark.parametrize("top_k", [1, 5, 64])
@pytest.mark.parametrize("f", [1, 63, 64, 65, 300])
def test_select_views_on_synthetic_counts(lib, f, top_k):
    rng = np.random.default_rng(100 * f + top_k)
    h, w = 480, 640
    for k in (1, 65):
        visible, box = synthetic_counts(rng, k, f, h, w)
        top, tv, _ = run_select_views(lib, visible, box, h, w, top_k, 1, 3, 0.1)
        t = min(top_k, f)
        assert top[0, :t].tolist() == list(range(t)) and (tv[0, :t] == 7).all()                 # the pure tie: slot order
        assert (top[0, t:] == -1).all() and (tv[0, t:] == 0).all()
        if k > 3:
            assert top[1, :t].tolist() == list(range(t)) and top[2, :t].tolist() == list(range(f - 1, f - 1 - t, -1))
            assert (top[3] == -1).all()
        run_select_views(lib, visible, box, h, w, top_k, 4, 2, 0.25)                             # min_points cuts candidates


@pytest.mark.parametrize("case", range(len(CROP_CASES)))
def test_select_views_crops_by_hand(lib, case):
    b, h, w, r, want = CROP_CASES[case]
    visible = np.array([[0, 6, 0]], np.int32)
    box = np.array([[[w, h, -1, -1], list(b), [w, h, -1, -1]]], np.int32)
    top, tv, crops = run_select_views(lib, visible, box, h, w, 2, 1, 3, r)
    assert top.tolist() == [[1, -1]] and tv.tolist() == [[6, 0]] and crops[0, 0].tolist() == [list(c) for c in want]


def test_no_slot_and_no_instance(lib):
    from beyond_fixed_forms_amd import views
    i32 = torch.int32
    top, tv, crops = views.select_views(torch.zeros((2, 0), dtype=i32, device=DEV), torch.zeros((2, 0, 4), dtype=i32, device=DEV),
                                        8, 9, 3, 1, 2, 0.1)
    assert (top == -1).all() and not tv.any() and (crops.cpu() == torch.tensor([9, 8, -1, -1], dtype=i32)).all()
    assert crops.shape == (2, 3, 2, 4)
    top, tv, crops = views.select_views(torch.zeros((0, 5), dtype=i32, device=DEV), torch.zeros((0, 5, 4), dtype=i32, device=DEV),
                                        8, 9, 3, 1, 2, 0.1)
    assert top.shape == (0, 3) and tv.shape == (0, 3) and crops.shape == (0, 3, 2, 4)


# ------------------------------------------------------------------ 3. geometry end to end
def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


def object_instances(scene, seed=0):
    """Instances of a generator scene in the ORIGINAL point order, bool [K][n]: every cuboid, the room, an empty row, one
    cuboid twice, a union of two, and a random sprinkle."""
    obj = np.asarray(scene.point_object)
    rng = np.random.default_rng(seed)
    ids = [k for k in np.unique(obj) if k >= 0]
    rows = [obj == k for k in ids] + [obj == -1, np.zeros(obj.size, bool), obj == ids[0], (obj == ids[0]) | (obj == ids[1]),
                                     rng.random(obj.size) < 0.01]
    return np.stack(rows)


def as_result(bits):
    rows = to_dev(wr.pack(bits)) if bits.shape[0] else None
    return types.SimpleNamespace(rows=rows, conf=[0.5] * bits.shape[0], final_class=["x"] * bits.shape[0])


def oracle_table(points_sorted, poses, k33, depths):
    """The table of the sorted cloud over the given frames from the oracle's projection and visibility helpers."""
    cloud_h = pref.homogeneous_cloud(points_sorted)
    n = points_sorted.shape[0]
    vis, u, v = [], [], []
    for pose, depth in zip(poses, depths):
        pts = pref.world_to_camera(cloud_h, pose)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pix = pref.project_to_pixels(pts, k33)
        vis.append(pref.visibility(pts, pix, depth, pref.DEPTH_THRESH))
        u.append(pix[:, 0])
        v.append(pix[:, 1])
    return wr.table_from_dense(np.stack(vis), np.stack(u), np.stack(v), (n + 1023) // 1024 * 16)


def expected_views(scene, geom, bits, frame_keys, depths, cfg):
    from beyond_fixed_forms_amd import views
    perm = geom.perm.cpu().numpy().astype(np.int64)
    pts = np.asarray(scene.points)[perm]
    k33 = np.asarray(scene.cam_intr)[:3, :3]
    table = oracle_table(pts, [np.asarray(scene.poses[f]) for f in frame_keys], k33, depths)
    c = views.check_config(cfg)
    exp = wr.scene_views(wr.pack(bits[:, perm]), *table, pts.shape[0], geom.height, geom.width, c["top_k"], c["min_points"],
                         c["levels"], c["expand"])
    exp["n_pairs"] = int(table[2].size)
    return exp


def assert_views(got, exp, frame_keys, h, w):
    assert list(got) == list(NAMES) + ["frame_ids", "height", "width", "depth_thresh"]
    assert got["frame_ids"] == [f"{f}.jpg" for f in frame_keys]
    assert (got["height"], got["width"], got["depth_thresh"]) == (h, w, 0.08)
    for name in NAMES:
        g = got[name]
        assert torch.is_tensor(g) and not g.is_cuda and g.dtype == torch.int32, name
        assert tuple(g.shape) == exp[name].shape and np.array_equal(g.numpy(), exp[name]), name


def same_views(a, b):
    assert list(a) == list(b)
    for name in a:
        assert torch.equal(a[name], b[name]) if torch.is_tensor(a[name]) else a[name] == b[name], name


@pytest.fixture(scope="module")
def c1(lib):
    from beyond_fixed_forms_amd.scene import geometry_for_depth_frames
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("c1", seed=0)
    cfg = cfg_for(scene)
    frames = list(scene.poses)
    geom = geometry_for_depth_frames(scene, cfg, [f"{f}.jpg" for f in frames], DEV)
    bits = object_instances(scene)
    exp = expected_views(scene, geom, bits, frames, [scene.depths[f] for f in frames], cfg)
    n_pairs = exp.pop("n_pairs")
    for a in exp.values():
        a.setflags(write=False)
    return types.SimpleNamespace(scene=scene, cfg=cfg, frames=frames, geom=geom, bits=bits, exp=exp, n_pairs=n_pairs)


def test_scene_views_all_frames(lib, c1):
    from beyond_fixed_forms_amd import views
    assert c1.geom.frame_ids == c1.frames and c1.geom.sweep_depth is not None and c1.geom.viewed is None
    before = lib.visibility_builds()
    got = views.scene_views(c1.geom, as_result(c1.bits), c1.cfg)
    assert lib.visibility_builds() == before + 1                     # one table over all frames
    assert_views(got, c1.exp, c1.frames, c1.scene.height, c1.scene.width)
    exp = c1.exp
    k = c1.bits.shape[0]
    assert exp["area"].tolist() == c1.bits.sum(axis=1).tolist() and (exp["visible"] > 50).any()
    empty = k - 4
    assert exp["area"][empty] == 0 and (exp["top"][empty] == -1).all() and (exp["crops"][empty] == [640, 480, -1, -1]).all()
    assert np.array_equal(exp["visible"][0], exp["visible"][k - 3]) and (exp["top"][:, 0] >= 0).sum() >= k // 2
    assert (exp["crops"][..., 2, :] != exp["crops"][..., 0, :]).any()           # some crop grows with its level
    assert "_vis_tables" not in c1.geom.__dict__                     # the projection's bookkeeping is left alone


def test_scene_views_subset_in_permuted_order(lib, c1):
    from beyond_fixed_forms_amd import views
    pick = [7, 2, 9, 0, 4]
    frames = [c1.frames[i] for i in pick]
    got = views.scene_views(c1.geom, as_result(c1.bits), c1.cfg, frame_ids=[f"{f}.jpg" for f in frames])
    assert got["frame_ids"] == [f"{f}.jpg" for f in frames]
    assert np.array_equal(got["visible"].numpy(), c1.exp["visible"][:, pick])
    assert np.array_equal(got["boxes"].numpy(), c1.exp["boxes"][:, pick])
    sub = wr.select_views(c1.exp["visible"][:, pick], c1.exp["boxes"][:, pick], 480, 640, 5, 1, 3, 0.1)
    for name, e in zip(("top", "top_visible", "crops"), sub):
        assert np.array_equal(got[name].numpy(), e), name
    again = views.scene_views(c1.geom, as_result(c1.bits), c1.cfg, frame_ids=frames)            # ids without ".jpg"
    same_views(got, again)
    with pytest.raises(KeyError, match="31"):
        views.scene_views(c1.geom, as_result(c1.bits), c1.cfg, frame_ids=["0.jpg", "31.jpg"])
    cfg = cfg_for(c1.scene, views_top_k=2, views_min_points=400, views_crop_levels=1, views_crop_expand=0.5)
    got = views.scene_views(c1.geom, as_result(c1.bits), cfg)
    exp = wr.select_views(c1.exp["visible"], c1.exp["boxes"], 480, 640, 2, 400, 1, 0.5)
    for name, e in zip(("top", "top_visible", "crops"), exp):
        assert np.array_equal(got[name].numpy(), e), name
    assert (exp[0] == -1).any() and (exp[0] >= 0).any()


def test_scene_views_in_slot_groups(lib, c1, monkeypatch):
    from beyond_fixed_forms_amd import projection, views
    need = sum(lib.visibility_table_bytes(c1.geom.n_points, len(c1.frames), c1.n_pairs))
    monkeypatch.setenv("BFF_VIS_TABLE_MAX_MB", repr(need / 3.5 / (1 << 20)))     # no three groups hold the whole table
    assert 3 * projection.vis_table_max_bytes() < need and c1.n_pairs > 10000
    before = lib.visibility_builds()
    got = views.scene_views(c1.geom, as_result(c1.bits), c1.cfg)
    assert lib.visibility_builds() - before >= 3                     # at least three slot groups
    assert_views(got, c1.exp, c1.frames, 480, 640)


def test_scene_views_without_instances(lib, c1):
    from beyond_fixed_forms_amd import views
    got = views.scene_views(c1.geom, as_result(c1.bits[:0]), c1.cfg)
    f = len(c1.frames)
    shapes = dict(area=(0,), visible=(0, f), boxes=(0, f, 4), top=(0, 5), top_visible=(0, 5), crops=(0, 5, 3, 4))
    for name in NAMES:
        assert got[name].dtype == torch.int32 and tuple(got[name].shape) == shapes[name], name
    assert got["frame_ids"] == [f"{x}.jpg" for x in c1.frames]


def test_scene_views_with_rendered_depth(lib, c1):
    from beyond_fixed_forms_amd import views
    from beyond_fixed_forms_amd.scene import geometry_for_depth_frames, rendered_depth_on_device
    cfg = cfg_for(c1.scene, depth_from_cloud=2)
    scene = types.SimpleNamespace(scene_id=c1.scene.scene_id, points=c1.scene.points, cam_intr=c1.scene.cam_intr,
                                  poses=c1.scene.poses, depths={}, depths_raw=None, stage1=None)      # no depth frame at all
    frames = c1.frames[:4]
    geom = geometry_for_depth_frames(scene, cfg, frames, DEV)
    # the frames the geometry rendered, as float32 (H, W) images (the separate resize pass: bit-identical to the sweep's)
    depth = rendered_depth_on_device(geom.xyz, geom.n_points, geom.inv_pose_host, scene.cam_intr, 480, 640, 2, geom.tile_bounds,
                                     raw_depth_resident=False)[0]
    depths = depth.cpu().numpy().reshape(len(frames), 480, 640)
    assert (depths != 0).mean() > 0.01
    exp = expected_views(c1.scene, geom, c1.bits, frames, depths, cfg)
    exp.pop("n_pairs")
    got = views.scene_views(geom, as_result(c1.bits), cfg)
    assert_views(got, exp, frames, 480, 640)
    # a condition on the input, not on the kernel: the case says something (the resize mixes a sparse cloud's texels with
    # the holes beside them, so these frames confirm far fewer points than the sensor's) and is another case than the first
    assert exp["visible"].sum() > 100 and (exp["top"] >= 0).any() and not np.array_equal(exp["visible"], c1.exp["visible"][:, :4])


def test_scene_views_of_the_hand_scene(lib):
    from beyond_fixed_forms_amd import views
    from beyond_fixed_forms_amd.scene import geometry_for_depth_frames
    scene = hs.scene([])
    # the hand scene's depths (1 + f metres) confirm none of its points (z from 2.1 to 2.9): every box is the sentinel; a
    # second set of frames at the points' own depths sees them
    for depths in (scene.depths, {f: np.full((hs.H, hs.W), 2.1 + 0.2 * (i % 5), np.float32) for i, f in enumerate(scene.depths)}):
        scene.depths = depths
        cfg = hs.config()
        frames = ["20", "0", "30", "5"]
        geom = geometry_for_depth_frames(scene, cfg, frames, DEV)
        assert geom.perm.cpu().tolist() == hs.PERM
        bits = np.array([[1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 1], [0, 1, 1, 0, 0]], bool)
        exp = expected_views(scene, geom, bits, frames, [scene.depths[f] for f in frames], cfg)
        assert exp.pop("n_pairs") == exp["visible"][0].sum()
        got = views.scene_views(geom, as_result(bits), cfg)
        assert_views(got, exp, frames, hs.H, hs.W)
        assert exp["area"].tolist() == [5, 0, 2, 2]
    assert exp["visible"].any() and (exp["top"][0] >= 0).any()


def test_scene_views_reuses_the_geometry_table(lib):
    from beyond_fixed_forms_amd import views
    from beyond_fixed_forms_amd.projection import VisibilityTable, run_projection
    from beyond_fixed_forms_amd.scene import geometry_for_depth_frames, prepare_class, prepare_geometry
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=11)
    cfg = cfg_for(scene)
    geom = prepare_geometry(scene, cfg, [scene.mask_2d], device=DEV)
    ds = prepare_class(geom, scene.mask_2d, cfg)
    res = [run_projection(ds, cfg) for _ in range(2)][1]            # the second projection of the class builds the table
    tab = geom.__dict__["_vis_tables"][0.08]
    assert isinstance(tab, VisibilityTable) and res.debug["sweep"] == "cached" and res.rows.shape[0] > 0
    torch.cuda.synchronize()
    before = lib.visibility_builds()
    got = views.scene_views(ds, res, cfg)                            # a DeviceScene that shares the geometry
    also = views.scene_views(geom, res, cfg, frame_ids=geom.frame_ids[::-1])
    assert lib.visibility_builds() == before, "scene_views built a table although the geometry holds one"
    assert geom.__dict__["_vis_tables"][0.08] is tab
    fresh = geometry_for_depth_frames(scene, cfg, geom.frame_ids, DEV)
    exp = views.scene_views(fresh, res, cfg)
    assert lib.visibility_builds() == before + 1
    same_views(got, exp)
    assert got["visible"].any() and torch.equal(also["visible"], got["visible"].flip(1))
    assert torch.equal(also["boxes"], got["boxes"].flip(1))
    bits = wr.unpack(res.rows.cpu().numpy().view(np.uint64), geom.n_points)
    ref = expected_views(scene, geom, bits, geom.frame_ids, [scene.depths[f] for f in geom.frame_ids], cfg)
    ref.pop("n_pairs")
    assert_views(got, ref, geom.frame_ids, scene.height, scene.width)


# ------------------------------------------------------------------ 4. the tool
def tool_tree(tmp_path):
    """Two tiny scenes on disk in the reference's layout (16-bit depth PNGs), the instances of class "table" of a final
    stage -- dense for one scene, the reference's empty form for the other -- and an assembled file of the first."""
    from PIL import Image
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.synthetic import make_scene
    scenes = {}
    for seed, scene_id in ((40, "scene_a"), (41, "scene_b")):
        sc = make_scene("tiny", seed=seed)
        sc.scene_id = scene_id
        sd = tmp_path / "2d" / scene_id
        for sub in ("intrinsic", "pose", "depth", "color"):
            (sd / sub).mkdir(parents=True)
        (tmp_path / "npy").mkdir(exist_ok=True)
        np.savetxt(sd / "intrinsic" / "intrinsic_color.txt", sc.cam_intr)
        np.save(tmp_path / "npy" / f"{scene_id}.npy", sc.points)
        for f in sc.color_files:
            (sd / "color" / f).write_bytes(b"")
        for fid, pose in sc.poses.items():
            np.savetxt(sd / "pose" / f"{fid}.txt", pose)
            Image.fromarray(np.round(sc.depths[fid].astype(np.float64) * 1000).astype(np.uint16)).save(sd / "depth" / f"{fid}.png")
        scenes[scene_id] = sc
    bits = object_instances(scenes["scene_a"])
    bits = bits[bits.any(axis=1)]
    final = {"ins": torch.from_numpy(bits), "conf": torch.linspace(0.9, 0.1, bits.shape[0]), "final_class": ["table"] * bits.shape[0]}
    (tmp_path / "final" / "table").mkdir(parents=True)
    (tmp_path / "assembled").mkdir()
    torch.save(final, tmp_path / "final" / "table" / "scene_a.pth")
    torch.save({"ins": torch.tensor([[]]), "conf": torch.tensor([]), "final_class": []}, tmp_path / "final" / "table" / "scene_b.pth")
    torch.save(dict(final, classes=["table"], source=torch.zeros((bits.shape[0], 2), dtype=torch.int64),
                    removed_by=torch.full((bits.shape[0],), -1)), tmp_path / "assembled" / "scene_a.pth")
    sc = scenes["scene_a"]
    cfg = Config.with_defaults(width_2d=sc.width, height_2d=sc.height, scene_2d_dir=str(tmp_path / "2d"),
                               scene_npy_dir=str(tmp_path / "npy"), final_output_dir=str(tmp_path / "final"),
                               mask_3d_dir=str(tmp_path / "m3d"), assembled_output_dir=str(tmp_path / "assembled"),
                               views_output_dir=str(tmp_path / "views"), views_top_k=3, views_crop_levels=2)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    return scenes, bits, cfg


def test_tool(lib, tmp_path):
    from beyond_fixed_forms_amd import cli, views
    from beyond_fixed_forms_amd.scene import geometry_for_depth_frames
    scenes, bits, cfg = tool_tree(tmp_path)
    argv = ["--config", str(tmp_path / "config.yaml")]
    assert cli.select_views_main(argv + ["--cls", "table"]) == 0
    assert sorted(os.listdir(tmp_path / "views" / "table")) == ["scene_a.pth", "scene_b.pth"]
    sc = scenes["scene_a"]
    frames = list(sc.poses)                                          # every downsample_ratio-th colour frame
    kinds = dict(frame_ids=list, height=int, width=int, depth_thresh=float)
    out = torch.load(tmp_path / "views" / "table" / "scene_a.pth", weights_only=False)
    assert list(out) == list(NAMES) + list(kinds) and all(type(out[k]) is t for k, t in kinds.items())
    k, f = bits.shape[0], len(frames)
    shapes = dict(area=(k,), visible=(k, f), boxes=(k, f, 4), top=(k, 3), top_visible=(k, 3), crops=(k, 3, 2, 4))
    for name in NAMES:
        assert out[name].dtype == torch.int32 and tuple(out[name].shape) == shapes[name], name
    assert out["frame_ids"] == [f"{x}.jpg" for x in frames] and (out["height"], out["width"]) == (sc.height, sc.width)
    # the PNGs hold the generator's own millimetres: the in-memory scene gives the same
    geom = geometry_for_depth_frames(sc, cfg, frames, DEV)
    same_views(out, views.scene_views(geom, as_result(bits), cfg))
    assert out["visible"].any() and (out["top"] >= 0).any() and out["area"].tolist() == bits.sum(axis=1).tolist()
    # the empty form: K = 0 arrays of the same shapes
    empty = torch.load(tmp_path / "views" / "table" / "scene_b.pth", weights_only=False)
    assert list(empty) == list(out) and len(empty["frame_ids"]) == len(scenes["scene_b"].poses)
    f = len(empty["frame_ids"])
    for name, shape in dict(area=(0,), visible=(0, f), boxes=(0, f, 4), top=(0, 3), top_visible=(0, 3), crops=(0, 3, 2, 4)).items():
        assert empty[name].dtype == torch.int32 and tuple(empty[name].shape) == shape, name
    # --every: another frame set; --assembled: the assembly tool's file, saved without a class directory
    assert cli.select_views_main(argv + ["--cls", "table", "--every", "20"]) == 0
    wide = torch.load(tmp_path / "views" / "table" / "scene_a.pth", weights_only=False)
    assert wide["frame_ids"] == out["frame_ids"][::2] and torch.equal(wide["visible"], out["visible"][:, ::2])
    assert cli.select_views_main(argv + ["--assembled"]) == 0
    assert sorted(os.listdir(tmp_path / "views")) == ["scene_a.pth", "table"]
    same_views(torch.load(tmp_path / "views" / "scene_a.pth", weights_only=False), out)
