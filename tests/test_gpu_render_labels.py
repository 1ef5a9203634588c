"""3-D instances rendered back into the views on the GPU: bff_point_labels, bff_render_labels_u16 and the label image ->
run tables step against their NumPy statements (tests/label_render_ref.py), the depth half against the depth renderers
themselves, the run tables against masks2d.encode_masks of the dense masks, and reproject.instance_masks_2d and the
command-line tool against the statement.  Everything is compared for equality."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import label_render_ref as lr
import render_depth_ref as rd
import test_gpu_splat_depth as tg
from oracle import rle_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_PAD, F, K33, R = tg.N, tg.N_PAD, tg.F, tg.K33, lr.R
RENDER_CASES = [(h, w, stride, nf, radius) for (h, w, stride, nf) in tg.CASES for radius in (0.0, R)]


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def as_i16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV)


# ------------------------------------------------------------------ bff_point_labels
@pytest.mark.parametrize("k,n", [(1, 1500), (3, 1500), (70, 1500), (200, 1500), (3, 64), (70, 1)])
def test_point_labels_equal_numpy(lib, k, n):
    """Overlapping rows, an empty row, n_points no multiple of 64 (and one that is, and a single point), with and without
    unsort; K = 70 and 200 hold instances beyond the first 64."""
    from beyond_fixed_forms_amd import reproject
    rng = np.random.default_rng(k * 7 + n)
    dense = rng.random((k, n)) < (0.6 / k + 0.01)
    if k >= 3:
        dense[1] = False                                                 # an empty row
        dense[k - 1] |= dense[0]                                         # the last row overlaps the first
        dense[k - 1, n - 1] = True
    rows = lib.pack_rows(torch.from_numpy(dense).to(DEV))
    assert tuple(rows.shape) == (k, (n + 63) // 64)
    exp = lr.point_labels_ref(dense)
    if k >= 3 and n > 64:
        assert (dense.sum(0) > 1).any() and (exp == 0).any() and exp.max() <= k and 2 not in exp
    got = reproject.point_labels(rows, n)
    assert got.dtype == torch.int16 and tuple(got.shape) == (n,)
    assert np.array_equal(u16(got), exp)
    perm = rng.permutation(n)
    unsort = np.empty(n, np.int32)
    unsort[perm] = np.arange(n, dtype=np.int32)
    got = reproject.point_labels(rows, n, torch.from_numpy(unsort).to(DEV))
    assert np.array_equal(u16(got), lr.point_labels_ref(dense, unsort)) and np.array_equal(u16(got), exp[perm])
    order = rng.permutation(k)                                           # priority by another order: that order's first row
    got = reproject.point_labels(rows, n, order=order)
    assert np.array_equal(u16(got), lr.point_labels_ref(dense[order]))


def test_point_labels_limits(lib):
    from beyond_fixed_forms_amd import reproject
    with pytest.raises(ValueError, match="65534"):
        reproject.point_labels(torch.zeros((65535, 1), dtype=torch.int64, device=DEV), 10)
    none = reproject.point_labels(torch.zeros((0, 2), dtype=torch.int64, device=DEV), 100)
    assert tuple(none.shape) == (100,) and int(none.count_nonzero()) == 0


# ------------------------------------------------------------------ bff_render_labels_u16
@functools.lru_cache(maxsize=None)
def reference(k, h, w, stride, nf, radius):
    """The statement's (labels, depth) -- computed once, never written to."""
    xyz, inv, _, lab = lr.label_cloud(k)
    out = lr.render_labels_ref(xyz, lab[:N], inv[:nf], K33, h, w, *rd.rendered_size(h, w, stride), radius)
    for a in out:
        a.setflags(write=False)
    return out


def render(lib, k, h, w, stride, nf=F, radius=0.0, bounds=False, want_depth=True, **kw):
    _, inv, soa, lab = lr.label_cloud(k)
    dh, dw = rd.rendered_size(h, w, stride)
    xyz = torch.from_numpy(soa).to(DEV)
    lab_dev = as_i16(lab)[:N]                                            # the padding's labels lie behind the view
    tb = lib.point_tile_bounds(xyz, N) if bounds else None
    labels, depth = lib.render_labels(xyz, N, lab_dev, torch.from_numpy(inv[:nf].copy()).to(DEV), K33, h, w, dh, dw,
                                      tile_bounds=tb, splat_radius=radius, want_depth=want_depth, **kw)
    assert labels.dtype == torch.int16 and tuple(labels.shape) == (nf, dh, dw)
    return u16(labels), (u16(depth) if want_depth else depth)


def render_depth(lib, k, h, w, stride, nf, radius):
    _, inv, soa, _ = lr.label_cloud(k)
    out = lib.render_depth(torch.from_numpy(soa).to(DEV), N, torch.from_numpy(inv[:nf].copy()).to(DEV), K33, h, w,
                           *rd.rendered_size(h, w, stride), splat_radius=radius)
    return u16(out)


@pytest.mark.parametrize("h,w,stride,nf,radius", RENDER_CASES)
def test_kernel_equals_statement(lib, h, w, stride, nf, radius):
    exp_l, exp_d = reference(70, h, w, stride, nf, radius)
    labels, depth = render(lib, 70, h, w, stride, nf, radius)
    assert np.array_equal(labels, exp_l), np.argwhere(labels != exp_l)[:10]
    assert np.array_equal(depth, exp_d), np.argwhere(depth != exp_d)[:10]
    # the depth half is the matching depth renderer's frame, byte for byte
    assert depth.tobytes() == render_depth(lib, 70, h, w, stride, nf, radius).tobytes()
    culled, culled_d = render(lib, 70, h, w, stride, nf, radius, bounds=True)   # same frames with the culling table
    assert np.array_equal(culled, exp_l) and np.array_equal(culled_d, exp_d)
    only, none = render(lib, 70, h, w, stride, nf, radius, want_depth=False)    # and without the depth output
    assert none is None and only.tobytes() == labels.tobytes()


@pytest.mark.parametrize("h,w,stride,nf,radius", [(50, 70, 1, 3, 0.0), (50, 70, 3, 5, R), (48, 64, 2, 3, R), (48, 64, 8, 6, 0.0)])
def test_three_instances_equal_statement(lib, h, w, stride, nf, radius):
    exp_l, exp_d = reference(3, h, w, stride, nf, radius)
    labels, depth = render(lib, 3, h, w, stride, nf, radius, bounds=True)
    assert np.array_equal(labels, exp_l) and np.array_equal(depth, exp_d) and labels.max() == 3


def test_crafted_pairs(lib):
    """Frame 0 at stride 1, radius 0 (test_label_render_host pins the statement on the same pixels): at equal
    millimetres the smaller label wins and background wins over every label; one millimetre decides otherwise; the
    padding's labelled point (it would land at m = 100) is never read."""
    for k, hi in ((3, 3), (70, 5)):
        for h, w in ((50, 70), (48, 64)):
            labels, depth = render(lib, k, h, w, 1, 1)
            at = lambda px, img: int(img[0, px[1], px[0]])
            assert [at(p, labels) for p in (lr.PIX_TIE, lr.PIX_TIE_BG, lr.PIX_BEHIND, lr.PIX_FRONT)] == [2, 0, 0, hi]
            assert [at(p, depth) for p in (lr.PIX_TIE, lr.PIX_TIE_BG, lr.PIX_BEHIND, lr.PIX_FRONT)] == [300] * 4
            assert not (depth == 100).any()
    labels, depth = render(lib, 70, 50, 70, 1, F)
    assert not labels[F - 1].any() and not depth[F - 1].any()            # the NaN pose sees nothing
    assert (labels[0][depth[0] != 0] == 0).any() and (labels[0] != 0).any()     # background holds texels of its own


@pytest.mark.parametrize("tile", [1, 4, 0])
@pytest.mark.parametrize("h,w,stride,radius", [(50, 70, 2, R), (48, 64, 3, 0.0)])
def test_frame_tiles_and_culling_table(lib, h, w, stride, radius, tile):
    exp_l, exp_d = reference(70, h, w, stride, F, radius)
    for bounds in (False, True):
        labels, depth = render(lib, 70, h, w, stride, F, radius, bounds=bounds, frames_per_block=tile)
        assert np.array_equal(labels, exp_l) and np.array_equal(depth, exp_d), (bounds, tile)


def test_scratch_smaller_than_the_frames_and_repeat_runs(lib):
    exp_l, exp_d = reference(70, 50, 70, 8, F, R)
    a = render(lib, 70, 50, 70, 8, F, R, bounds=True, scratch_texels=4 * 7 * 9 + 5)     # runs of 4, 4 and 1 frames
    b = render(lib, 70, 50, 70, 8, F, R, scratch_texels=1, frames_per_block=8)          # frame by frame
    for labels, depth in (a, b):
        assert np.array_equal(labels, exp_l) and np.array_equal(depth, exp_d)
    x, y = render(lib, 70, 50, 70, 1, 3, R), render(lib, 70, 50, 70, 1, 3, R)
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


def test_bad_arguments_and_empty_inputs(lib):
    _, inv, soa, lab = lr.label_cloud(70)
    xyz, poses = torch.from_numpy(soa).to(DEV), torch.from_numpy(inv).to(DEV)
    for bad in (float("nan"), -R, float("inf")):
        with pytest.raises(RuntimeError, match="splat_radius"):
            lib.render_labels(xyz, N, as_i16(lab)[:N], poses, K33, 50, 70, 7, 9, splat_radius=bad)
    with pytest.raises(ValueError, match="labels for"):
        lib.render_labels(xyz, N, as_i16(lab), poses, K33, 50, 70, 7, 9)
    with pytest.raises(ValueError, match="device tensors"):
        lib.render_labels(xyz, N, as_i16(lab)[:N].cpu(), poses, K33, 50, 70, 7, 9)
    labels, depth = lib.render_labels(xyz, N, as_i16(lab)[:N], poses[:0], K33, 50, 70, 7, 9, want_depth=True)
    assert tuple(labels.shape) == (0, 7, 9) == tuple(depth.shape)
    labels, depth = lib.render_labels(xyz, 0, as_i16(lab)[:0], poses, K33, 50, 70, 7, 9, splat_radius=R, want_depth=True)
    torch.cuda.synchronize()
    assert tuple(labels.shape) == (F, 7, 9) and int(labels.count_nonzero()) == 0 and int(depth.count_nonzero()) == 0


# ------------------------------------------------------------------ label image -> run tables
def dense_masks(labels, h, w, min_pixels=1):
    """The test's own upsampling, by torch indexing: per frame the dense masks up == L of the labels present, and L - 1."""
    lab = labels.to(torch.int32) & 0xFFFF
    _, dh, dw = lab.shape
    vi = (torch.arange(h, device=lab.device) * dh) // h
    ui = (torch.arange(w, device=lab.device) * dw) // w
    up = lab[:, vi][:, :, ui]
    frames, names = [], []
    for f in range(up.shape[0]):
        present = [int(v) for v in torch.unique(up[f]).tolist() if v >= 1 and int((up[f] == v).sum()) >= max(1, min_pixels)]
        frames.append(torch.stack([up[f] == v for v in present]) if present else
                      torch.zeros((0, h, w), dtype=torch.bool, device=lab.device))
        names += [v - 1 for v in present]
    return frames, names


def check_runs(lib, labels, h, w, min_pixels=1, n_labels=None):
    from beyond_fixed_forms_amd import masks2d, reproject
    frames, names = dense_masks(labels, h, w, min_pixels)
    views = masks2d.encode_masks(frames)
    exp = views[0].owner
    got, mask_label = reproject.label_runs(labels, h, w, min_pixels, n_labels)
    assert got.n_masks == exp.n_masks == len(names) and got.n_pixels == h * w and got.frame_offs == exp.frame_offs
    for a, b in ((got.run_start, exp.run_start), (got.run_end, exp.run_end), (got.mask_run_offs, exp.mask_run_offs)):
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)
    assert mask_label.dtype == torch.int32 and mask_label.tolist() == names
    again, again_label = reproject.label_runs(labels, h, w, min_pixels, n_labels)       # a pure function of the image
    assert torch.equal(again.run_start, got.run_start) and torch.equal(again.run_end, got.run_end)
    assert torch.equal(again.mask_run_offs, got.mask_run_offs) and torch.equal(again_label, mask_label)
    for view, e in zip(got.frames(), views):                             # the per-frame views line up, too
        assert len(view) == len(e) and view.first_mask == e.first_mask
    return got, names


@pytest.mark.parametrize("stride,radius", [(1, 0.0), (3, R), (3, 0.0), (8, R)])
def test_runs_of_rendered_frames(lib, stride, radius):
    """The frames rendered above at 50 x 70; at stride 3 (17 x 24 texels) neither size divides."""
    labels, _ = render(lib, 70, 50, 70, stride, 5, radius)
    got, names = check_runs(lib, as_i16(labels), 50, 70, n_labels=70)
    assert got.n_masks > 20 and int(got.run_start.shape[0]) > got.n_masks
    check_runs(lib, as_i16(labels), 50, 70)                              # the label bound found by the call itself
    s, e, o, ml, fo = lr.label_runs_ref(labels, 50, 70)                  # and the NumPy statement
    assert np.array_equal(got.run_start.cpu().numpy(), s) and np.array_equal(got.run_end.cpu().numpy(), e)
    assert np.array_equal(got.mask_run_offs.cpu().numpy(), o) and fo == got.frame_offs and ml.tolist() == names


def hand_images():
    hand = np.zeros((5, 6, 8), np.uint16)
    hand[0] = 3                                                          # a whole frame of one label
    hand[1, 5, 7] = 2                                                    # a single last pixel
    hand[3].reshape(-1)[::2] = 1                                         # (frame 2: no label) alternating every pixel
    hand[3].reshape(-1)[1::2] = 4
    hand[4, 2, 3:5] = 9                                                  # present in one frame only: 2 pixels
    hand[4, 0:2] = 1
    return hand


def test_runs_of_hand_made_images(lib):
    hand = as_i16(hand_images())
    got, names = check_runs(lib, hand, 6, 8)
    assert names == [2, 1, 0, 3, 0, 8] and got.frame_offs == [0, 1, 2, 2, 4, 6]
    assert got.run_start[:2].tolist() == [0, 47] and got.run_end[:2].tolist() == [48, 48]     # one run across every row end
    assert got.mask_run_offs.tolist() == [0, 1, 2, 26, 50, 51, 52]
    got, names = check_runs(lib, hand, 6, 8, min_pixels=3)               # the single pixel and the 2-pixel mask drop out
    assert names == [2, 0, 3, 0] and got.frame_offs == [0, 1, 1, 1, 3, 4] and got.mask_run_offs.tolist() == [0, 1, 25, 49, 50]
    check_runs(lib, hand, 6, 8, n_labels=20)                             # a generous bound changes nothing
    check_runs(lib, hand, 13, 20)                                        # upsampled by ratios that do not divide
    check_runs(lib, hand, 4, 5)                                          # and sampled down
    got, _ = check_runs(lib, hand, 6, 8, min_pixels=100)
    assert got.n_masks == 0 and got.frame_offs == [0] * 6 and got.run_start.numel() == 0
    from beyond_fixed_forms_amd import reproject
    none, lab = reproject.label_runs(hand[:0], 6, 8)
    assert none.n_masks == 0 and none.frame_offs == [0] and lab.numel() == 0


def test_runs_across_a_tile_edge(lib):
    """130 x 100 pixels: a frame spans two 8192-pixel tiles; label 2 runs across the edge (pixel 8192 = row 81, column 92),
    label 5 alternates with it pixel by pixel further up, label 1 ends on the last pixel; frame 1 holds one pixel on
    either side of the edge."""
    assert lib.load().bff_label_runs_tile_pixels() == 8192
    img = np.zeros((2, 130, 100), np.uint16)
    img[0, 80:84] = 2
    img[0].reshape(-1)[8100:8160:2] = 5
    img[0, 129, 50:] = 1
    img[1].reshape(-1)[8191] = 3
    img[1].reshape(-1)[8192] = 4
    got, names = check_runs(lib, as_i16(img), 130, 100)
    assert names == [0, 1, 4, 2, 3]
    check_runs(lib, as_i16(img[:, ::2, ::2].copy()), 130, 100)           # the same through the integer map


# ------------------------------------------------------------------ the path: rows -> masks of a view
def two_planes(far_is_instance):
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import Stage2Result
    scene, _, n_far = rd.two_plane_scene()
    n = scene.points.shape[0]
    dense = np.zeros((2 if far_is_instance else 1, n), bool)
    dense[0, n_far:] = True                                              # instance 0: the near plane
    if far_is_instance:
        dense[1, :n_far] = True
    rows = _lib.pack_rows(torch.from_numpy(dense).to(DEV))
    conf = torch.tensor([0.75, 0.25][:dense.shape[0]], dtype=torch.float16)
    result = Stage2Result(scene.scene_id, n, rows, conf.to(DEV), ["table", "floor"][:dense.shape[0]], [], {})
    cfg = Config.with_defaults(width_2d=64, height_2d=48, depth_from_cloud=1, min_aggragated_masks=1,
                               if_detected_ratio_threshold=False)
    return scene, result, cfg


def test_two_planes_by_hand(lib):
    """render_depth_ref.two_plane_scene at stride 1, radius 0: the near plane (instance 0) covers rows 16..31, columns
    20..43 and hides the far plane there."""
    from beyond_fixed_forms_amd import reproject
    scene, result, cfg = two_planes(False)
    geom = reproject.geometry_for_frames(scene, cfg, ["0"], DEV)
    assert geom.unsort is not None and geom.depth is None and geom.depth_raw is None
    lab = reproject.point_labels(result.rows, geom.n_points, geom.unsort)
    labels = u16(reproject.render_labels(geom, lab, geom.inv_pose_host))
    exp = np.zeros((1, 48, 64), np.uint16)
    exp[0, 16:32, 20:44] = 1
    assert np.array_equal(labels, exp)
    m = reproject.instance_masks_2d(geom, ["0.jpg"], result, cfg)
    assert len(m) == 1 and m[0]["frame_id"] == "0.jpg" and m[0]["labels"] == ["table"] and m[0]["instance_ids"].tolist() == [0]
    assert m[0]["confidences"].dtype == torch.float16 and m[0]["confidences"].tolist() == [0.75]
    runs = m[0]["segmented_frame_masks"]
    assert runs.run_start.tolist() == [v * 64 + 20 for v in range(16, 32)]
    assert runs.run_end.tolist() == [v * 64 + 44 for v in range(16, 32)]
    # the far plane as instance 1: the complement, and no pixel belongs to both
    scene, result, cfg = two_planes(True)
    m = reproject.instance_masks_2d(geom, ["0"], result, cfg)
    assert m[0]["labels"] == ["table", "floor"] and m[0]["instance_ids"].tolist() == [0, 1]
    from beyond_fixed_forms_amd import masks2d
    rles = masks2d.encode_2d_masks([dict(m[0])])[0]["segmented_frame_masks"]
    dense = rle_ref.rle_decode_batch_ref(rles).bool().numpy().reshape(2, 48, 64)
    assert np.array_equal(dense[0], exp[0] == 1) and np.array_equal(dense[1], exp[0] == 0)


def test_masks_go_through_prepare_scene_and_the_rle_form(lib):
    """instance_masks_2d's list as a scene's mask_2d: prepare_scene takes it as it is (its run tables are the list's), and
    encode_2d_masks turns it into RLE dicts that decode to the statement's dense masks."""
    import copy
    from beyond_fixed_forms_amd import masks2d, reproject
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import Stage2Result
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = rd.without_depth(make_scene("tiny", seed=3, n_points=700))
    n = scene.points.shape[0]
    objects = [k for k in np.unique(scene.point_object) if k >= 0][:6]
    dense = np.stack([scene.point_object == k for k in objects])
    rows = lib.pack_rows(torch.from_numpy(dense).to(DEV))
    conf = torch.linspace(0.2, 0.9, len(objects)).to(torch.float16)
    result = Stage2Result(scene.scene_id, n, rows, conf.to(DEV), [f"thing {k}" for k in objects], [], {})
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height, depth_from_cloud=2, reproject_stride=2,
                               reproject_splat_radius=0.05, reproject_min_pixels=4)
    ids = list(scene.poses)
    geom = reproject.geometry_for_frames(scene, cfg, ids, DEV)
    masks = reproject.instance_masks_2d(geom, ids, result, cfg)
    assert [fr["frame_id"] for fr in masks] == [f"{f}.jpg" for f in ids] and sum(len(fr["labels"]) for fr in masks) > 3
    # the statement, from the cloud in its original order
    inv = np.stack([np.linalg.inv(scene.poses[f]) for f in ids])
    dh, dw = rd.rendered_size(scene.height, scene.width, 2)
    labels, _ = lr.render_labels_ref(scene.points, lr.point_labels_ref(dense), inv, scene.cam_intr[:3, :3], scene.height,
                                     scene.width, dh, dw, 0.05)
    s, e, o, ml, fo = lr.label_runs_ref(labels, scene.height, scene.width, 4)
    owner = masks[0]["segmented_frame_masks"].owner
    assert np.array_equal(owner.run_start.cpu().numpy(), s) and np.array_equal(owner.run_end.cpu().numpy(), e)
    assert np.array_equal(owner.mask_run_offs.cpu().numpy(), o) and owner.frame_offs == fo
    for fr, a, b in zip(masks, fo[:-1], fo[1:]):
        assert fr["instance_ids"].tolist() == ml[a:b].tolist() and fr["labels"] == [f"thing {objects[i]}" for i in ml[a:b]]
        assert torch.equal(fr["confidences"], conf[ml[a:b].astype(np.int64)])
    # prepare_scene, unchanged
    scene2 = copy.copy(scene)
    scene2.mask_2d = masks
    ds = prepare_scene(scene2, cfg, DEV, with_viewed=False)
    assert ds.n_rows == len(ml) and torch.equal(ds.run_start, owner.run_start) and torch.equal(ds.run_end, owner.run_end)
    assert torch.equal(ds.mask_run_offs, owner.mask_run_offs) and ds.labels == [f"thing {objects[i]}" for i in ml]
    # the RLE form decodes to the dense masks
    up = lr.upsample(labels, scene.height, scene.width)
    for f, fr in enumerate(masks2d.encode_2d_masks([dict(fr) for fr in masks])):
        rles = fr["segmented_frame_masks"]
        assert isinstance(rles, list) and len(rles) == fo[f + 1] - fo[f]
        if rles:
            got = rle_ref.rle_decode_batch_ref(rles).bool().numpy()
            exp = np.stack([(up[f] == l + 1).reshape(-1) for l in ml[fo[f]:fo[f + 1]]])
            assert np.array_equal(got, exp)


def test_command_line_tool(lib, tmp_path):
    """tools/reproject_3d_to_2d.py on a scene directory without depth/: one entry per selected frame, whose RLE dicts
    decode to the statement's masks; a class without an output directory exits 1."""
    import yaml
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=3, n_points=700)
    cls = "table"
    rd.write_scene_without_depth(tmp_path, scene, {cls: scene.mask_2d})
    objects = [k for k in np.unique(scene.point_object) if k >= 0][:5]
    dense = np.stack([scene.point_object == k for k in objects])
    final = {"ins": torch.from_numpy(dense), "conf": torch.linspace(0.3, 0.8, len(objects)),
             "final_class": [f"thing {k}" for k in objects]}
    (tmp_path / "final" / cls).mkdir(parents=True)
    torch.save(final, tmp_path / "final" / cls / f"{scene.scene_id}.pth")
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height, scene_2d_dir=str(tmp_path / "2d"),
                               scene_npy_dir=str(tmp_path / "npy"), mask_2d_dir=str(tmp_path / "m2d"),
                               final_output_dir=str(tmp_path / "final"), mask_3d_dir=str(tmp_path / "m3d"),
                               reprojected_2d_dir=str(tmp_path / "r2d"), reproject_stride=3, reproject_splat_radius=0.04)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    tool = [sys.executable, os.path.join(ROOT, "tools", "reproject_3d_to_2d.py"), "--config", str(tmp_path / "config.yaml")]
    r = subprocess.run(tool + ["--cls", cls], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    saved = torch.load(tmp_path / "r2d" / cls / f"{scene.scene_id}.pth", weights_only=False)
    ids = list(scene.poses)                                              # every downsample_ratio-th colour frame
    assert [fr["frame_id"] for fr in saved] == [f"{f}.jpg" for f in ids]
    inv = np.stack([np.linalg.inv(scene.poses[f]) for f in ids])
    dh, dw = rd.rendered_size(scene.height, scene.width, 3)
    labels, _ = lr.render_labels_ref(scene.points, lr.point_labels_ref(dense), inv, scene.cam_intr[:3, :3], scene.height,
                                     scene.width, dh, dw, 0.04)
    up = lr.upsample(labels, scene.height, scene.width)
    total = 0
    for f, fr in enumerate(saved):
        present = [int(l) for l in np.unique(up[f]) if l >= 1]
        assert fr["instance_ids"].tolist() == [l - 1 for l in present]
        assert fr["labels"] == [f"thing {objects[l - 1]}" for l in present] and len(fr["confidences"]) == len(present)
        rles = fr["segmented_frame_masks"]
        assert isinstance(rles, list) and len(rles) == len(present)
        if present:
            assert all(int(x["length"]) == scene.height * scene.width for x in rles)
            got = rle_ref.rle_decode_batch_ref(rles).bool().numpy()
            assert np.array_equal(got, np.stack([(up[f] == l).reshape(-1) for l in present]))
        total += len(present)
    assert total > 3
    r = subprocess.run(tool + ["--cls", "no such class"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "no such class" in r.stderr
