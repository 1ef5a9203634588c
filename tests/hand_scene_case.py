"""One scene small enough to prepare by hand, and the tables it must become, written out value by value from the rules
(P:413-461 for the mask frames, P:538-567 for the frames of the detection-ratio sweep, scene.prepare_scene's comments
for the layout): nothing here is computed by a function of the package.  Used on the CPU (test_multiclass_host.py) and
through the native / staged path on the GPU (test_gpu_ingest.py).

4 x 4 images, five points, downsample_ratio 2.  The colour files make the viewed frames 0, 10, 20, 30.  The depth of
frame f is the constant 1 + f and its pose a translation by f / 8 along x, so the frame that sits in a depth slot or
behind a kernel frame can be read back from the tables.  Every mask is one one-pixel run; confidences are float16.

m32: frame 10 with labels a b; frame 20 without masks; frame 10 again with a; frame 5 (not viewed) with c.
m64: m32 + frame 30 with 33 masks labelled d.

What the expected tables show: the frame without masks gets no kernel frame and, for a single class, a later slot (20
after 0) while the union of a multi-class run gives it the second slot; a frame id that comes twice is flagged on its
first appearance only and keeps one slot; a frame outside the viewed set is never flagged; the viewed-only tail follows
the viewed order; one frame with 33 masks makes the whole class 64-bit, in one chunk."""
import types

import numpy as np
import torch

H = W = 4
COLOR_FILES = ["30.jpg", "x.png", "5.jpg", "0.jpg", "25.jpg", "10.jpg", "20.jpg", "15.jpg"]
FRAMES = (0, 5, 10, 15, 20, 25, 30)
# original order: descending along the diagonal, so the Morton order is the reverse
POINTS = np.array([[0.9 - 0.2 * k, 0.9 - 0.2 * k, 2.9 - 0.2 * k, 0.0, 0.0, 0.0] for k in range(5)])
PERM = [4, 3, 2, 1, 0]


def _frame(fid, pixels, labels, conf):
    return {"frame_id": f"{fid}.jpg", "labels": list(labels), "confidences": torch.tensor(conf, dtype=torch.float16),
            "segmented_frame_masks": [{"length": H * W, "counts": np.array([p + 1, 1])} for p in pixels]}   # 1-based start


def masks():
    m32 = [_frame(10, [3, 7], "ab", [0.5, 0.25]), _frame(20, [], "", []), _frame(10, [0], "a", [0.75]),
           _frame(5, [15], "c", [0.125])]
    m64 = m32 + [_frame(30, [k % 16 for k in range(33)], "d" * 33, [k / 64 for k in range(33)])]
    return m32, m64


def scene(mask_2d):
    """SceneInputs-like; float32 (H, W) depth in metres."""
    pose = lambda f: np.array([[1, 0, 0, f / 8], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    intr = np.array([[2.0, 0, 2, 0], [0, 2.0, 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return types.SimpleNamespace(
        scene_id="hand", points=POINTS.copy(), cam_intr=intr, poses={str(f): pose(f) for f in FRAMES},
        depths={str(f): np.full((H, W), 1 + f, dtype=np.float32) for f in FRAMES}, mask_2d=mask_2d,
        color_files=list(COLOR_FILES), stage1=None, height=H, width=W, depths_raw=None, depth_staged=None)


def config():
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=W, height_2d=H, downsample_ratio=2)


_ROWS32 = dict(run_start=[3, 7, 0, 15], labels=list("abac"), label_id=[0, 1, 0, 2], conf=[0.5, 0.25, 0.75, 0.125])
_ROWS64 = dict(run_start=_ROWS32["run_start"] + [k % 16 for k in range(33)], labels=list("abac") + ["d"] * 33,
               label_id=[0, 1, 0, 2] + [3] * 33, conf=_ROWS32["conf"] + [k / 64 for k in range(33)])

# frames: the frame id behind each kernel frame (its pose); slots: the frame id in each depth slot
EXPECTED = {
    "scene m32": dict(
        _ROWS32, frames=[10, 10, 5, 0, 20, 30], depth_index=[0, 0, 1, 2, 3, 4], frame_mask=[0, 1, 2, -1, -1, -1],
        frame_rowbase=[0, 2, 3, 0, 0, 0], frame_nmask=[2, 1, 1, 0, 0, 0], frame_flags=[1, 0, 0, 1, 1, 1],
        view_mask_offs=[0, 2, 3, 4], n_mask_frames=3, n_rows=4, word_bits=32, n_label_ids=3, n_viewed=4,
        slots=[10, 5, 0, 20, 30]),
    "scene m32 without viewed": dict(
        _ROWS32, frames=[10, 10, 5], depth_index=[0, 0, 1], frame_mask=[0, 1, 2], frame_rowbase=[0, 2, 3],
        frame_nmask=[2, 1, 1], frame_flags=[0, 0, 0], view_mask_offs=[0, 2, 3, 4], n_mask_frames=3, n_rows=4,
        word_bits=32, n_label_ids=3, n_viewed=0, slots=[10, 5]),
    "scene m64": dict(
        _ROWS64, frames=[10, 10, 5, 30, 0, 20], depth_index=[0, 0, 1, 2, 3, 4], frame_mask=[0, 1, 2, 3, -1, -1],
        frame_rowbase=[0, 2, 3, 4, 0, 0], frame_nmask=[2, 1, 1, 33, 0, 0], frame_flags=[1, 0, 0, 1, 1, 1],
        view_mask_offs=[0, 2, 3, 4, 37], n_mask_frames=4, n_rows=37, word_bits=64, n_label_ids=4, n_viewed=4,
        slots=[10, 5, 30, 0, 20]),
    "class m32": dict(
        _ROWS32, frames=[10, 10, 5], depth_index=[0, 0, 2], frame_mask=[0, 1, 2], frame_rowbase=[0, 2, 3],
        frame_nmask=[2, 1, 1], frame_flags=[0, 0, 0], view_mask_offs=[0, 2, 3, 4], n_mask_frames=3, n_rows=4,
        word_bits=32, n_label_ids=3, n_viewed=4, slots=[10, 20, 5, 30, 0]),
    "class m64": dict(
        _ROWS64, frames=[10, 10, 5, 30], depth_index=[0, 0, 2, 3], frame_mask=[0, 1, 2, 3], frame_rowbase=[0, 2, 3, 4],
        frame_nmask=[2, 1, 1, 33], frame_flags=[0, 0, 0, 0], view_mask_offs=[0, 2, 3, 4, 37], n_mask_frames=4,
        n_rows=37, word_bits=64, n_label_ids=4, n_viewed=4, slots=[10, 20, 5, 30, 0]),
}


def check_tables(ds, row, shared):
    """A DeviceScene against one entry of EXPECTED, element for element and dtype for dtype.  `shared`: the
    SceneGeometry the class was prepared against, or None for a single-class scene."""
    exp = EXPECTED[row]
    i32 = lambda k: (getattr(ds, k).dtype, getattr(ds, k).cpu().tolist())
    for k in ("depth_index", "frame_mask", "frame_rowbase", "frame_nmask", "frame_flags", "view_mask_offs", "label_id"):
        assert i32(k) == (torch.int32, exp[k]), (row, k, i32(k))
    nf, n_rows = len(exp["frames"]), exp["n_rows"]
    for k in ("n_mask_frames", "n_rows", "word_bits", "n_label_ids", "n_viewed", "labels"):
        assert getattr(ds, k) == exp[k], (row, k)
    assert (ds.n_frames, ds.n_points, ds.nw, ds.height, ds.width, ds.scene_id) == (nf, 5, 1, H, W, "hand")
    # one one-pixel run per mask
    assert i32("run_start") == (torch.int32, exp["run_start"])
    assert i32("run_end") == (torch.int32, [p + 1 for p in exp["run_start"]])
    assert i32("mask_run_offs") == (torch.int32, list(range(n_rows + 1)))
    assert ds.conf.dtype == torch.float16 and ds.conf.cpu().tolist() == exp["conf"]     # all exact in float16
    # the inverse of a translation by f / 8 along x is the translation by -f / 8
    inv = np.tile(np.eye(4).reshape(1, 16), (nf, 1))
    inv[:, 3] = [-f / 8 for f in exp["frames"]]
    assert ds.inv_pose.dtype == torch.float64 and np.array_equal(ds.inv_pose.cpu().numpy(), inv), row
    # the depth slots, and the cloud in Morton order
    assert ds.depth_raw is None and ds.depth_size is None and ds.depth.dtype == torch.float32
    depth = ds.depth.cpu().numpy()
    assert depth.shape == (len(exp["slots"]), H * W)
    assert np.array_equal(depth, np.repeat(1.0 + np.array(exp["slots"], np.float32)[:, None], H * W, axis=1)), row
    xyz = ds.xyz.cpu().numpy()
    assert ds.xyz.dtype == torch.float64 and xyz.shape == (3, 1024) and not xyz[:, 5:].any()
    assert np.array_equal(xyz[:, :5], POINTS[PERM, :3].T)
    assert i32("perm") == (torch.int32, PERM) and i32("unsort") == (torch.int32, PERM)
    assert np.array_equal(ds.cam_intr, np.array([[2.0, 0, 2], [0, 2.0, 2], [0, 0, 1]]))
    if shared is None:
        assert ds.geometry is None and ds.viewed_in is None
    else:
        assert ds.geometry is shared and ds.xyz is shared.xyz and ds.depth is shared.depth
        assert ds.viewed_in is shared.viewed
        assert shared.frame_ids == [str(f) for f in exp["slots"]] and shared.n_viewed == exp["n_viewed"]
