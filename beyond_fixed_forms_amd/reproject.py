"""3-D instances rendered back into the views as 2-D masks, on the device (include/bff_hip.h: bff_point_labels,
bff_render_labels_u16, bff_label_runs_count / bff_label_runs_emit).

The path otherwise runs one way: 2-D masks in, instance rows out (Stage2Result.rows, FinalResult.rows).  Here an
instance goes back into any posed view -- the frames it came from, or the nine in ten the 2-D stage never segmented:

    point_labels(rows, n_points, unsort)          instance bit rows -> one uint16 label per point of the sorted cloud
    render_labels(geom, lab, inv_pose, ...)       the point z-buffer with a label next to the depth: a label image per view
    label_runs(label_frames, height, width)       label images -> masks2d.DeviceRuns at the working resolution, no dense plane
    instance_masks_2d(geom, frame_ids, result, cfg)   the three in a row -> a mask_2d list (scene.prepare_scene and
                                                  masks2d.encode_2d_masks take it as it is)

Occlusion is decided by the cloud itself: the nearest point of a texel wins whether it belongs to an instance or not, and
at equal millimetres the smaller label (background first).  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .masks2d import MAX_PIXELS, DeviceRuns, _fetch_runs

MAX_LABEL = _lib.MAX_POINT_LABEL


def point_labels(rows, n_points, unsort=None, order=None):
    """rows: int64 [K][nw] instance bit rows in the caller's (original) point order, on the device.  -> int16 [n_points]
    holding uint16 labels: 1 + the first row that holds the point, 0 = background.  Priority is row order; `order`
    (indices, e.g. by descending confidence) reorders the rows first, and label L then names rows[order[L - 1]].
    unsort (DeviceScene.unsort / SceneGeometry.unsort): the labels come out in the sorted cloud's order."""
    if not torch.is_tensor(rows) or not rows.is_cuda:
        raise ValueError("point_labels takes device bit rows (no CPU path)")
    if order is not None:
        rows = rows[torch.as_tensor(order, dtype=torch.long, device=rows.device)]
    if rows.shape[0] > MAX_LABEL:
        raise ValueError(f"point_labels: {rows.shape[0]} instances, at most {MAX_LABEL}")
    return _lib.point_labels(rows.contiguous(), int(n_points), unsort)


def rendered_size(height, width, stride):
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"reproject stride must be an integer >= 1, got {stride}")
    return -(-int(height) // stride), -(-int(width) // stride)


def render_labels(geom, lab, inv_pose, stride=1, splat_radius=0.0, want_depth=False, frames_per_block=0,
                  scratch_texels=None):
    """geom: a scene.SceneGeometry or scene.DeviceScene (its sorted cloud, intrinsics, image size and culling table are
    used).  lab: point_labels(..., unsort=geom.unsort).  inv_pose: f64 [F][16] inverse poses (device tensor or array).
    -> int16 [F][ceil(H / stride)][ceil(W / stride)] label frames (uint16 values), or (labels, depth) with want_depth.
    The frames are rendered in runs of as many as the scratch holds (_lib.RENDER_SCRATCH_TEXELS)."""
    xyz = geom.xyz
    if not xyz.is_cuda:
        raise ValueError("render_labels needs a scene on a GPU device (there is no CPU renderer)")
    if not torch.is_tensor(inv_pose):
        inv_pose = torch.as_tensor(np.ascontiguousarray(inv_pose, dtype=np.float64).reshape(-1, 16))
    inv_pose = inv_pose.reshape(-1, 16).to(xyz.device).contiguous()
    dh, dw = rendered_size(geom.height, geom.width, stride)
    labels, depth = _lib.render_labels(xyz, geom.n_points, lab, inv_pose, np.asarray(geom.cam_intr, np.float64)[:3, :3],
                                       geom.height, geom.width, dh, dw, tile_bounds=geom.tile_bounds,
                                       frames_per_block=frames_per_block, scratch_texels=scratch_texels,
                                       splat_radius=float(splat_radius), want_depth=want_depth)
    return (labels, depth) if want_depth else labels


def label_runs(label_frames, height, width, min_pixels=1, n_labels: Optional[int] = None):
    """label_frames: int16 [F][dh][dw] (uint16 labels, 0 = none) on the device.  The image of frame f at the working
    resolution is up[v][u] = label_frames[f][(v * dh) // height][(u * dw) // width]; label L of frame f becomes a mask iff
    it covers at least max(1, min_pixels) pixels of it.  -> (masks2d.DeviceRuns with frame_offs, masks ordered by (f, L);
    mask_label int32 [n_masks] holding L - 1).  Neither `up` nor a dense mask is ever built: one count pass, one scan and
    one read-back (the totals and the per-frame mask counts), one emit pass, two library sorts.  n_labels: an upper bound
    of the labels (the number of instances); None = the frames' maximum, which costs a read-back of its own."""
    if not torch.is_tensor(label_frames) or not label_frames.is_cuda:
        raise ValueError("label_runs takes device label frames (no CPU path)")
    if label_frames.dtype != torch.int16 or label_frames.dim() != 3:
        raise TypeError("label_runs: int16 [F][dh][dw] label frames expected")
    height, width = int(height), int(width)
    if height * width > MAX_PIXELS:
        raise ValueError(f"label_runs: H*W = {height * width} pixels, at most 2^31 - 1")
    labels = label_frames.contiguous()
    dev, f = labels.device, int(labels.shape[0])
    i32, i64 = torch.int32, torch.int64
    with torch.cuda.device(dev):
        if n_labels is None:
            n_labels = int((labels.to(i32) & 0xFFFF).max().item()) if labels.numel() else 0
        n_labels = int(n_labels)
        if f == 0 or n_labels == 0:
            z = torch.zeros(0, dtype=i32, device=dev)
            return (DeviceRuns(z, z.clone(), torch.zeros(1, dtype=i32, device=dev), height * width, 0, [0] * (f + 1)),
                    z.clone())
        n_runs, n_pix = _lib.label_runs_count(labels, height, width, n_labels)
        keep = n_pix >= max(1, int(min_pixels))                              # [F][n_labels]
        flat = keep.reshape(-1)
        rank = torch.cumsum(flat, 0) - 1                                     # the mask (f, L) becomes, in (f, L) order
        runs64 = n_runs.reshape(-1).to(i64)
        head = torch.cat([keep.sum(1), (runs64 * flat).sum().reshape(1)])
        host = _fetch_runs(head)[0]                                          # the call's one read-back
        per_frame, total = host[:f].astype(np.int64), int(host[f])
        n_masks = int(per_frame.sum())
        if total >= 1 << 31:
            raise ValueError(f"label_runs: {total} runs in one call, at most 2^31 - 1 (encode fewer frames per call)")
        frame_offs = [0] + np.cumsum(per_frame).tolist()
        # compaction without a nonzero(): every dropped (f, L) writes to the spare slot n_masks
        slot = torch.where(flat, rank, torch.full_like(rank, n_masks))
        mask_runs = torch.zeros(n_masks + 1, dtype=i64, device=dev).scatter_(0, slot, runs64)[:n_masks]
        which = torch.arange(f * n_labels, device=dev) % n_labels
        mask_label = torch.zeros(n_masks + 1, dtype=i64, device=dev).scatter_(0, slot, which)[:n_masks].to(i32)
        offs = torch.zeros(n_masks + 1, dtype=i32, device=dev)
        offs[1:] = torch.cumsum(mask_runs, 0)
        if total == 0:
            z = torch.zeros(0, dtype=i32, device=dev)
            return DeviceRuns(z, z.clone(), offs, height * width, n_masks, frame_offs), mask_label
        mask_index = torch.where(flat, rank, torch.full_like(rank, -1)).to(i32).reshape(f, n_labels).contiguous()
        start_keys, end_keys = _lib.label_runs_emit(labels, height, width, mask_index, total)
        bits = min(64, 31 + max(1, n_masks.bit_length()))
        low = (1 << 31) - 1
        run_start = (start_keys[_lib.argsort_i64(start_keys, bits).long()] & low).to(i32)
        run_end = (end_keys[_lib.argsort_i64(end_keys, bits).long()] & low).to(i32)
    return DeviceRuns(run_start, run_end, offs, height * width, n_masks, frame_offs), mask_label


def reproject_stride(cfg) -> int:
    s = cfg.get("reproject_stride", 1)
    s = 1 if s is None else s
    if isinstance(s, bool) or int(s) != s or int(s) < 1:
        raise ValueError(f"reproject_stride must be an integer >= 1, got {s!r}")
    return int(s)


def reproject_splat_radius(cfg) -> float:
    r = cfg.get("reproject_splat_radius", 0.0)
    r = 0.0 if r is None else float(r)
    if not (r >= 0.0 and np.isfinite(r)):
        raise ValueError(f"reproject_splat_radius must be a finite number of metres >= 0, got {r!r}")
    return r


def reproject_min_pixels(cfg) -> int:
    m = cfg.get("reproject_min_pixels", 1)
    return max(1, int(1 if m is None else m))


def _frame_key(frame_id):
    """A frame's slot key ("1230") and colour file name ("1230.jpg") from either."""
    s = str(frame_id)
    return (s[:-4], s) if s.endswith(".jpg") else (s, s + ".jpg")


def instance_masks_2d(geom, frame_ids, result, cfg):
    """Render the instances of `result` (a Stage2Result / FinalResult: `rows` int64 [K][nw] in the original point order,
    `conf`, `final_class`) into the frames `frame_ids` of `geom` (a SceneGeometry holding those frames, or a DeviceScene
    that shares one).  -> a mask_2d list, one entry per frame in the given order:
        frame_id               the colour file name
        segmented_frame_masks  the frame's DeviceRuns view (the masks of the instances visible in it)
        confidences            those instances' `conf`
        labels                 those instances' `final_class`
        instance_ids           int64 tensor (host): which instance each mask renders
    Config keys: reproject_stride, reproject_splat_radius, reproject_min_pixels."""
    g = getattr(geom, "geometry", None) or geom
    if not hasattr(g, "slot"):
        raise ValueError("instance_masks_2d needs a SceneGeometry (or a DeviceScene prepared against one): it looks the "
                         "frames' poses up by frame id")
    keys = [_frame_key(fid) for fid in frame_ids]
    missing = [k for k, _ in keys if k not in g.slot]
    if missing:
        raise KeyError(f"scene {g.scene_id}: no pose resident for frames {missing[:5]}")
    dev = g.xyz.device
    rows = getattr(result, "rows", None)
    k = 0 if rows is None else int(rows.shape[0])
    classes = list(result.final_class)
    conf = result.conf
    conf = torch.as_tensor(conf).reshape(-1).cpu() if k and not isinstance(conf, (list, tuple)) else \
        (torch.stack([torch.as_tensor(c) for c in conf]).reshape(-1).cpu() if k else torch.zeros(0, dtype=torch.float16))
    if k and not (len(classes) == k and conf.shape[0] == k):
        raise ValueError(f"scene {g.scene_id}: {k} instance rows, {len(classes)} classes, {conf.shape[0]} confidences")
    if k == 0 or not keys:
        runs, mask_label = label_runs(torch.zeros((len(keys), 1, 1), dtype=torch.int16, device=dev), g.height, g.width, 1, 0)
    else:
        lab = point_labels(rows.to(dev), g.n_points, g.unsort)
        inv = g.inv_pose_host[np.array([g.slot[key] for key, _ in keys], dtype=np.int64)]
        frames = render_labels(g, lab, inv, reproject_stride(cfg), reproject_splat_radius(cfg))
        runs, mask_label = label_runs(frames, g.height, g.width, reproject_min_pixels(cfg), k)
    ids = torch.from_numpy(_fetch_runs(mask_label)[0].astype(np.int64)) if len(runs) else torch.zeros(0, dtype=torch.int64)
    out = []
    for (_, name), view, a, b in zip(keys, runs.frames(), runs.frame_offs[:-1], runs.frame_offs[1:]):
        inst = ids[a:b]
        out.append({"frame_id": name, "segmented_frame_masks": view, "confidences": conf[inst],
                    "labels": [classes[i] for i in inst.tolist()], "instance_ids": inst})
    return out


def geometry_for_frames(scene, cfg, frame_ids, device="cuda"):
    """A SceneGeometry that holds the sorted cloud, the intrinsics and the inverse poses of `frame_ids` and NO depth:
    what rendering instances into views needs (scene: SceneInputs-like; only points, cam_intr and poses are read)."""
    from .scene import cloud_host_layout, new_geometry
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("reprojection needs a GPU device (there is no CPU renderer)")
    ids = [_frame_key(f)[0] for f in frame_ids]
    soa, perm, unsort, n, _ = cloud_host_layout(scene.points, True)
    inv = np.stack([np.linalg.inv(np.asarray(scene.poses[f], dtype=np.float64)).reshape(16) for f in ids]) if ids \
        else np.zeros((0, 16))
    xyz = torch.as_tensor(soa).to(dev)
    bounds = _lib.point_tile_bounds(xyz, n) if n else None
    t32 = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    return new_geometry(scene, int(cfg.height_2d), int(cfg.width_2d), n, ids, inv, 0, xyz, (None, None, None), bounds,
                        t32(unsort), t32(perm))
