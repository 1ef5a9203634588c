"""The frames that see a 3-D instance best, and the boxes to cut it out of them, on the device (include/bff_hip.h:
bff_instance_views, bff_select_views).

Every stage stops at 3-D instances.  What describes one -- CLIP crops, captions, thumbnails -- is cut out of the colour
frames in which the instance is really seen: unoccluded, and by the most points.  The scene's visibility table
(_lib.visibility_table) already answers per (frame, point) whether the REAL depth frame confirms the point, and at which
pixel; it depends on no mask and no class.  Here it is read from the instances' side:

    instance_views(table, rows_sorted, n_points, height, width)   per (instance, slot): confirmed points and their pixel box
    select_views(visible, box, height, width, top_k, ...)         per instance: the top_k slots and their crops at every level
    scene_views(geom, result, cfg, frame_ids=None, ...)           the two in a row for a stage's result -> the tool's dict

For instance k and slot f, S(k, f) = the points of row k that are visible in f.  visible = |S|; box = (min u, min v, max u,
max v) of their pixels, inclusive, (W, H, -1, -1) when S is empty.  The candidates of k are the slots with visible >=
max(1, views_min_points), by visible descending, ties to the earlier slot; past them top holds -1, top_visible 0 and the
crops (W, H, -1, -1).  Crop level l of a view with box (u0, v0, u1, v1) and r = views_crop_expand:
    ex = (int)floor((double)(u1 - u0) * r) * l,  ey likewise;  (max(0, u0 - ex), max(0, v0 - ey), min(W - 1, u1 + ex), min(H - 1, v1 + ey))
tests/views_ref.py restates all of it in NumPy.  The defaults (views_top_k 5, views_crop_levels 3, views_crop_expand 0.1,
views_min_points 1) are OpenMask3D's and untuned here.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, instances3d
from ._lib import i32, i64
from .scene import DEPTH_THRESH

MAX_TOP_K = 64
MAX_LEVELS = 8


# ------------------------------------------------------------------ config
def views_top_k(cfg) -> int:
    t = instances3d.positive_int("views_top_k", cfg.get("views_top_k"), 5)
    if t > MAX_TOP_K:
        raise ValueError(f"views_top_k must be an integer in 1 .. {MAX_TOP_K}, got {t!r}")
    return t


def views_min_points(cfg) -> int:
    return instances3d.positive_int("views_min_points", cfg.get("views_min_points"), 1)


def views_crop_levels(cfg) -> int:
    n = instances3d.positive_int("views_crop_levels", cfg.get("views_crop_levels"), 3)
    if n > MAX_LEVELS:
        raise ValueError(f"views_crop_levels must be an integer in 1 .. {MAX_LEVELS}, got {n!r}")
    return n


def views_crop_expand(cfg) -> float:
    r = cfg.get("views_crop_expand")
    r = 0.1 if r is None else r
    if not instances3d._is_number(r) or not (float(r) >= 0.0 and np.isfinite(float(r))):      # NaN fails the comparison
        raise ValueError(f"views_crop_expand must be a finite number >= 0, got {r!r}")
    return float(r)


def check_config(cfg):
    """Every views_* value of the config, so that a bad one stops a run before anything is loaded."""
    return dict(top_k=views_top_k(cfg), min_points=views_min_points(cfg), levels=views_crop_levels(cfg),
                expand=views_crop_expand(cfg))


# ------------------------------------------------------------------ the two kernels
def _table_parts(table):
    """(vis_mask, vis_off, vis_pix, n_pixels) of a projection.VisibilityTable or of _lib.visibility_table(..., with_count=True)."""
    if hasattr(table, "mask") and hasattr(table, "pix"):
        # a table without a pair keeps one element of vis_pix that no offset leads to
        return table.mask, table.off, table.pix, int(table.pix.shape[0])
    if isinstance(table, (tuple, list)) and len(table) == 4:
        return table[0], table[1], table[2], int(table[3])
    raise TypeError("instance_views: a projection.VisibilityTable or (vis_mask, vis_off, vis_pix, n_pairs) expected")


def instance_views(table, rows_sorted, n_points, height, width):
    """table: the scene's visibility table; rows_sorted: int64 [K][>= ceil(n_points / 64)] instance bit rows in the SORTED
    point order (the table's), padding bits zero.  -> (visible int32 [K][F], box int32 [K][F][4]) on the device."""
    mask, off, pix, n_pixels = _table_parts(table)
    rows = rows_sorted
    if not torch.is_tensor(rows) or not rows.is_cuda or not mask.is_cuda:
        raise ValueError("instance_views takes device bit rows and a device table (no CPU path)")
    if rows.dtype != i64 or rows.dim() != 2:
        raise TypeError("instance_views: int64 [K][nw] bit rows expected")
    n = int(n_points)
    nw = (n + 63) // 64
    if n < 0 or int(rows.shape[1]) < nw:
        raise ValueError(f"instance_views: rows of {int(rows.shape[1])} words for {n} points")
    if mask.dim() != 2 or int(mask.shape[1]) < nw or mask.shape != off.shape:
        raise ValueError(f"instance_views: a table of {tuple(mask.shape)} words for {n} points")
    if mask.device != rows.device:
        raise ValueError("instance_views: the rows and the table live on different devices")
    if int(rows.shape[1]) != nw:
        rows = rows[:, :nw]
    with torch.cuda.device(rows.device):
        return _lib.instance_views(rows.contiguous(), (mask, off, pix), min(n_pixels, int(pix.shape[0])), int(height), int(width))


def select_views(visible, box, height, width, top_k=5, min_points=1, levels=3, expand=0.1):
    """visible int32 [K][F] and box int32 [K][F][4] of instance_views -> (top int32 [K][top_k], top_visible int32
    [K][top_k], crops int32 [K][top_k][levels][4]) on the device."""
    if not torch.is_tensor(visible) or not visible.is_cuda or not torch.is_tensor(box) or not box.is_cuda:
        raise ValueError("select_views takes device tensors (no CPU path)")
    if visible.dtype != i32 or box.dtype != i32 or visible.dim() != 2 or tuple(box.shape) != tuple(visible.shape) + (4,):
        raise TypeError("select_views: visible int32 [K][F] and box int32 [K][F][4] expected")
    cfg = dict(views_top_k=top_k, views_min_points=min_points, views_crop_levels=levels, views_crop_expand=expand)
    c = check_config(cfg)
    with torch.cuda.device(visible.device):
        return _lib.select_views(visible.contiguous(), box.contiguous(), int(height), int(width), c["top_k"], c["min_points"],
                                 c["levels"], c["expand"])


# ------------------------------------------------------------------ a scene
def _frame_key(frame_id):
    s = str(frame_id)
    return (s[:-4], s) if s.endswith(".jpg") else (s, s + ".jpg")


def _resident_table(g, key, dev):
    """The geometry's own table for the threshold, if projection.scene_visibility has built one over the geometry's slots;
    the current stream is ordered behind its build as scene_visibility does it."""
    from .projection import VisibilityTable
    tab = g.__dict__.get("_vis_tables", {}).get(key)
    if not isinstance(tab, VisibilityTable) or int(tab.mask.shape[0]) != len(g.frame_ids):
        return None
    raw = _lib.raw_stream()
    if raw not in tab.streams:
        st = torch.cuda.current_stream(dev)
        st.wait_event(tab.ready)
        for t in tab.tensors():
            t.record_stream(st)
        tab.streams.add(raw)
    return tab


def _group_views(g, rows, slots, key, dev, poses):
    """visible / box of `rows` over the geometry's depth slots `slots` (a list), from a table built for them alone, or
    None where that table would exceed projection.vis_table_max_bytes() and the group can still be halved."""
    from .projection import vis_table_max_bytes
    whole = slots == list(range(len(g.frame_ids)))
    idx = torch.as_tensor(np.asarray(slots, dtype=np.int64)).to(dev)
    depth = g.sweep_depth if whole else g.sweep_depth[idx].contiguous()
    got = _lib.visibility_table(g.xyz, g.n_points, poses[idx].contiguous(), g.cam_intr, depth, g.height, g.width, key,
                                g.tile_bounds, depth_size=g.depth_size,
                                max_bytes=vis_table_max_bytes() if len(slots) > 1 else None, with_count=True)
    if got is None:
        return None
    return instance_views(got, rows, g.n_points, g.height, g.width)


def scene_views(geom, result, cfg, frame_ids=None, depth_thresh=DEPTH_THRESH):
    """The views of the instances of `result` (a Stage2Result / FinalResult or cli._saved_instances' namespace: `rows` int64
    [K][nw] in the ORIGINAL point order, as reproject.instance_masks_2d takes them) among the frames `frame_ids` of `geom`
    (a SceneGeometry that holds their poses and depth, e.g. scene.geometry_for_depth_frames, or a DeviceScene that shares
    one; None = all of the geometry's frames, in slot order).  -> the dict tools/select_views_3d.py saves (host tensors):
        frame_ids    the colour file names; a position in this list is what `top` holds
        area         int32 [K]  points of each instance
        visible      int32 [K][F], boxes int32 [K][F][4], top int32 [K][T], top_visible int32 [K][T], crops int32 [K][T][L][4]
        height, width, depth_thresh
    A table the geometry already holds for the threshold (projection.scene_visibility) is read as it is; otherwise one is
    built over the frames asked for -- in groups of slots where the whole would exceed projection.vis_table_max_bytes(),
    which changes no result.  Config keys: views_top_k, views_min_points, views_crop_levels, views_crop_expand."""
    c = check_config(cfg)
    g = getattr(geom, "geometry", None) or geom
    if not hasattr(g, "slot") or g.sweep_depth is None:
        raise ValueError("scene_views needs a SceneGeometry with depth frames (or a DeviceScene prepared against one)")
    dev = g.xyz.device
    if dev.type != "cuda":
        raise ValueError("scene_views needs a scene on a GPU device (no CPU path)")
    keys = [_frame_key(f) for f in (g.frame_ids if frame_ids is None else frame_ids)]
    missing = [k for k, _ in keys if k not in g.slot]
    if missing:
        raise KeyError(f"scene {g.scene_id}: no depth frame resident for frames {missing[:5]}")
    slots = [g.slot[k] for k, _ in keys]
    n, nw, h, w = g.n_points, (g.n_points + 63) // 64, g.height, g.width
    rows = getattr(result, "rows", None)
    k = 0 if rows is None else int(rows.shape[0])
    f, key = len(slots), float(depth_thresh)
    with torch.cuda.device(dev):
        if k == 0:
            rows = torch.zeros((0, nw), dtype=i64, device=dev)
        else:
            if not torch.is_tensor(rows) or rows.dtype != i64 or rows.dim() != 2 or int(rows.shape[1]) < nw:
                raise TypeError(f"scene_views: int64 [K][>= {nw}] bit rows expected")
            rows = rows.to(dev)[:, :nw].contiguous()
            if g.perm is not None and n:
                rows = _lib.permute_bits(rows, g.perm, n)             # bit s of the sorted row = bit perm[s] of the original
        area = _lib.popcount_rows(rows) if k and nw else torch.zeros(k, dtype=i32, device=dev)
        visible = torch.zeros((k, f), dtype=i32, device=dev)
        box = torch.tensor([w, h, -1, -1], dtype=i32, device=dev).repeat(k, f, 1)
        if k and f and n:
            at = torch.as_tensor(np.asarray(slots, dtype=np.int64)).to(dev)
            tab = _resident_table(g, key, dev)
            if tab is not None:
                vis_all, box_all = instance_views(tab, rows, n, h, w)
                visible, box = vis_all[:, at].contiguous(), box_all[:, at].contiguous()
            else:
                from .projection import vis_table_max_bytes
                poses = torch.as_tensor(np.ascontiguousarray(g.inv_pose_host, dtype=np.float64).reshape(-1, 16)).to(dev)
                per_slot = sum(_lib.visibility_table_bytes(n, 1))
                size = max(1, min(f, vis_table_max_bytes() // max(per_slot, 1)))
                done, parts = 0, []
                while done < f:
                    got = _group_views(g, rows, slots[done:done + size], key, dev, poses)
                    if got is None:                                   # the pixels did not fit: a smaller group
                        size = max(1, size // 2)
                        continue
                    parts.append(got)
                    done += size
                visible = torch.cat([p[0] for p in parts], dim=1).contiguous()
                box = torch.cat([p[1] for p in parts], dim=1).contiguous()
        top, top_visible, crops = _lib.select_views(visible, box, h, w, c["top_k"], c["min_points"], c["levels"], c["expand"])
        host = _lib.fetch(area, visible, box, top, top_visible, crops)      # the call's one read-back
    out = dict(zip(("area", "visible", "boxes", "top", "top_visible", "crops"), (torch.from_numpy(a) for a in host)))
    out.update(frame_ids=[name for _, name in keys], height=int(h), width=int(w), depth_thresh=key)
    return out
