"""3-D instances split into spatially connected parts, on the device (include/bff_hip.h: bff_voxel_*, bff_split_*;
DESIGN.md section 7g).

An instance is a bit row over the cloud, assembled from votes and IoU components; nothing keeps it in one piece.  Here
the cloud is binned into a voxel grid once per scene and every row is cut into the classes of 26-adjacency between its
occupied cells -- a pure function of the inputs, independent of point order, thread schedule and run:

    voxel_grid(points, cell)                      the grid of a scene: cell ranks per point, the distinct keys, the 13
                                                  forward neighbours of every cell
    split_rows(grid, rows, n_points, ...)         bit rows -> the parts' bit rows, the parent row and the points of each
    split_instances(grid, result, cfg)            a FinalResult / Stage2Result / saved-file namespace with `rows` replaced,
                                                  `conf` and `final_class` taken from each part's parent

The statement is the header's; tests/spatial_ref.py restates it in NumPy.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib, instances3d
from ._lib import _ptr, call, i32, i64
from .instances3d import KEPT_FIRST_READ, _take  # noqa: F401  (importable under their names here)

MAX_AXIS_CELLS = 1 << 21
MODES = ("split", "largest")


@dataclasses.dataclass
class VoxelGrid:
    cell: float
    lo: np.ndarray                 # float64 [3], the minimum over the finite points (NaN without one)
    n_points: int
    n_voxels: int
    vox: torch.Tensor              # int32 [N] (device): the rank of the point's cell, -1 for a non-finite point
    keys: torch.Tensor             # int64 [V] (device): the distinct cell keys, ascending
    nbr: torch.Tensor              # int32 [V][13] (device): the forward neighbours' ranks, -1 = none


def _decode_box(box):
    """bff_voxel_bounds' order-preserving integers -> (lo, hi) float64 [3] each, or None without a finite point."""
    u = box.cpu().numpy().view(np.uint64)
    if u[0] == np.uint64(0xFFFFFFFFFFFFFFFF):
        return None
    top = np.uint64(1) << np.uint64(63)
    bits = np.where(u >> np.uint64(63), u ^ top, ~u)
    d = bits.view(np.float64)
    return d[:3].copy(), d[3:].copy()


def voxel_grid(points, cell, device="cuda") -> VoxelGrid:
    """points: the (N, >= 3) array of <scene>.npy (x, y, z first), or a float64 device tensor of that shape.  cell: metres,
    > 0 and finite.  Two read-backs (the box, the number of cells); the grid serves every class and call of the scene."""
    cell = instances3d.metres("voxel_grid: cell", cell)
    pts = instances3d.device_points("voxel_grid", points, device)
    dev, n, stride = pts.device, int(pts.shape[0]), int(pts.shape[1])
    with torch.cuda.device(dev):
        empty = lambda: VoxelGrid(cell, np.full(3, np.nan), n, 0, torch.full((n,), -1, dtype=i32, device=dev),
                                  torch.zeros(0, dtype=i64, device=dev), torch.zeros((0, 13), dtype=i32, device=dev))
        if n == 0:
            return empty()
        box = torch.empty(6, dtype=i64, device=dev)
        call("bff_voxel_bounds", _ptr(pts), n, stride, _ptr(box))
        lo_hi = _decode_box(box)                                              # read-back: the box
        if lo_hi is None:
            return empty()
        lo, hi = lo_hi
        key = torch.empty(n, dtype=i64, device=dev)
        call("bff_voxel_keys", _ptr(pts), n, stride, lo.ctypes.data, hi.ctypes.data, cell, _ptr(key))
        order = _lib.argsort_i64(key, 63)
        sorted_keys = key[order.long()]
        head = torch.empty(n, dtype=i32, device=dev)
        call("bff_voxel_heads", _ptr(sorted_keys), n, _ptr(head))
        incl = torch.cumsum(head, 0, dtype=i64)
        v = int(incl[-1].item())                                              # read-back: the number of cells
        vox = torch.empty(n, dtype=i32, device=dev)
        keys = torch.empty(v, dtype=i64, device=dev)
        call("bff_voxel_ranks", _ptr(sorted_keys), _ptr(order, i32), _ptr(incl), n, v, _ptr(vox), _ptr(keys) if v else None)
        nbr = torch.empty((v, 13), dtype=i32, device=dev)
        call("bff_voxel_neighbours", _ptr(keys) if v else None, v, _ptr(nbr) if v else None)
    return VoxelGrid(cell, lo, n, v, vox, keys, nbr)


def split_voxel(cfg) -> float:
    return instances3d.config_metres(cfg, "split_voxel")


def split_min_points(cfg) -> int:
    return instances3d.positive_int("split_min_points", cfg.get("split_min_points"), 1)


def split_mode(cfg) -> str:
    return instances3d.one_of("split_mode", cfg.get("split_mode"), MODES, "split")


def voxel_grid_for(geom_or_scene, cfg, device="cuda") -> VoxelGrid:
    """The grid of a scene at the config's split_voxel.  geom_or_scene: anything with `points` in the caller's order (a
    SceneInputs), a resident scene (SceneGeometry / DeviceScene: its sorted cloud is put back into the original point
    order through `unsort`), or the array itself."""
    cell = split_voxel(cfg)
    points = getattr(geom_or_scene, "points", None)
    if points is not None:
        return voxel_grid(points, cell, device)
    xyz = getattr(geom_or_scene, "xyz", None)
    if torch.is_tensor(xyz):                                                # f64 [3][n_pad], sorted
        unsort = getattr(geom_or_scene, "unsort", None)
        cloud = xyz[:, :int(geom_or_scene.n_points)] if unsort is None else xyz[:, unsort.long()]
        return voxel_grid(cloud.t().contiguous(), cell)
    return voxel_grid(geom_or_scene, cell, device)


def split_rows(grid: VoxelGrid, rows, n_points, min_points=1, mode="split"):
    """rows: int64 [K][nw] bit rows in the grid's point order, on the device; bits at positions >= n_points are ignored.
    -> (rows_out int64 [R][nw] on the device, parent int64 [R], points int64 [R]; the two lists are decided on the host and
    stay there).  mode "split": every component with >= min_points points, by (parent, points descending, anchor);
    "largest": per parent only the first of those.  Two read-backs: the element counts of the rows, then the kept
    components (past KEPT_FIRST_READ of them a third fetches the rest)."""
    rows, k, nw, n, dev = instances3d.check_rows("split_rows", rows, n_points, grid.n_points, "grid", grid.vox)
    instances3d.one_of("split_rows: mode", mode, MODES)
    min_points, v = instances3d.positive_int("split_rows: min_points", min_points), grid.n_voxels
    none = lambda: instances3d.no_rows(nw, dev)
    if k == 0 or n == 0 or v == 0:
        return none()
    vw = (v + 63) // 64
    with torch.cuda.device(dev):
        occ = torch.empty((k, vw), dtype=i64, device=dev)
        prefix = torch.empty((k, vw), dtype=i32, device=dev)
        elem_offs = torch.zeros(k + 1, dtype=i32, device=dev)
        row_total = torch.empty(k, dtype=i32, device=dev)
        head = (_ptr(rows), k, nw, n, _ptr(grid.vox, i32), v, _ptr(occ), _ptr(prefix))
        call("bff_split_occupancy", *head, _ptr(row_total))
        elem_offs[1:] = torch.cumsum(row_total, 0)
        offs = elem_offs.cpu().numpy().astype(np.int64)                       # read-back 1: the rows' element counts
        t = int(offs[k])
        if t == 0:
            return none()
        parent = torch.empty(t, dtype=i32, device=dev)
        call("bff_split_union", _ptr(occ), _ptr(prefix), _ptr(elem_offs), k, v, _ptr(grid.nbr, i32), t, _ptr(parent))
        return instances3d.emit_kept(head, elem_offs, offs, parent, t, min_points, mode, nw) or none()


def split_instances(grid: VoxelGrid, result, cfg):
    """result: a FinalResult, a Stage2Result or the namespace cli._saved_instances returns (`rows` int64 [K][nw] in the
    original point order, `conf`, `final_class`).  -> the same kind with `rows` replaced by the parts and `conf`,
    `final_class` taken from each part's parent, plus the attribute `parent` (int64 [R], host).  A result whose rows is
    None comes back as it is.  Config keys: split_min_points, split_mode (split_voxel made the grid)."""
    rows = getattr(result, "rows", None)
    if rows is None:
        return result
    out_rows, parent, _ = split_rows(grid, rows, grid.n_points, split_min_points(cfg), split_mode(cfg))
    return instances3d.replace_rows(result, out_rows, parent)
