"""3-D instances lifted from a subsampled cloud to the full cloud, on the device (include/bff_hip.h: bff_nn_search,
bff_rows_to_columns, bff_lift_bits).

Everything the projection stage costs scales with the points of <scene>.npy, and beyond 2 097 152 of them a scene is
rejected.  The way round: run on a voxel subsample, carry every instance back to the full cloud by nearest neighbour,
refine and score at full resolution -- a pure function of the inputs, independent of thread schedule and run:

    subsample(points, voxel)                      the smallest point index of every occupied cell, ascending
    nearest_index(source_points, max_dist)        the search index of a source cloud: its grid at cell = max_dist, the
                                                  points of every cell, the cloud gathered into that order
    nearest(index, query_points)                  per query the nearest source point within max_dist, -1 = none
    lift_rows(nn, rows, n_source, n_target)       bit rows over the source -> bit rows over the target
    lift_instances(nn, result, n_source, n_target)
                                                  a FinalResult / Stage2Result / saved-file namespace with `rows` replaced

The statement is the header's; tests/lift_ref.py restates it in NumPy.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib, instances3d, spatial, superpoints
from ._lib import _ptr, call, f64, i32, i64


@dataclasses.dataclass
class NearestIndex:
    max_dist: float
    n_source: int
    grid: spatial.VoxelGrid        # the source cloud's grid at cell = max_dist
    order: torch.Tensor            # int32 [M'] (device): the source points with a cell, by (cell, point)
    offs: torch.Tensor             # int32 [V + 1] (device): cell v is order[offs[v] : offs[v + 1]]
    cloud: torch.Tensor            # float64 [M'][3] (device): source_points[order]


def subsample_voxel(cfg) -> float:
    return instances3d.config_metres(cfg, "subsample_voxel")


def lift_max_dist(cfg) -> float:
    """Absent: 2 x subsample_voxel (every finite point of the cloud the subsample was taken from has a source once the
    radius reaches sqrt(3) x subsample_voxel)."""
    if cfg.get("lift_max_dist") is None:
        if cfg.get("subsample_voxel") is None:
            raise ValueError("lift_max_dist is not set in the config, and neither is subsample_voxel (metres, > 0)")
        return 2.0 * subsample_voxel(cfg)
    return instances3d.config_metres(cfg, "lift_max_dist")


def subsample(points, voxel, device="cuda") -> torch.Tensor:
    """points: the (N, >= 3) array of <scene>.npy, or a float64 device tensor of that shape.  -> sample int32 [V] on the
    device: the smallest point index of every occupied cell of spatial.voxel_grid(points, voxel), in ascending point
    index.  A non-finite point has no cell and is never sampled."""
    voxel = instances3d.metres("subsample: voxel", voxel)
    pts = instances3d.device_points("subsample", points, device)
    grid = spatial.voxel_grid(pts, voxel)
    dev, n, v = pts.device, grid.n_points, grid.n_voxels
    if v == 0:
        return torch.zeros(0, dtype=i32, device=dev)
    with torch.cuda.device(dev):
        idx = torch.arange(n, dtype=i64, device=dev)
        has = grid.vox >= 0
        first = torch.full((v,), n, dtype=i64, device=dev)
        first.scatter_reduce_(0, grid.vox[has].long(), idx[has], "amin")        # a minimum: the same on every run
        mark = torch.zeros(n, dtype=torch.bool, device=dev)
        mark[first] = True
        return torch.nonzero(mark).reshape(-1).to(i32)


def nearest_index(source_points, max_dist, device="cuda") -> NearestIndex:
    """source_points: an (M, >= 3) array or a float64 device tensor of that shape; max_dist: metres, > 0 and finite.  The
    index serves every query set."""
    r = instances3d.metres("nearest_index: max_dist", max_dist)
    pts = instances3d.device_points("nearest_index", source_points, device)
    grid = spatial.voxel_grid(pts, r)
    cells = superpoints.superpoints_from_grid(grid)                           # the cells' point lists, ascending index
    with torch.cuda.device(pts.device):
        cloud = pts[cells.order.long(), :3].contiguous()
    return NearestIndex(r, int(pts.shape[0]), grid, cells.order, cells.offs, cloud)


def nearest(index: NearestIndex, query_points, return_d2=False):
    """query_points: an (N, >= 3) array or a float64 device tensor of that shape.  -> nn int32 [N] on the device (the
    nearest source point within the index's max_dist, a tie to the smallest index, -1 = none), with return_d2 also
    d2 float64 [N] (the squared distance, +inf = none)."""
    dev = index.cloud.device
    q = instances3d.device_points("nearest", query_points, dev)
    if q.device != dev:
        raise ValueError("nearest: the queries and the index live on different devices")
    n, v, grid = int(q.shape[0]), index.grid.n_voxels, index.grid
    with torch.cuda.device(dev):
        nn = torch.empty(n, dtype=i32, device=dev)
        d2 = torch.empty(n, dtype=f64, device=dev) if return_d2 else None
        lo = np.ascontiguousarray(grid.lo, dtype=np.float64)
        call("bff_nn_search", _ptr(index.cloud) if v else None, _ptr(grid.keys) if v else None, _ptr(index.offs, i32) if v else None,
             _ptr(index.order, i32) if v else None, v, int(index.cloud.shape[0]), lo.ctypes.data if v else None, grid.cell,
             index.max_dist, _ptr(q) if n else None, n, int(q.shape[1]), _ptr(nn) if n else None, _ptr(d2) if n and return_d2 else None)
    return (nn, d2) if return_d2 else nn


def lift_rows(nn, rows, n_source, n_target) -> torch.Tensor:
    """nn: int32 [n_target] on the device; rows: int64 [K][nw] bit rows over the n_source source points, on the device
    (bits at positions >= n_source are ignored).  -> int64 [K][ceil(n_target / 64)]: bit p of row k = bit nn[p] of input
    row k, 0 where nn[p] is not a source point; bits at positions >= n_target are zero."""
    if not torch.is_tensor(rows) or not rows.is_cuda or not torch.is_tensor(nn) or not nn.is_cuda:
        raise ValueError("lift_rows takes device bit rows and a device nn (no CPU path)")
    if rows.dtype != i64 or rows.dim() != 2:
        raise TypeError("lift_rows: int64 [K][nw] bit rows expected")
    if nn.dtype != i32 or nn.dim() != 1:
        raise TypeError("lift_rows: int32 [n_target] nn expected")
    m, n = int(n_source), int(n_target)
    if m < 0 or n != int(nn.shape[0]):
        raise ValueError(f"lift_rows: nn of {int(nn.shape[0])} entries for {n} target points")
    rows, nn = rows.contiguous(), nn.contiguous()
    k, nw, dev = int(rows.shape[0]), int(rows.shape[1]), rows.device
    if nw < (m + 63) // 64:
        raise ValueError(f"lift_rows: rows of {nw} words for {m} points")
    if nn.device != dev:
        raise ValueError("lift_rows: the rows and nn live on different devices")
    kw = (k + 63) // 64
    with torch.cuda.device(dev):
        out = torch.empty((k, (n + 63) // 64), dtype=i64, device=dev)
        if k == 0 or n == 0:
            return out
        cols = torch.empty((m, kw), dtype=i64, device=dev)                   # the rows transposed: scratch of this call
        call("bff_rows_to_columns", _ptr(rows), k, nw, m, _ptr(cols) if m else None)
        call("bff_lift_bits", _ptr(cols) if m else None, m, k, _ptr(nn), n, _ptr(out))
    return out


def lift_instances(nn, result, n_source, n_target):
    """result: a FinalResult, a Stage2Result or the namespace cli._saved_instances returns (`rows` int64 [K][nw] over the
    source cloud, `conf`, `final_class`).  -> the same kind with `rows` replaced by the rows over the target cloud; `conf`,
    `final_class`, the row count and the order are untouched, rows that end up empty included (`n_points`, where the result
    has it, becomes n_target).  A result whose rows is None comes back as it is."""
    rows = getattr(result, "rows", None)
    if rows is None:
        return result
    return instances3d.replace_rows(result, lift_rows(nn, rows, n_source, n_target), n_points=n_target)
