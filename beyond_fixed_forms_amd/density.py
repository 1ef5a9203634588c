"""3-D instances clustered by density, on the device: DBSCAN(eps, min_samples) with a deterministic border rule
(include/bff_hip.h: bff_dbscan_*).

The split (spatial.py) links whole voxel cells: a cell with one point links like a cell with fifty, and no distance in
metres is looked at.  Here every instance is cut by density instead -- core points, their eps-connected clusters, border
points to their nearest core neighbour, noise dropped -- a pure function of the inputs, independent of point order,
thread schedule and run:

    density_index(points, eps)                    the search index of a scene: lift.nearest_index of the cloud at a cell
                                                  a hair above eps, the cloud itself, the bit row of the finite points
    cluster_rows(index, rows, n_points, ...)      bit rows -> the clusters' bit rows, the parent row and the points of each
    cluster_instances(index, result, cfg)         a FinalResult / Stage2Result / saved-file namespace with `rows` replaced,
                                                  `conf` and `final_class` taken from each cluster's parent

The statement is the header's; tests/density_ref.py restates it in NumPy.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib, instances3d, lift, spatial
from ._lib import _ptr, call, i32, i64

MODES = spatial.MODES
CELL_SLACK = 1.0 + 2.0 ** -20      # the grid's cell over eps: neighbours never sit two cells apart (the header says why)


@dataclasses.dataclass
class DensityIndex:
    eps: float
    n_points: int
    nearest: lift.NearestIndex     # the cloud's grid at cell = eps * CELL_SLACK, the points of every cell, the gathered cloud
    points: torch.Tensor           # float64 [N][>= 3] (device): the cloud in the caller's order
    finite: torch.Tensor           # int64 [ceil(N / 64)] (device): bit p = point p has a cell
    ident: torch.Tensor            # int32 [N] (device): p for a point with a cell, -1 for the others


def density_index(points, eps, device="cuda") -> DensityIndex:
    """points: the (N, >= 3) array of <scene>.npy (x, y, z first), or a float64 device tensor of that shape.  eps: metres,
    > 0 and finite.  The index serves every class, row set and min_samples of the scene."""
    eps = instances3d.metres("density_index: eps", eps)
    pts = instances3d.device_points("density_index", points, device)
    nearest = lift.nearest_index(pts, eps * CELL_SLACK)
    n = int(pts.shape[0])
    with torch.cuda.device(pts.device):
        has = nearest.grid.vox >= 0
        finite = _lib.pack_rows(has.reshape(1, n)).reshape(-1) if n else torch.zeros(0, dtype=i64, device=pts.device)
        ident = torch.where(has, torch.arange(n, dtype=i32, device=pts.device), torch.full_like(nearest.grid.vox, -1))
    return DensityIndex(eps, n, nearest, pts, finite, ident)


def cluster_eps(cfg) -> float:
    return instances3d.config_metres(cfg, "cluster_eps")


def cluster_min_samples(cfg) -> int:
    return instances3d.positive_int("cluster_min_samples", cfg.get("cluster_min_samples"))


def cluster_min_points(cfg) -> int:
    return instances3d.positive_int("cluster_min_points", cfg.get("cluster_min_points"), 1)


def cluster_mode(cfg) -> str:
    return instances3d.one_of("cluster_mode", cfg.get("cluster_mode"), MODES, "split")


def cluster_rows(index: DensityIndex, rows, n_points, min_samples, min_points=1, mode="split"):
    """rows: int64 [K][nw] bit rows in the index's point order, on the device; bits at positions >= n_points are ignored.
    -> (rows_out int64 [R][nw] on the device, parent int64 [R], points int64 [R]; the two lists are decided on the host and
    stay there).  mode "split": every cluster with >= min_points points, by (parent, points descending, anchor);
    "largest": per parent only the first of those.  Two read-backs, as spatial.split_rows: the element counts of the
    rows, then the kept clusters."""
    rows, k, nw, n, dev = instances3d.check_rows("cluster_rows", rows, n_points, index.n_points, "index", index.points)
    instances3d.one_of("cluster_rows: mode", mode, MODES)
    min_samples = instances3d.positive_int("cluster_rows: min_samples", min_samples)
    min_points = instances3d.positive_int("cluster_rows: min_points", min_points)
    near, grid, vw = index.nearest, index.nearest.grid, (n + 63) // 64
    v = grid.n_voxels
    none = lambda: instances3d.no_rows(nw, dev)
    if k == 0 or n == 0 or v == 0:
        return none()
    lo = np.ascontiguousarray(grid.lo, dtype=np.float64)
    search = (_ptr(index.points), int(index.points.shape[1]), _ptr(near.cloud), _ptr(grid.keys), _ptr(near.offs, i32),
              _ptr(near.order, i32), v, int(near.cloud.shape[0]), lo.ctypes.data, grid.cell, index.eps)
    with torch.cuda.device(dev):
        elems = torch.empty((k, vw), dtype=i64, device=dev)                   # rows & finite: the elements
        prefix = torch.empty((k, vw), dtype=i32, device=dev)
        elem_offs = torch.zeros(k + 1, dtype=i32, device=dev)
        row_total = torch.empty(k, dtype=i32, device=dev)
        call("bff_dbscan_elements", _ptr(rows), k, nw, n, _ptr(index.finite), _ptr(elems), _ptr(prefix), _ptr(row_total))
        core = torch.empty((k, vw), dtype=i64, device=dev)
        call("bff_dbscan_core", _ptr(elems), k, n, *search, min_samples, _ptr(core))     # needs no read-back: queued first
        elem_offs[1:] = torch.cumsum(row_total, 0)
        offs = elem_offs.cpu().numpy().astype(np.int64)                       # read-back 1: the rows' element counts
        t = int(offs[k])
        if t == 0:
            return none()
        parent = torch.empty(t, dtype=i32, device=dev)
        call("bff_dbscan_link", _ptr(elems), _ptr(core), _ptr(prefix), _ptr(elem_offs), k, n, *search, t, _ptr(parent))
        # the split's tail with every point its own cell: rows = occ = the elements
        head = (_ptr(elems), k, vw, n, _ptr(index.ident, i32), n, _ptr(elems), _ptr(prefix))
        out, par, pts = instances3d.emit_kept(head, elem_offs, offs, parent, t, min_points, mode, vw) or none()
        if out.shape[1] < nw:                                                 # spare words of the input rows: zero
            out = torch.cat([out, torch.zeros((len(par), nw - vw), dtype=i64, device=dev)], dim=1)
    return out, par, pts


def cluster_instances(index: DensityIndex, result, cfg):
    """result: a FinalResult, a Stage2Result or the namespace cli._saved_instances returns (`rows` int64 [K][nw] in the
    original point order, `conf`, `final_class`).  -> the same kind with `rows` replaced by the clusters and `conf`,
    `final_class` taken from each cluster's parent, plus the attribute `parent` (int64 [R], host).  A result whose rows is
    None comes back as it is.  Config keys: cluster_min_samples, cluster_min_points, cluster_mode (cluster_eps made the
    index)."""
    rows = getattr(result, "rows", None)
    if rows is None:
        return result
    out_rows, parent, _ = cluster_rows(index, rows, index.n_points, cluster_min_samples(cfg), cluster_min_points(cfg),
                                       cluster_mode(cfg))
    return instances3d.replace_rows(result, out_rows, parent)
