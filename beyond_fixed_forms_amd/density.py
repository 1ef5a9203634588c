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

from . import _lib, lift, spatial
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
    eps = float(eps)
    if not (eps > 0.0 and np.isfinite(eps)):
        raise ValueError(f"density_index: eps must be a finite number of metres > 0, got {eps!r}")
    pts = lift._device_points("density_index", points, device)
    nearest = lift.nearest_index(pts, eps * CELL_SLACK)
    n = int(pts.shape[0])
    with torch.cuda.device(pts.device):
        has = nearest.grid.vox >= 0
        finite = _lib.pack_rows(has.reshape(1, n)).reshape(-1) if n else torch.zeros(0, dtype=i64, device=pts.device)
        ident = torch.where(has, torch.arange(n, dtype=i32, device=pts.device), torch.full_like(nearest.grid.vox, -1))
    return DensityIndex(eps, n, nearest, pts, finite, ident)


def _number(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not (float(x) > 0.0 and np.isfinite(float(x))):
        raise ValueError(f"{name} must be a finite number of metres > 0, got {x!r}")
    return float(x)


def _count(name, m, default=None):
    m = default if m is None else m
    if m is None:
        raise ValueError(f"{name} is not set in the config (an integer >= 1)")
    if isinstance(m, bool) or not isinstance(m, (int, float)) or m != m or int(m) != m or int(m) < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {m!r}")
    return int(m)


def cluster_eps(cfg) -> float:
    e = cfg.get("cluster_eps")
    if e is None:
        raise ValueError("cluster_eps is not set in the config (metres, > 0)")
    return _number("cluster_eps", e)


def cluster_min_samples(cfg) -> int:
    return _count("cluster_min_samples", cfg.get("cluster_min_samples"))


def cluster_min_points(cfg) -> int:
    return _count("cluster_min_points", cfg.get("cluster_min_points", 1), 1)


def cluster_mode(cfg) -> str:
    m = cfg.get("cluster_mode", "split")
    m = "split" if m is None else m
    if m not in MODES:
        raise ValueError(f"cluster_mode must be one of {MODES}, got {m!r}")
    return m


def cluster_rows(index: DensityIndex, rows, n_points, min_samples, min_points=1, mode="split"):
    """rows: int64 [K][nw] bit rows in the index's point order, on the device; bits at positions >= n_points are ignored.
    -> (rows_out int64 [R][nw] on the device, parent int64 [R], points int64 [R]; the two lists are decided on the host and
    stay there).  mode "split": every cluster with >= min_points points, by (parent, points descending, anchor);
    "largest": per parent only the first of those.  Two read-backs, as spatial.split_rows: the element counts of the
    rows, then the kept clusters."""
    if not torch.is_tensor(rows) or not rows.is_cuda:
        raise ValueError("cluster_rows takes device bit rows (no CPU path)")
    if rows.dtype != i64 or rows.dim() != 2:
        raise TypeError("cluster_rows: int64 [K][nw] bit rows expected")
    if mode not in MODES:
        raise ValueError(f"cluster_rows: mode must be one of {MODES}, got {mode!r}")
    for name, m in (("min_samples", min_samples), ("min_points", min_points)):
        if isinstance(m, bool) or int(m) != m or int(m) < 1:
            raise ValueError(f"cluster_rows: {name} must be an integer >= 1, got {m!r}")
    n, min_samples, min_points = int(n_points), int(min_samples), int(min_points)
    if n != index.n_points:
        raise ValueError(f"cluster_rows: rows over {n} points, the index holds {index.n_points}")
    rows = rows.contiguous()
    k, nw, dev = int(rows.shape[0]), int(rows.shape[1]), rows.device
    vw = (n + 63) // 64
    if nw < vw:
        raise ValueError(f"cluster_rows: rows of {nw} words for {n} points")
    if index.points.device != dev:
        raise ValueError("cluster_rows: the rows and the index live on different devices")
    near, grid = index.nearest, index.nearest.grid
    v = grid.n_voxels
    none = lambda: (torch.zeros((0, nw), dtype=i64, device=dev), torch.zeros(0, dtype=i64), torch.zeros(0, dtype=i64))
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
        count = torch.empty(t, dtype=i32, device=dev)
        kept = torch.empty((1 + t, 2), dtype=i32, device=dev)
        call("bff_split_count", *head, _ptr(elem_offs), _ptr(parent), t, min_points, _ptr(count), _ptr(kept))
        first = min(t, spatial.KEPT_FIRST_READ)
        got = kept[:1 + first].cpu().numpy()                                  # read-back 2: the kept clusters
        n_kept = int(got[0, 0])
        if n_kept > first:
            got = np.concatenate([got, kept[1 + first:1 + n_kept].cpu().numpy()])
        elem, pts = got[1:1 + n_kept, 0].astype(np.int64), got[1:1 + n_kept, 1].astype(np.int64)
        par = np.searchsorted(offs, elem, side="right") - 1
        order = np.lexsort((elem, -pts, par))                                  # within a row, element order = anchor order
        if mode == "largest" and len(order):
            p = par[order]
            order = order[np.concatenate([[True], p[1:] != p[:-1]])]
        r = len(order)
        if r == 0:
            return none()
        table = torch.full((t,), -1, dtype=i32, device=dev)
        table[torch.from_numpy(elem[order]).to(dev)] = torch.arange(r, dtype=i32, device=dev)
        out = torch.empty((r, vw), dtype=i64, device=dev)
        call("bff_split_emit", *head, _ptr(elem_offs), _ptr(parent), t, _ptr(table), r, _ptr(out))
        if nw > vw:                                                           # spare words of the input rows: zero
            out = torch.cat([out, torch.zeros((r, nw - vw), dtype=i64, device=dev)], dim=1)
    return out, torch.from_numpy(par[order].astype(np.int64)), torch.from_numpy(pts[order])


def cluster_instances(index: DensityIndex, result, cfg):
    """result: a FinalResult, a Stage2Result or the namespace cli._saved_instances returns (`rows` int64 [K][nw] in the
    original point order, `conf`, `final_class`).  -> the same kind with `rows` replaced by the clusters and `conf`,
    `final_class` taken from each cluster's parent, plus the attribute `parent` (int64 [R], host).  A result whose rows is
    None comes back as it is.  Config keys: cluster_min_samples, cluster_min_points, cluster_mode (cluster_eps made the
    index)."""
    import copy
    rows = getattr(result, "rows", None)
    if rows is None:
        return result
    out_rows, parent, _ = cluster_rows(index, rows, index.n_points, cluster_min_samples(cfg), cluster_min_points(cfg),
                                       cluster_mode(cfg))
    classes = list(result.final_class)
    new = copy.copy(result)
    new.rows = out_rows
    new.final_class = [classes[i] for i in parent.tolist()]
    new.conf = spatial._take(result.conf, parent)
    if getattr(result, "conf_host", None) is not None:
        new.conf_host = spatial._take(result.conf_host, parent)
    if getattr(result, "prefetch", None) is not None:                       # a Stage2Result's refinement inputs: of the
        new.prefetch = None                                                 # unclustered rows
    new.parent = parent
    return new
