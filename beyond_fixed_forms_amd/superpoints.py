"""3-D instances snapped to superpoints, on the device (include/bff_hip.h: bff_spp_*).

A stage-2 instance is a ragged set of points: holes where the sensor depth was missing, frayed borders, stray points on
neighbouring surfaces.  The datasets ship an over-segmentation of every scan into superpoints (superpoints/<scene>.pth,
one integer id per point); here a superpoint that holds enough of an instance's points goes to the instance whole, and
one that does not leaves it -- integer arithmetic, a pure function of the inputs, independent of thread schedule and run:

    superpoint_index(spp)                         the index of a scene: ranks per point, the distinct ids, the points of
                                                  every superpoint, the bit row of the points without one
    superpoints_from_grid(grid)                   the same with the cells of a spatial.VoxelGrid as superpoints
    snap_rows(index, rows, n_points, ...)         bit rows -> the snapped bit rows, the parent row and the points of each
    snap_instances(index, result, cfg)            a FinalResult / Stage2Result / saved-file namespace with `rows` replaced,
                                                  `conf` and `final_class` taken from each row's parent

The statement is the header's; tests/superpoints_ref.py restates it in NumPy.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib, instances3d
from ._lib import _ptr, call, i32, i64

MODES = ("snap", "exclusive")
NO_ID = (1 << 63) - 1              # the sort key of a negative id: after every id (bff_voxel_heads' key without a cell)


@dataclasses.dataclass
class SuperpointIndex:
    n_points: int
    n_segments: int
    ids: torch.Tensor              # int64 [S] (device): the distinct ids >= 0, ascending
    seg: torch.Tensor              # int32 [N] (device): the rank of the point's id, -1 for a negative id
    order: torch.Tensor            # int32 [N'] (device): the points with a superpoint, by (superpoint, point)
    offs: torch.Tensor             # int32 [S + 1] (device): superpoint s is order[offs[s] : offs[s + 1]]
    size: torch.Tensor             # int32 [S] (device): the points of every superpoint
    free: torch.Tensor             # int64 [1][ceil(N / 64)] (device): the bit row of the points with seg = -1
    size_host: np.ndarray = None   # int64 [S]: `size` on the host, what `need` is computed from
    _need: dict = dataclasses.field(default_factory=dict, repr=False)

    def need(self, ratio) -> torch.Tensor:
        """int32 [S] (device): the points a row must hold of every superpoint at this ratio; once per (index, ratio)."""
        ratio = float(ratio)
        if ratio not in self._need:
            self._need[ratio] = torch.from_numpy(need_points(self.size_host, ratio)).to(self.seg.device)
        return self._need[ratio]


def need_points(size, ratio) -> np.ndarray:
    """need[s] = max(1, ceil(float64(ratio) * size[s])) as int32: the definition, product and ceiling in float64."""
    size = np.asarray(size, dtype=np.int64)
    return np.maximum(1, np.ceil(np.float64(ratio) * size.astype(np.float64))).astype(np.int32)


def superpoint_index(spp, device="cuda") -> SuperpointIndex:
    """spp: one integer id per point in the caller's point order -- a NumPy array, a tensor or a device tensor of any
    integer dtype (what torch.load gives for superpoints/<scene>.pth).  Two read-backs (the number of superpoints, their
    sizes); the index serves every class, ratio and mode of the scene."""
    if torch.is_tensor(spp):
        if spp.dtype.is_floating_point or spp.dtype.is_complex or spp.dtype == torch.bool:
            raise TypeError(f"superpoint_index: integer ids expected, got {spp.dtype}")
        ids = spp.reshape(-1)
        if not ids.is_cuda:
            if torch.device(device).type != "cuda":
                raise ValueError("superpoint_index needs a GPU device (no CPU path)")
            ids = ids.to(device)
        ids = ids.to(i64)
    else:
        if torch.device(device).type != "cuda":
            raise ValueError("superpoint_index needs a GPU device (no CPU path)")
        a = np.asarray(spp)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"superpoint_index: integer ids expected, got {a.dtype}")
        ids = torch.from_numpy(np.ascontiguousarray(a.reshape(-1).astype(np.int64, copy=False))).to(device)
    dev, n = ids.device, int(ids.shape[0])
    if n >= 1 << 31:
        raise ValueError(f"superpoint_index: {n} points, at most 2^31 - 1")
    with torch.cuda.device(dev):
        seg = torch.full((n,), -1, dtype=i32, device=dev)
        free = torch.zeros((1, (n + 63) // 64), dtype=i64, device=dev)
        empty = lambda: SuperpointIndex(n, 0, torch.zeros(0, dtype=i64, device=dev), seg, torch.zeros(0, dtype=i32, device=dev),
                                        torch.zeros(1, dtype=i32, device=dev), torch.zeros(0, dtype=i32, device=dev), free,
                                        np.zeros(0, np.int64))
        if n == 0:
            return empty()
        key = torch.where(ids < 0, torch.full_like(ids, NO_ID), ids).contiguous()
        order = _lib.argsort_i64(key, 63)                                     # stable: equal ids stay in point order
        sorted_keys = key[order.long()]
        head = torch.empty(n, dtype=i32, device=dev)
        call("bff_voxel_heads", _ptr(sorted_keys), n, _ptr(head))
        incl = torch.cumsum(head, 0, dtype=i64)
        s = int(incl[-1].item())                                              # read-back: the number of superpoints
        distinct = torch.empty(s, dtype=i64, device=dev)
        call("bff_voxel_ranks", _ptr(sorted_keys), _ptr(order, i32), _ptr(incl), n, s, _ptr(seg), _ptr(distinct) if s else None)
        free = _lib.pack_rows((seg < 0).view(1, n))
        if s == 0:
            return empty()
        # offs[r] = the position of superpoint r's head in the sorted list; slot s + 1 swallows the other positions
        offs = torch.empty(s + 2, dtype=i64, device=dev)
        offs.scatter_(0, torch.where(head == 1, incl - 1, torch.full_like(incl, s + 1)), torch.arange(n, dtype=i64, device=dev))
        offs[s] = (sorted_keys != NO_ID).sum()
        offs = offs[:s + 1].to(i32)
        size = offs[1:] - offs[:-1]
        size_host = size.cpu().numpy().astype(np.int64)                       # read-back: the sizes (for `need`)
        order = order[:int(size_host.sum())].contiguous()
    return SuperpointIndex(n, s, distinct, seg, order, offs, size, free, size_host)


def superpoints_from_grid(grid) -> SuperpointIndex:
    """The index whose superpoints are the cells of a spatial.VoxelGrid, for scenes that have no superpoint file; a point
    without a cell (vox = -1) is free."""
    if not torch.is_tensor(grid.vox) or not grid.vox.is_cuda:
        raise ValueError("superpoints_from_grid takes a device grid (no CPU path)")
    return superpoint_index(grid.vox)


def snap_ratio(cfg) -> float:
    r = cfg.get("snap_ratio")
    return instances3d.ratio("snap_ratio", 0.5 if r is None else r)


def snap_mode(cfg) -> str:
    return instances3d.one_of("snap_mode", cfg.get("snap_mode"), MODES, "snap")


def snap_min_points(cfg) -> int:
    return instances3d.positive_int("snap_min_points", cfg.get("snap_min_points"), 1)


def snap_rows(index: SuperpointIndex, rows, n_points, ratio=0.5, mode="snap", min_points=1):
    """rows: int64 [K][nw] bit rows in the index's point order, on the device; bits at positions >= n_points are ignored
    and zero in the result.  -> (rows_out int64 [R][nw] on the device, parent int64 [R], points int64 [R]; the two lists
    are decided on the host and stay there): the rows that keep at least min_points points, in their order.  One
    read-back: the point counts."""
    rows, k, nw, n, dev = instances3d.check_rows("snap_rows", rows, n_points, index.n_points, "index", index.seg)
    instances3d.one_of("snap_rows: mode", mode, MODES)
    ratio = instances3d.ratio("snap_rows: ratio", ratio)
    min_points, s = instances3d.positive_int("snap_rows: min_points", min_points), index.n_segments
    none = lambda: instances3d.no_rows(nw, dev)
    if k == 0 or n == 0:
        return none()
    with torch.cuda.device(dev):
        free = index.free.reshape(-1)
        if nw > free.shape[0]:                                                # words past the cloud: nothing is free there
            free = torch.cat([free, torch.zeros(nw - free.shape[0], dtype=i64, device=dev)])
        out = rows.clone()
        _lib.and_rows(out, free)                                              # rows & free; free's bits >= N are zero
        if s:
            need = index.need(ratio)
            count = torch.empty((k, s), dtype=i32, device=dev)
            call("bff_spp_count", _ptr(rows), k, nw, n, _ptr(index.seg, i32), s, _ptr(count))
            owner = None
            if mode == "exclusive":
                owner = torch.empty(s, dtype=i32, device=dev)
                call("bff_spp_owner", _ptr(count), k, s, _ptr(need, i32), _ptr(owner))
            call("bff_spp_fill", _ptr(count), k, s, _ptr(need, i32), _ptr(owner), _ptr(index.order, i32), _ptr(index.offs, i32),
                 _ptr(out), nw)
        points = _lib.popcount_rows(out).cpu().to(i64)                        # the read-back: the rows' points
        parent = torch.nonzero(points >= min_points).reshape(-1)
        if len(parent) == 0:
            return none()
        if len(parent) < k:
            out = _lib.gather_rows(out, parent.to(i32).to(dev))
    return out, parent, points[parent]


def snap_instances(index: SuperpointIndex, result, cfg):
    """result: a FinalResult, a Stage2Result or the namespace cli._saved_instances returns (`rows` int64 [K][nw] in the
    original point order, `conf`, `final_class`).  -> the same kind with `rows` replaced by the snapped rows that survive
    and `conf`, `final_class` taken from each one's parent, plus the attribute `parent` (int64 [R], host).  A result whose
    rows is None comes back as it is.  Config keys: snap_ratio, snap_mode, snap_min_points."""
    rows = getattr(result, "rows", None)
    if rows is None:
        return result
    out_rows, parent, _ = snap_rows(index, rows, index.n_points, snap_ratio(cfg), snap_mode(cfg), snap_min_points(cfg))
    return instances3d.replace_rows(result, out_rows, parent)
