"""What the optional 3-D stages share (spatial.py, superpoints.py, lift.py, density.py; DESIGN.md sections 7g-7j): the
points and bit rows they take, the values they read from the config, the tail that turns a forest over a row set's
elements into the kept parts' bit rows, and the result they hand back.  Only what at least two stages use.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from ._lib import _ptr, call, f64, i32, i64

KEPT_FIRST_READ = 1 << 16          # kept components the second read-back of a split call fetches with their count


def device_points(what, points, device):
    """points: an (N, >= 3) array or a float64 device tensor of that shape -> float64 [N][>= 3] on the device, contiguous."""
    if torch.is_tensor(points):
        if not points.is_cuda:
            raise ValueError(f"{what} takes an array or a device tensor (no CPU path)")
        if points.dtype != f64 or points.dim() != 2 or points.shape[1] < 3:
            raise TypeError(f"{what}: float64 [N][>= 3] points expected")
        return points.contiguous()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"{what} needs a GPU device (no CPU path)")
    a = np.asarray(points)
    if a.ndim != 2 or a.shape[1] < 3:
        raise TypeError(f"{what}: an (N, >= 3) array expected, got {a.shape}")
    return torch.as_tensor(np.ascontiguousarray(a[:, :3], dtype=np.float64)).to(dev)


def _is_number(x):
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer))


def metres(name, x) -> float:
    """A length a caller passes: anything float() takes, finite and > 0."""
    if not (float(x) > 0.0 and np.isfinite(float(x))):
        raise ValueError(f"{name} must be a finite number of metres > 0, got {x!r}")
    return float(x)


def config_metres(cfg, key) -> float:
    """A length of the config: a number, and there is no default."""
    x = cfg.get(key)
    if x is None:
        raise ValueError(f"{key} is not set in the config (metres, > 0)")
    if not _is_number(x):
        raise ValueError(f"{key} must be a finite number of metres > 0, got {x!r}")
    return metres(key, x)


def positive_int(name, m, default=None) -> int:
    m = default if m is None else m
    if m is None:
        raise ValueError(f"{name} is not set in the config (an integer >= 1)")
    if not _is_number(m) or m != m or int(m) != m or int(m) < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {m!r}")
    return int(m)


def ratio(name, r) -> float:
    if not _is_number(r) or not (0.0 < float(r) <= 1.0):                      # NaN fails both
        raise ValueError(f"{name} must be a number in (0, 1], got {r!r}")
    return float(r)


def one_of(name, m, choices, default=None):
    m = default if m is None else m
    if isinstance(m, bool) or m not in choices:
        raise ValueError(f"{name} must be one of {choices}, got {m!r}")
    return m


def check_rows(what, rows, n_points, holds, holder, index_tensor):
    """The bit rows of split_rows, snap_rows and cluster_rows against their grid or index (`holder`, of `holds` points, with
    `index_tensor` on its device).  -> (rows contiguous, K, nw, N, device)"""
    if not torch.is_tensor(rows) or not rows.is_cuda:
        raise ValueError(f"{what} takes device bit rows (no CPU path)")
    if rows.dtype != i64 or rows.dim() != 2:
        raise TypeError(f"{what}: int64 [K][nw] bit rows expected")
    n = int(n_points)
    if n != holds:
        raise ValueError(f"{what}: rows over {n} points, the {holder} holds {holds}")
    k, nw = int(rows.shape[0]), int(rows.shape[1])
    if nw < (n + 63) // 64:
        raise ValueError(f"{what}: rows of {nw} words for {n} points")
    if index_tensor.device != rows.device:
        raise ValueError(f"{what}: the rows and the {holder} live on different devices")
    return rows.contiguous(), k, nw, n, rows.device


def no_rows(nw, dev):
    """What split_rows, snap_rows and cluster_rows return when nothing is kept."""
    return torch.zeros((0, nw), dtype=i64, device=dev), torch.zeros(0, dtype=i64), torch.zeros(0, dtype=i64)


def kept_order(offs, elem, pts, mode):
    """offs int64 [K + 1]: the rows' first elements; elem, pts int64 [n]: the kept components' root elements and point
    counts, in any order.  -> (order int64 [R]: positions into elem by (parent row, points descending, anchor) -- within a
    row, element order is anchor order -- in mode "largest" only the first of every parent; par int64 [n]: the parent row
    of every kept component)."""
    par = np.searchsorted(offs, elem, side="right") - 1
    order = np.lexsort((elem, -pts, par))
    if mode == "largest" and len(order):
        p = par[order]
        order = order[np.concatenate([[True], p[1:] != p[:-1]])]
    return order, par


def emit_kept(head, elem_offs, offs, parent, t, min_points, mode, width):
    """The tail of split_rows and cluster_rows.  head: the leading arguments of bff_split_count / bff_split_emit (rows, K,
    nw, N, vox, V, occ, prefix); elem_offs int32 [K + 1] on the device and offs, its host copy; parent int32 [t]: the
    flattened forest; width: the words of an output row.  -> (rows_out, parent row, points) or None when nothing is
    kept.  One read-back, the kept components; past KEPT_FIRST_READ of them a second fetches the rest."""
    dev = parent.device
    count = torch.empty(t, dtype=i32, device=dev)
    kept = torch.empty((1 + t, 2), dtype=i32, device=dev)
    call("bff_split_count", *head, _ptr(elem_offs), _ptr(parent), t, min_points, _ptr(count), _ptr(kept))
    first = min(t, KEPT_FIRST_READ)
    got = kept[:1 + first].cpu().numpy()
    n_kept = int(got[0, 0])
    if n_kept > first:
        got = np.concatenate([got, kept[1 + first:1 + n_kept].cpu().numpy()])
    elem, pts = got[1:1 + n_kept, 0].astype(np.int64), got[1:1 + n_kept, 1].astype(np.int64)
    order, par = kept_order(offs, elem, pts, mode)
    r = len(order)
    if r == 0:
        return None
    table = torch.full((t,), -1, dtype=i32, device=dev)
    table[torch.from_numpy(elem[order]).to(dev)] = torch.arange(r, dtype=i32, device=dev)
    out = torch.empty((r, width), dtype=i64, device=dev)
    call("bff_split_emit", *head, _ptr(elem_offs), _ptr(parent), t, _ptr(table), r, _ptr(out))
    return out, torch.from_numpy(par[order].astype(np.int64)), torch.from_numpy(pts[order])


def _take(conf, parent):
    """conf[parent] in conf's own container kind and dtype."""
    idx = parent.tolist()
    if isinstance(conf, (list, tuple)):
        return type(conf)(conf[i] for i in idx)
    if torch.is_tensor(conf):
        return conf.reshape(-1)[parent.to(conf.device)]
    return np.asarray(conf).reshape(-1)[np.asarray(idx, dtype=np.int64)]


def replace_rows(result, rows, parent=None, n_points=None):
    """result: a FinalResult, a Stage2Result or the namespace cli._saved_instances returns.  -> a copy with `rows` replaced;
    with parent (int64 [R], host), `conf`, `conf_host` and `final_class` are taken from every new row's parent and the copy
    gets the attribute `parent`; with n_points, a result that has `n_points` gets the new one (to_dict() unpacks to it).
    A Stage2Result's `prefetch`, the refinement inputs of the rows that were replaced, is dropped.  rows None: the result
    itself."""
    if rows is None:
        return result
    new = copy.copy(result)
    new.rows = rows
    if parent is not None:
        classes = list(result.final_class)
        new.final_class = [classes[i] for i in parent.tolist()]
        new.conf = _take(result.conf, parent)
        if getattr(result, "conf_host", None) is not None:
            new.conf_host = _take(result.conf_host, parent)
        new.parent = parent
    if n_points is not None and hasattr(result, "n_points"):
        new.n_points = int(n_points)
    if getattr(result, "prefetch", None) is not None:
        new.prefetch = None
    return new
