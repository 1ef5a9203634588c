"""A scene's prediction assembled from all of its query classes, with a 3-D mask NMS, on the device (include/bff_hip.h:
bff_nms_pairs, bff_nms_greedy).

Every stage works on one query class at a time and leaves <cls>/<scene>.pth; the refinement hands a matched stage-1 mask
to every class whose stage-2 mask matched it, so the same object sits in several classes' files.  Here the rows of all
classes of a scene become one set of instances:

    nms_rows(rows, n_points, score, cls, thres, ...)      which rows survive a greedy NMS by score, and who removed the others
    assemble_rows(rows, n_points, score, cls, ...)        the surviving rows best first, optionally made exclusive, small ones dropped
    assemble_scene(results, n_points, cfg, device)        {class: saved file or result} -> one result with mixed `final_class`
    point_labels(assembled)                               an instance and a class per point

Rank: score descending, ties by ascending input index.  Rank r hits a later rank s iff !(v < thres) in float32, v the IoU or
the containment |i & j| / min(|i|, |j|) as one float32 division of exactly converted integers; with scope "class" only rows
of one class hit each other.  In rank order a row is kept iff no kept row hits it.  tests/assemble_ref.py restates all of it
in NumPy.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, instances3d
from ._lib import _ptr, call, i32, i64

CRITERIA = ("iou", "containment")
SCOPES = ("all", "class")
MAX_AREA = 1 << 23                 # points of a row: below it every float32 conversion of the overlap value is exact


# ------------------------------------------------------------------ config
def assemble_nms_thres(cfg):
    """The NMS threshold in (0, 1], or None: absent and 0 both mean no NMS."""
    t = cfg.get("assemble_nms_thres")
    if t is None or (instances3d._is_number(t) and t == 0):
        return None
    return instances3d.ratio("assemble_nms_thres", t)


def assemble_criterion(cfg) -> str:
    return instances3d.one_of("assemble_criterion", cfg.get("assemble_criterion"), CRITERIA, "iou")


def assemble_scope(cfg) -> str:
    return instances3d.one_of("assemble_scope", cfg.get("assemble_scope"), SCOPES, "all")


def assemble_exclusive(cfg) -> bool:
    x = cfg.get("assemble_exclusive")
    x = False if x is None else x
    if not isinstance(x, bool):
        raise ValueError(f"assemble_exclusive must be true or false, got {x!r}")
    return x


def assemble_min_points(cfg) -> int:
    return instances3d.positive_int("assemble_min_points", cfg.get("assemble_min_points"), 1)


def check_config(cfg):
    """Every assemble_* value of the config, so that a bad one stops a run before its first scene."""
    return dict(thres=assemble_nms_thres(cfg), criterion=assemble_criterion(cfg), scope=assemble_scope(cfg),
                exclusive=assemble_exclusive(cfg), min_points=assemble_min_points(cfg))


# ------------------------------------------------------------------ rows
def max_rows() -> int:
    return int(_lib.load().bff_resolve_overlaps_max_rows())


def _ones_row(n, dev):
    """int64 [ceil(n / 64)] on the device: the first n bits set."""
    vw = (n + 63) // 64
    keep = np.full(vw, -1, dtype=np.int64)
    if n % 64:
        keep[-1] = (1 << (n % 64)) - 1
    return torch.from_numpy(keep).to(dev)


def _ranked(what, rows, n_points, score, cls, thres, criterion, scope):
    """What nms_rows and assemble_rows share.  -> (clean: the rows' first ceil(N / 64) words with the bits >= N cleared, a
    copy on the device; area int64 [K] host; kept int64 [R] host: input indices, best first; removed_by int64 [K] host).
    Read-backs: the rows' areas, then -- with an NMS -- the keep bits and `by` in one."""
    if not torch.is_tensor(rows) or not rows.is_cuda:
        raise ValueError(f"{what} takes device bit rows (no CPU path)")
    if rows.dtype != i64 or rows.dim() != 2:
        raise TypeError(f"{what}: int64 [K][nw] bit rows expected")
    n, k, dev = int(n_points), int(rows.shape[0]), rows.device
    vw = (n + 63) // 64
    if n < 0 or int(rows.shape[1]) < vw:
        raise ValueError(f"{what}: rows of {int(rows.shape[1])} words for {n} points")
    score = np.asarray(score.detach().cpu() if torch.is_tensor(score) else score, dtype=np.float64).reshape(-1)
    cls = np.asarray(cls.detach().cpu() if torch.is_tensor(cls) else cls).reshape(-1)
    if len(score) != k or len(cls) != k:
        raise ValueError(f"{what}: {k} rows, {len(score)} scores and {len(cls)} classes")
    if np.isnan(score).any():
        raise ValueError(f"{what}: a NaN score")
    thres = None if thres is None or thres == 0 else instances3d.ratio(f"{what}: thres", thres)
    instances3d.one_of(f"{what}: criterion", criterion, CRITERIA)
    instances3d.one_of(f"{what}: scope", scope, SCOPES)
    removed_by = np.full(k, -1, dtype=np.int64)
    with torch.cuda.device(dev):
        clean = rows[:, :vw].clone()
        if k == 0 or vw == 0:
            removed_by[:] = -2
            return clean, np.zeros(k, dtype=np.int64), np.zeros(0, dtype=np.int64), removed_by
        _lib.and_rows(clean, _ones_row(n, dev))
        area_dev = _lib.popcount_rows(clean)
        area = area_dev.cpu().numpy().astype(np.int64)                          # read-back 1: the rows' areas
        full = np.flatnonzero(area > 0)
        removed_by[area == 0] = -2
        kn, limit = len(full), max_rows()
        if kn > limit:
            raise ValueError(f"{what}: {kn} non-empty rows, more than the {limit} a scene may hold (BFF_E_LIMIT)")
        if kn and int(area.max()) >= MAX_AREA:
            raise ValueError(f"{what}: a row of {int(area.max())} points, the limit is {MAX_AREA - 1} (BFF_E_LIMIT)")
        order = np.lexsort((np.arange(kn), -score[full]))                       # ranks over the non-empty rows
        if thres is None or kn == 0:
            return clean, area, full[order].astype(np.int64), removed_by
        idx = torch.from_numpy(full.astype(np.int32)).to(dev)
        inter = _lib.cross_popcount(clean, clean, idx, idx)                     # [kn][kn] in the order of `full`
        w = (kn + 63) // 64
        sup = torch.empty((kn, w), dtype=i64, device=dev)
        cls_dev = torch.from_numpy(cls[full].astype(np.int32)).to(dev) if scope == "class" else None
        area_full = area_dev[idx.long()].contiguous()                            # held until the launch: no temporaries
        order_dev = torch.from_numpy(order.astype(np.int32)).to(dev)
        call("bff_nms_pairs", _ptr(inter, i32), _ptr(area_full, i32), _ptr(order_dev, i32), _ptr(cls_dev, i32), kn,
             CRITERIA.index(criterion), float(thres), _ptr(sup))
        back = torch.zeros(2 * w + kn + 1, dtype=i32, device=dev)               # keep bits (8-byte aligned) | by | n_kept
        by_dev, n_kept_dev = back[2 * w:2 * w + kn], back[2 * w + kn:]
        call("bff_nms_greedy", _ptr(sup), kn, _ptr(back), _ptr(by_dev), _ptr(n_kept_dev))
        got = back.cpu().numpy()                                                # read-back 2: keep bits and by
    keep = np.unpackbits(got[:2 * w].view(np.uint8), bitorder="little")[:kn].astype(bool)
    by = got[2 * w:2 * w + kn].astype(np.int64)
    if int(keep.sum()) != int(got[-1]) or ((by < 0) != keep).any():
        raise RuntimeError(f"{what}: the keep bits and `by` of bff_nms_greedy disagree")
    ranked = full[order].astype(np.int64)
    removed_by[ranked[~keep]] = ranked[by[~keep]]
    return clean, area, ranked[keep], removed_by


def nms_rows(rows, n_points, score, cls, thres, criterion="iou", scope="all"):
    """rows: int64 [K][nw] bit rows on the device, nw >= ceil(N / 64), the bits at positions >= n_points ignored; score
    float [K] and cls int [K], host.  thres in (0, 1]; None or 0: no NMS.  -> (kept int64 [R]: the input indices of the
    surviving rows, best first; removed_by int64 [K]: the input index of the keeper, -1 for a surviving row, -2 for an empty
    row, dropped before anything else), both on the host.  A NaN score, more than max_rows() non-empty rows or a row of
    2^23 points or more raise ValueError."""
    _, _, kept, removed_by = _ranked("nms_rows", rows, n_points, score, cls, thres, criterion, scope)
    return torch.from_numpy(kept), torch.from_numpy(removed_by)


def assemble_rows(rows, n_points, score, cls, thres=None, criterion="iou", scope="all", exclusive=False, min_points=1):
    """nms_rows, then the surviving rows themselves.  -> (rows_out int64 [R][ceil(N / 64)] on the device, best first;
    source int64 [R]: their input indices; points int64 [R]; removed_by int64 [K]; the three lists on the host).
    exclusive: every row loses the points of the surviving rows of better rank (bff_resolve_overlaps with sizes R - position),
    one more read-back for the new point counts.  min_points: a row with fewer points -- after the exclusive step -- is
    dropped; its points are not handed back, and removed_by keeps its -1."""
    min_points = instances3d.positive_int("assemble_rows: min_points", min_points)
    if not isinstance(exclusive, bool):
        raise ValueError(f"assemble_rows: exclusive must be a bool, got {exclusive!r}")
    clean, area, kept, removed_by = _ranked("assemble_rows", rows, n_points, score, cls, thres, criterion, scope)
    dev, r = clean.device, len(kept)
    points = area[kept]
    with torch.cuda.device(dev):
        if r == 0:
            out = torch.zeros((0, clean.shape[1]), dtype=i64, device=dev)
        else:
            out = _lib.gather_rows(clean, torch.from_numpy(kept.astype(np.int32)).to(dev))
        if exclusive and r >= 2:
            sizes = torch.arange(r, 0, -1, dtype=i32, device=dev)               # distinct: priority is the position
            _, after = _lib.resolve_overlaps_filtered(out, sizes, None)
            points = after.cpu().numpy().astype(np.int64)
        big = points >= min_points
        if not big.all():
            out = out[torch.from_numpy(np.flatnonzero(big)).to(dev)].contiguous()
            kept, points = kept[big], points[big]
    return out, torch.from_numpy(kept), torch.from_numpy(points), torch.from_numpy(removed_by)


# ------------------------------------------------------------------ scenes
def _scores(conf, k, cls_name):
    if torch.is_tensor(conf):
        conf = conf.detach().cpu().to(torch.float64).reshape(-1).numpy()
    elif isinstance(conf, (list, tuple)):
        conf = np.asarray([float(c) for c in conf], dtype=np.float64)
    else:
        conf = np.asarray(conf, dtype=np.float64).reshape(-1)
    if len(conf) != k:
        raise ValueError(f"class {cls_name!r}: {k} instances and {len(conf)} confidences")
    return conf


def assemble_scene(results, n_points, cfg, device="cuda"):
    """results: an ordered {class name: a saved stage file (dict), a FinalResult, a Stage2Result or the namespace
    cli._saved_instances returns}; the rows are gathered by that function's conventions (dense, RLE; the reference's empty
    list forms contribute nothing).  Score = float(conf), class index = the position in `results`.  Config keys:
    assemble_nms_thres, assemble_criterion, assemble_scope, assemble_exclusive, assemble_min_points.
    -> a namespace: rows int64 [R][ceil(N / 64)] (device, best first), conf float64 [R] (the rows' scores), final_class (the
    rows' class names), classes (the names of `results`), source_class and source_row int64 [R] (where every row came
    from), removed_by int64 [K][2] ((class, row) of the keeper of every gathered row in gathering order, (-1, -1) for a
    surviving and (-2, -2) for an empty row), n_points."""
    from .cli import _saved_instances
    opts = check_config(cfg)
    n = int(n_points)
    vw = (n + 63) // 64
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("assemble_scene needs a GPU device (no CPU path)")
    classes = [str(c) for c in results]
    pieces, score, cls, row = [], [], [], []
    for ci, item in enumerate(results.values()):
        inst = _saved_instances(item, n, dev) if isinstance(item, dict) else item
        rows = getattr(inst, "rows", None)
        if rows is None or rows.shape[0] == 0:
            continue
        if getattr(inst, "n_points", n) != n:
            raise ValueError(f"class {classes[ci]!r}: a result over {inst.n_points} points, the scene has {n}")
        if rows.shape[1] < vw:
            raise ValueError(f"class {classes[ci]!r}: rows of {rows.shape[1]} words for {n} points")
        k = int(rows.shape[0])
        pieces.append(rows[:, :vw].to(dev))
        score.append(_scores(inst.conf, k, classes[ci]))
        cls.append(np.full(k, ci, dtype=np.int32))
        row.append(np.arange(k, dtype=np.int64))
    if pieces:
        all_rows = torch.cat(pieces).contiguous()
        score, cls, row = np.concatenate(score), np.concatenate(cls), np.concatenate(row)
    else:
        all_rows = torch.zeros((0, vw), dtype=i64, device=dev)
        score, cls, row = np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
    out, source, _, removed = assemble_rows(all_rows, n, score, cls, **opts)
    source, removed = source.numpy(), removed.numpy()
    by = np.stack([removed, removed], axis=1)
    gone = removed >= 0
    by[gone, 0], by[gone, 1] = cls[removed[gone]], row[removed[gone]]
    src_cls = cls[source].astype(np.int64)
    return SimpleNamespace(rows=out, conf=torch.from_numpy(score[source].astype(np.float64)),
                           final_class=[classes[c] for c in src_cls.tolist()], classes=classes,
                           source_class=torch.from_numpy(src_cls), source_row=torch.from_numpy(row[source]),
                           removed_by=torch.from_numpy(by), n_points=n)


def point_labels(assembled):
    """-> (instance uint16 [N] on the device: 0 = none, else 1 + the first -- best -- output row that holds the point
    (bff_point_labels); semantic int32 [N] on the device: that row's class position, -1 = none)."""
    rows, n = assembled.rows, int(assembled.n_points)
    with torch.cuda.device(rows.device):
        instance = _lib.point_labels(rows, n)
        table = torch.cat([torch.full((1,), -1, dtype=i32), assembled.source_class.to(i32)]).to(rows.device)
        semantic = table[instance.to(i64) & 0xFFFF]
    return instance.view(torch.uint16), semantic
