"""The NumPy statement of the scene assembly (beyond_fixed_forms_amd/assemble.py; include/bff_hip.h: bff_nms_pairs,
bff_nms_greedy): rank, the hits matrix, the greedy walk, `by`, the exclusive step, the minimum
size and the point labels, on dense bool rows.  Everything the device computes is compared with this for equality."""
import numpy as np

CRITERIA = ("iou", "containment")
SCOPES = ("all", "class")


def rank(score):
    """Score descending, ties by ascending index (a stable sort).  -> order: order[r] = the index of rank r."""
    score = np.asarray(score, dtype=np.float64)
    if np.isnan(score).any():
        raise ValueError("a NaN score")
    return np.lexsort((np.arange(len(score)), -score))


def hits(inter, area, order, cls, thres, criterion="iou", scope="all"):
    """inter int [K][K], area int [K], cls int [K]: all in input order.  -> bool [K][K] by rank: h[r][s] = r < s and r hits s.
    One float32 division of exactly converted integers, and the reference's keep-test `v < thres` in float32, negated."""
    assert criterion in CRITERIA and scope in SCOPES
    inter, area, order = np.asarray(inter, dtype=np.int64), np.asarray(area, dtype=np.int64), np.asarray(order)
    both = inter[np.ix_(order, order)]
    a = area[order]
    den = a[:, None] + a[None, :] - both if criterion == "iou" else np.minimum(a[:, None], a[None, :])
    assert den.max(initial=0) < 1 << 24 and both.max(initial=0) < 1 << 24
    with np.errstate(invalid="ignore", divide="ignore"):
        v = both.astype(np.float32) / den.astype(np.float32)
    h = ~(v < np.float32(thres))
    if scope == "class":
        c = np.asarray(cls)[order]
        h &= c[:, None] == c[None, :]
    return np.triu(h, 1)


def greedy(h):
    """h bool [K][K] by rank, upper triangle.  In rank order r is kept iff no kept q < r hits it.
    -> (keep bool [K], by int32 [K]: the smallest kept q that hits r, -1 for a kept r)."""
    k = len(h)
    keep, by = np.zeros(k, dtype=bool), np.full(k, -1, dtype=np.int32)
    removed = np.zeros(k, dtype=bool)
    for r in range(k):
        if removed[r]:
            continue
        keep[r] = True
        new = h[r] & ~removed
        by[new] = r
        removed |= new
    return keep, by


def pack_bits(bits):
    """bool [R][n] -> uint64 [R][ceil(n / 64)], bit p of a row in word p >> 6 at position p & 63."""
    bits = np.asarray(bits, dtype=bool)
    r, n = bits.shape
    w = (n + 63) // 64
    padded = np.zeros((r, w * 64), dtype=np.uint8)
    padded[:, :n] = bits
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(r, w)


def unpack_bits(words, n):
    words = np.ascontiguousarray(words).view(np.uint64).reshape(len(words), -1)
    return np.unpackbits(words.astype("<u8").view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def nms(dense, score, cls, thres, criterion="iou", scope="all"):
    """dense bool [K][N] (only the N points of the scene), score float [K], cls int [K].  thres None or 0: no NMS.
    -> (kept int64 [R]: input indices, best first; removed_by int64 [K]: the input index of the keeper, -1 for a row that
    survives, -2 for an empty row, dropped before anything else)."""
    dense = np.asarray(dense, dtype=bool)
    k = len(dense)
    order_all = rank(score)
    area = dense.sum(axis=1).astype(np.int64)
    removed_by = np.full(k, -1, dtype=np.int64)
    removed_by[area == 0] = -2
    order = order_all[area[order_all] > 0]                 # the ranks of the non-empty rows, input indices
    if not thres or len(order) == 0:
        return order.astype(np.int64), removed_by
    d = dense.astype(np.int64)
    h = hits(d @ d.T, area, order, cls, thres, criterion, scope)
    keep, by = greedy(h)
    gone = by >= 0
    removed_by[order[gone]] = order[by[gone]]
    return order[keep].astype(np.int64), removed_by


def assemble(dense, score, cls, thres, criterion="iou", scope="all", exclusive=False, min_points=1):
    """-> (rows bool [R][N] best first, source int64 [R]: input indices, points int64 [R], removed_by int64 [K]).
    exclusive: a kept row loses the points of the kept rows of better rank; min_points counts after that step, and the
    points of a row it drops are not handed back."""
    dense = np.asarray(dense, dtype=bool)
    kept, removed_by = nms(dense, score, cls, thres, criterion, scope)
    rows = dense[kept].copy()
    if exclusive:
        taken = np.zeros(dense.shape[1], dtype=bool)
        for r in range(len(rows)):
            mine = rows[r].copy()
            rows[r] &= ~taken
            taken |= mine
    points = rows.sum(axis=1).astype(np.int64)
    big = points >= min_points
    return rows[big], kept[big], points[big], removed_by


def point_labels(rows, row_cls):
    """rows bool [R][N] best first, row_cls int [R].  -> (instance uint16 [N]: 1 + the first row that holds the point, 0 =
    none; semantic int32 [N]: that row's class, -1 = none)."""
    rows = np.asarray(rows, dtype=bool)
    r, n = rows.shape
    if r == 0:
        return np.zeros(n, dtype=np.uint16), np.full(n, -1, dtype=np.int32)
    any_row = rows.any(axis=0)
    first = rows.argmax(axis=0)
    instance = np.where(any_row, first + 1, 0).astype(np.uint16)
    semantic = np.where(any_row, np.asarray(row_cls, dtype=np.int32)[first], -1).astype(np.int32)
    return instance, semantic
