"""The statement of include/bff_hip.h's bff_spp_* in NumPy, with dictionaries and plain loops.
Written from the statement; the reference project only loads superpoint files."""
import numpy as np

from spatial_ref import pack, unpack  # noqa: F401  (bit rows <-> bool, shared with the split's statement)


def index_ref(spp):
    """-> dict(ids int64 [S], seg int32 [N], size int64 [S], offs int64 [S + 1], order int64 [N'], free bool [N])."""
    spp = np.asarray(spp).reshape(-1)
    assert np.issubdtype(spp.dtype, np.integer)
    spp = spp.astype(np.int64)
    ids = np.array(sorted({int(v) for v in spp.tolist() if v >= 0}), dtype=np.int64)
    rank = {int(v): r for r, v in enumerate(ids.tolist())}
    seg = np.array([rank.get(int(v), -1) for v in spp.tolist()], dtype=np.int32)
    members = [[] for _ in ids]
    for p, s in enumerate(seg.tolist()):                                  # ascending point index within a superpoint
        if s >= 0:
            members[s].append(p)
    size = np.array([len(m) for m in members], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    order = np.array([p for m in members for p in m], dtype=np.int64)
    return dict(ids=ids, seg=seg, size=size, offs=offs, order=order, free=seg < 0)


def need_ref(size, ratio):
    """max(1, ceil(float64(ratio) * size)): product and ceiling in float64."""
    return np.maximum(1, np.ceil(np.float64(ratio) * np.asarray(size, dtype=np.int64).astype(np.float64))).astype(np.int64)


def count_ref(seg, n_segments, dense):
    """int64 [K][S]: the points of row k in superpoint s."""
    count = np.zeros((dense.shape[0], n_segments), np.int64)
    of_point = np.asarray(seg).tolist()
    for k in range(dense.shape[0]):
        for p in np.flatnonzero(dense[k]).tolist():
            if of_point[p] >= 0:
                count[k, of_point[p]] += 1
    return count


def owner_ref(count, need):
    """int64 [S]: the row with the largest count among those that reach need[s], the smallest index on a tie; -1 = none."""
    owner = np.full(count.shape[1], -1, np.int64)
    for s in range(count.shape[1]):
        best = 0
        for k in range(count.shape[0]):
            if count[k, s] >= need[s] and count[k, s] > best:
                best, owner[s] = count[k, s], k
    return owner


def snap_ref(spp, rows, n, ratio=0.5, mode="snap", min_points=1):
    """-> (rows_out int64 [R][nw], parent int64 [R], points int64 [R]) of the statement."""
    assert mode in ("snap", "exclusive") and 0.0 < ratio <= 1.0 and min_points >= 1
    ix = index_ref(spp)
    assert len(ix["seg"]) == n
    rows = np.asarray(rows)
    nw = rows.shape[1]
    dense = unpack(rows, n)
    seg, s = ix["seg"], len(ix["ids"])
    count, need = count_ref(seg, s, dense), need_ref(ix["size"], ratio)
    owner = owner_ref(count, need)
    out = dense & ix["free"][None, :]
    members = [ix["order"][ix["offs"][j]:ix["offs"][j + 1]] for j in range(s)]
    if mode == "exclusive":
        chosen = owner[None, :] == np.arange(dense.shape[0])[:, None]
    else:
        chosen = count >= need[None, :]
    for k, j in zip(*np.nonzero(chosen)):
        out[k, members[j]] = True
    points = out.sum(1).astype(np.int64)
    parent = np.flatnonzero(points >= min_points).astype(np.int64)
    packed = pack(out[parent], nw) if len(parent) else np.zeros((0, nw), np.int64)
    return packed, parent, points[parent]
