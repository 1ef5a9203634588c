"""The statement of include/bff_hip.h's bff_voxel_* / bff_split_* in NumPy, with dictionaries and a plain union-find
(DESIGN.md section 7g).  Written from the statement; the reference project has nothing like it."""
import numpy as np

AXIS = 1 << 21
# the 13 forward offsets (d2, d1, d0) > (0, 0, 0), lexicographically ascending
FORWARD = [(d2, d1, d0) for d2 in (-1, 0, 1) for d1 in (-1, 0, 1) for d0 in (-1, 0, 1) if (d2, d1, d0) > (0, 0, 0)]


def grid_ref(points, cell):
    """-> (lo float64 [3], vox int32 [N], keys int64 [V], nbr int32 [V][13])."""
    xyz = np.asarray(points, dtype=np.float64)[:, :3]
    n = xyz.shape[0]
    finite = np.isfinite(xyz).all(1)
    vox = np.full(n, -1, np.int32)
    if not finite.any():
        return np.full(3, np.nan), vox, np.zeros(0, np.int64), np.zeros((0, 13), np.int32)
    lo = xyz[finite].min(0)
    q = np.floor((xyz[finite] - lo) / np.float64(cell)).astype(np.int64)
    if (q >= AXIS).any():
        raise ValueError("more than 2^21 cells on an axis")
    key = q[:, 0] + (q[:, 1] << 21) + (q[:, 2] << 42)
    keys, inverse = np.unique(key, return_inverse=True)
    vox[finite] = inverse.reshape(-1).astype(np.int32)
    rank = {int(k): i for i, k in enumerate(keys)}
    nbr = np.full((len(keys), 13), -1, np.int32)
    for i, k in enumerate(keys.tolist()):
        q0, q1, q2 = k & (AXIS - 1), (k >> 21) & (AXIS - 1), k >> 42
        for j, (d2, d1, d0) in enumerate(FORWARD):
            a, b, c = q0 + d0, q1 + d1, q2 + d2
            if 0 <= a < AXIS and 0 <= b < AXIS and 0 <= c < AXIS:          # the axis itself: the key must not wrap
                nbr[i, j] = rank.get(a + (b << 21) + (c << 42), -1)
    return lo, vox, keys.astype(np.int64), nbr


def unpack(rows, n):
    """int64 / uint64 [K][nw] bit rows -> bool [K][n] (bits at positions >= n are ignored)."""
    rows = np.ascontiguousarray(rows).view(np.uint64)
    k = rows.shape[0]
    if k == 0 or n == 0:
        return np.zeros((k, n), bool)
    bits = (rows[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(k, -1)[:, :n].astype(bool)


def pack(dense, nw=None):
    """bool [K][n] -> int64 [K][nw] bit rows with zero padding bits."""
    dense = np.asarray(dense, bool)
    k, n = dense.shape
    nw = (n + 63) // 64 if nw is None else nw
    padded = np.zeros((k, nw * 64), np.uint64)
    padded[:, :n] = dense
    words = (padded.reshape(k, nw, 64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(2, dtype=np.uint64)
    return words.view(np.int64)


def components_ref(vox, keys, dense_row):
    """The components of one row: a list of (points, anchor, member mask bool [N]), unordered."""
    pts = np.flatnonzero(dense_row & (vox >= 0))
    cells = sorted(set(vox[pts].tolist()))
    coord = {c: (int(keys[c]) & (AXIS - 1), (int(keys[c]) >> 21) & (AXIS - 1), int(keys[c]) >> 42) for c in cells}
    where = {q: c for c, q in coord.items()}
    parent = {c: c for c in cells}

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    for c, (a, b, d) in coord.items():
        for da in (-1, 0, 1):
            for db in (-1, 0, 1):
                for dd in (-1, 0, 1):
                    o = where.get((a + da, b + db, d + dd))
                    if o is not None and o != c:
                        ra, rb = find(c), find(o)
                        if ra != rb:
                            parent[max(ra, rb)] = min(ra, rb)
    out = {}
    for p in pts.tolist():
        out.setdefault(find(int(vox[p])), []).append(p)
    anchor = {}
    for c in cells:                                                  # the smallest cell rank of every component
        r = find(c)
        anchor[r] = min(anchor.get(r, c), c)
    comps = []
    for root, members in out.items():
        mask = np.zeros(len(vox), bool)
        mask[members] = True
        comps.append((len(members), anchor[root], mask))
    return comps


def split_ref(points, cell, rows, n, min_points=1, mode="split"):
    """-> (rows_out int64 [R][nw], parent int64 [R], points int64 [R]) of the statement."""
    _, vox, keys, _ = grid_ref(points, cell)
    rows = np.asarray(rows)
    nw = rows.shape[1] if rows.ndim == 2 else (n + 63) // 64
    dense = unpack(rows, n)
    out, parent, count = [], [], []
    for k in range(dense.shape[0]):
        comps = [c for c in components_ref(vox, keys, dense[k]) if c[0] >= min_points]
        comps.sort(key=lambda c: (-c[0], c[1]))
        for size, _, mask in (comps[:1] if mode == "largest" else comps):
            out.append(mask), parent.append(k), count.append(size)
    packed = pack(np.stack(out), nw) if out else np.zeros((0, nw), np.int64)
    return packed, np.asarray(parent, np.int64), np.asarray(count, np.int64)
