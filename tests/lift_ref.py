"""The statement of include/bff_hip.h's subsample, bff_nn_search and bff_lift_bits in NumPy, with a dictionary of cells
and the literal 27-cell loop, plus an unrestricted brute force "nearest within r".  Written from
the statement; the reference project has no counterpart."""
import numpy as np

from spatial_ref import pack, unpack  # noqa: F401  (bit rows <-> bool, shared with the split's statement)

AXIS = 1 << 21


def three_planes(n=3000, lattice=False, seed=5, box=2.0):
    """n points on three planes of a `box` metre cube (x = 0.5, y = 1.0, z = 0.25), random coordinates or multiples of
    2^-6 (every difference, square and sum of the distance is then exact in float64)."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, int(box * 64) + 1, (n, 3)) / 64.0 if lattice else rng.random((n, 3)) * box
    plane = rng.integers(0, 3, n)
    pts[np.arange(n), plane] = np.array([0.5, 1.0, 0.25])[plane]
    return np.ascontiguousarray(pts, dtype=np.float64)


def finite_rows(points):
    return np.isfinite(np.asarray(points, dtype=np.float64)[:, :3]).all(1)


def grid_ref(points, cell):
    """-> (lo float64 [3] (NaN without a finite point), cells: {(q0, q1, q2): [point indices, ascending]})."""
    xyz = np.asarray(points, dtype=np.float64)[:, :3]
    fin = finite_rows(xyz)
    if not fin.any():
        return np.full(3, np.nan), {}
    lo = xyz[fin].min(0)
    q = np.floor((xyz - lo) / np.float64(cell))
    cells = {}
    for p in np.flatnonzero(fin).tolist():
        c = tuple(int(v) for v in q[p])
        assert all(0 <= v < AXIS for v in c)
        cells.setdefault(c, []).append(p)
    return lo, cells


def subsample_ref(points, voxel):
    """int32 [V]: the smallest point index of every occupied cell, ascending."""
    _, cells = grid_ref(points, voxel)
    return np.array(sorted(members[0] for members in cells.values()), dtype=np.int32)


def dist2(q, s):
    """(dx * dx + dy * dy) + dz * dz with dx = q.x - s.x, every operation rounded to float64.  s: [C][3]."""
    with np.errstate(all="ignore"):                                           # a far query overflows to inf: rejected
        d = q[None, :3] - s[:, :3]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _pick(cand, d2, r2):
    """The smallest d2 <= r2 among the candidates, a tie to the smallest index -> (index, d2) or (-1, inf)."""
    cand = np.asarray(cand, dtype=np.int64)
    ok = d2 <= r2                                                             # NaN fails
    if not ok.any():
        return -1, np.inf
    least = d2[ok].min()
    return int(cand[ok & (d2 == least)].min()), least


def nearest_ref(source, radius, queries):
    """The 27-cell statement -> (nn int32 [N], d2 float64 [N])."""
    src = np.asarray(source, dtype=np.float64)[:, :3]
    qs = np.asarray(queries, dtype=np.float64)[:, :3]
    c = np.float64(radius)
    r2 = c * c
    lo, cells = grid_ref(src, c)
    nn = np.full(len(qs), -1, np.int32)
    out = np.full(len(qs), np.inf, np.float64)
    if not cells:
        return nn, out
    with np.errstate(all="ignore"):
        cell = np.floor((qs - lo) / c)
    for p in range(len(qs)):
        if not np.isfinite(qs[p]).all() or not ((cell[p] >= -1) & (cell[p] <= AXIS)).all():       # tested on the doubles
            continue
        q0, q1, q2 = (int(v) for v in cell[p])
        cand = []
        for d2 in (-1, 0, 1):
            for d1 in (-1, 0, 1):
                for d0 in (-1, 0, 1):
                    cand += cells.get((q0 + d0, q1 + d1, q2 + d2), [])
        if cand:
            nn[p], out[p] = _pick(cand, dist2(qs[p], src[cand]), r2)
    return nn, out


def brute_ref(source, radius, queries):
    """Nearest within r over every finite source point, no grid -> (nn, d2)."""
    src = np.asarray(source, dtype=np.float64)[:, :3]
    qs = np.asarray(queries, dtype=np.float64)[:, :3]
    r2 = np.float64(radius) * np.float64(radius)
    cand = np.flatnonzero(finite_rows(src)).tolist() if len(src) else []
    nn = np.full(len(qs), -1, np.int32)
    out = np.full(len(qs), np.inf, np.float64)
    for p in range(len(qs)):
        if cand and np.isfinite(qs[p]).all():
            nn[p], out[p] = _pick(cand, dist2(qs[p], src[cand]), r2)
    return nn, out


def lift_ref(nn, rows, n_source, n_target):
    """rows: int64 [K][nw_in] -> int64 [K][ceil(n_target / 64)]."""
    rows = np.asarray(rows, dtype=np.int64)
    nn = np.asarray(nn).astype(np.int64)
    assert len(nn) == n_target
    dense = unpack(rows, n_source) if n_source else np.zeros((rows.shape[0], 0), bool)
    out = np.zeros((rows.shape[0], n_target), bool)
    ok = (nn >= 0) & (nn < n_source)
    out[:, ok] = dense[:, nn[ok]]
    packed = pack(out)
    return packed.reshape(rows.shape[0], (n_target + 63) // 64)
