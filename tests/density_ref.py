"""The statement of include/bff_hip.h's bff_dbscan_* in NumPy, by brute force: every pair of a row's points, no grid
(DESIGN.md section 7j).  Written from the statement; the reference project has nothing like it."""
import numpy as np

from spatial_ref import pack, unpack  # noqa: F401  (re-exported: the tests pack and unpack with them)

CHUNK = 512                        # rows of the pair matrix held at once


def d2_ref(a, b):
    """float64 [A][B]: (dx * dx + dy * dy) + dz * dz with dx = a.x - b.x, every operation rounded to float64."""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def labels_ref(points, eps, min_samples, dense_row):
    """One row.  -> (label int64 [N]: the anchor (smallest core point index) of the point's cluster, -1 for noise, for
    points outside the row and for non-finite points; core bool [N])."""
    xyz = np.asarray(points, dtype=np.float64)[:, :3]
    n = xyz.shape[0]
    label, core_all = np.full(n, -1, np.int64), np.zeros(n, bool)
    idx = np.flatnonzero(np.asarray(dense_row, bool)[:n] & np.isfinite(xyz).all(1))      # ascending point index
    m = len(idx)
    if m == 0:
        return label, core_all
    x = xyz[idx]
    eps2 = np.float64(eps) * np.float64(eps)
    near = np.zeros((m, m), bool)
    for i in range(0, m, CHUNK):
        near[i:i + CHUNK] = d2_ref(x[i:i + CHUNK], x) <= eps2
    core = near.sum(1) >= min_samples                                         # the point itself counts
    lab = np.full(m, -1, np.int64)
    for seed in np.flatnonzero(core):                                         # ascending: the seed is the anchor
        if lab[seed] >= 0:
            continue
        lab[seed] = idx[seed]
        frontier = np.array([seed])
        while len(frontier):
            reach = near[frontier].any(0) & core & (lab < 0)
            lab[reach] = idx[seed]
            frontier = np.flatnonzero(reach)
    border = np.flatnonzero(~core & (near & core[None, :]).any(1))
    for i in range(0, len(border), CHUNK):
        b = border[i:i + CHUNK]
        d = d2_ref(x[b], x)
        d[~(near[b] & core[None, :])] = np.inf
        lab[b] = lab[np.argmin(d, axis=1)]                                    # the first minimum: the smallest point index
    label[idx] = lab
    core_all[idx] = core
    return label, core_all


def clusters_ref(points, eps, min_samples, dense_row):
    """The clusters of one row: a list of (points, anchor, member mask bool [N]), unordered."""
    label, _ = labels_ref(points, eps, min_samples, dense_row)
    return [(int((label == a).sum()), int(a), label == a) for a in np.unique(label[label >= 0])]


def cluster_ref(points, eps, min_samples, rows, n, min_points=1, mode="split"):
    """-> (rows_out int64 [R][nw], parent int64 [R], points int64 [R]) of the statement."""
    rows = np.asarray(rows)
    nw = rows.shape[1] if rows.ndim == 2 else (n + 63) // 64
    dense = unpack(rows, n)
    out, parent, count = [], [], []
    for k in range(dense.shape[0]):
        comps = [c for c in clusters_ref(points, eps, min_samples, dense[k]) if c[0] >= min_points]
        comps.sort(key=lambda c: (-c[0], c[1]))
        for size, _, mask in (comps[:1] if mode == "largest" else comps):
            out.append(mask), parent.append(k), count.append(size)
    packed = pack(np.stack(out), nw) if out else np.zeros((0, nw), np.int64)
    return packed, np.asarray(parent, np.int64), np.asarray(count, np.int64)


def blobs(n, n_blobs=6, noise=0.25, seed=0, sigma=0.06):
    """n points: Gaussian blobs in the unit cube plus uniform noise, shuffled."""
    rng = np.random.default_rng(seed)
    n_noise = int(n * noise)
    centres = rng.random((n_blobs, 3))
    pts = centres[rng.integers(0, n_blobs, n - n_noise)] + sigma * rng.standard_normal((n - n_noise, 3))
    pts = np.concatenate([pts, rng.random((n_noise, 3)) * 1.4 - 0.2])
    return pts[rng.permutation(n)]
