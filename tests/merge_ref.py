"""Plain NumPy restatement of what bff_row_stats and bff_merge_components compute (include/bff_hip.h), and the
near-threshold inputs the tile-pass tests feed them.  No GPU, no library: tests/test_merge_ref.py checks this
reference against oracle.projection_ref, tests/test_gpu_merge_paths.py checks the device against it.

Two parts.  The reference proper, the only source of expected values: gram, iou_f32, edges, components and
row_stats_ref (with histogram and chunk_counts).  Input helpers, which build and vet test inputs and are never compared
with the device: hist_bound, chunk_bound, bound_passes, chained_rows, scaled_components and check_near_threshold (it
returns the reference components and edges of the input it has vetted, computed by the functions above)."""
import numpy as np

BINS = 64            # histogram bins per row, each ceil(nw / 64) words wide
CHUNK_WORDS = 8      # words per chunk (512 points)
CHUNK = 64 * CHUNK_WORDS


def gram(d, block=1 << 15):
    """Exact intersections I[i][j] = |row i & row j| of a bool (R, N) array, int64.  Blocked float32 matmul: every
    partial sum is an integer <= block < 2**24, hence exact."""
    d = np.asarray(d, dtype=bool)
    out = np.zeros((d.shape[0], d.shape[0]), np.int64)
    for lo in range(0, d.shape[1], block):
        f = d[:, lo:lo + block].astype(np.float32)
        out += (f @ f.T).astype(np.int64)
    return out


def iou_f32(inter, area):
    """iou = f32(I) / (f32(a_i) + f32(a_j) - f32(I)), every step rounded to float32; 0/0 -> NaN."""
    fi = np.asarray(inter).astype(np.float32)
    fa = np.asarray(area).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return fi / ((fa[:, None] + fa[None, :]) - fi)


def edges(inter, labels, thr, area=None):
    """bool (R, R): labels equal and iou > f32(thr), no self edges.  area defaults to the Gram's diagonal."""
    inter = np.asarray(inter)
    area = np.diag(inter) if area is None else np.asarray(area)
    labels = np.asarray(labels)
    with np.errstate(invalid="ignore"):
        e = (labels[:, None] == labels[None, :]) & (iou_f32(inter, area) > np.float32(thr))   # NaN > thr is False
    np.fill_diagonal(e, False)
    return e


def components(e, n=None, links=()):
    """comp[i] = smallest row index of i's component in the undirected graph of the bool matrix `e` (plus the extra
    (a, b) pairs in `links`)."""
    e = np.asarray(e, dtype=bool)
    n = e.shape[0] if n is None else n
    a = e | e.T
    if len(links):
        a = a.copy()
        for p, q in links:
            a[p, q] = a[q, p] = True
    comp = np.full(n, -1, np.int64)
    for i in range(n):
        if comp[i] >= 0:
            continue
        reach = np.zeros(n, bool)
        reach[i] = True
        frontier = np.array([i])
        while frontier.size:
            nxt = a[frontier].any(axis=0) & ~reach
            reach |= nxt
            frontier = np.flatnonzero(nxt)
        comp[reach] = i                    # i is the smallest: every smaller row already has its component
    return comp


def _word_pop(d, nw):
    """popcount of every 64-point word, int64 (R, nw)."""
    d = np.asarray(d, dtype=bool)
    pad = np.zeros((d.shape[0], nw * 64), bool)
    pad[:, :d.shape[1]] = d
    return pad.reshape(d.shape[0], nw, 64).sum(axis=2, dtype=np.int64)


def histogram(d, nw):
    """int64 (R, 64): set bits of the row per range of ceil(nw / 64) words."""
    wp = _word_pop(d, nw)
    bw = -(-max(nw, 1) // BINS)
    out = np.zeros((wp.shape[0], BINS), np.int64)
    for b in range(BINS):
        out[:, b] = wp[:, b * bw:(b + 1) * bw].sum(axis=1)
    return out


def chunk_counts(d, nw=None):
    """int64 (R, ceil(nw / 8)): set bits of the row per 512-point chunk."""
    nw = -(-np.asarray(d).shape[1] // 64) if nw is None else nw
    wp = _word_pop(d, nw)
    nc = -(-nw // CHUNK_WORDS)
    pad = np.zeros((wp.shape[0], nc * CHUNK_WORDS), np.int64)
    pad[:, :nw] = wp
    return pad.reshape(wp.shape[0], nc, CHUNK_WORDS).sum(axis=2)


def _min_sum(h):
    out = np.zeros((h.shape[0], h.shape[0]), np.int64)
    for i in range(h.shape[0]):
        out[i] = np.minimum(h[i][None, :], h).sum(axis=1)
    return out


def hist_bound(d, nw):
    """First-level bound of the tile pass: sum over the 64 bins of min(hist_i, hist_j) >= I(i, j)."""
    return _min_sum(histogram(d, nw))


def chunk_bound(d, nw=None):
    """Second-level bound: sum over the 512-point chunks of min(points of i, points of j) >= I(i, j)."""
    return _min_sum(chunk_counts(d, nw))


def bound_passes(bound, area, labels, thr):
    """Pairs (bool (R, R), no diagonal) a bound lets through: the exact test evaluated on min(bound, a_i, a_j)."""
    area = np.asarray(area)
    return edges(np.minimum(bound, np.minimum(area[:, None], area[None, :])), labels, thr, area)


def row_stats_ref(d, nw):
    """-> dict(area i32 [R], mean_word i32 [R], hist u32 [R][64], chunk_mask u64 [R][mw], chunk_pop u16 [R][64 mw],
    signature i64 [R]) as bff_row_stats defines them."""
    wp = _word_pop(d, nw)
    r = wp.shape[0]
    area = wp.sum(axis=1)
    weighted = (wp * np.arange(nw, dtype=np.int64)[None, :]).sum(axis=1)
    mean_word = np.where(area > 0, weighted // np.maximum(area, 1), 0x7fffffff)
    hist = histogram(d, nw)
    cc = chunk_counts(d, nw)
    mw = max(-(-cc.shape[1] // 64), 0)
    cpop = np.zeros((r, 64 * mw), np.int64)
    cpop[:, :cc.shape[1]] = cc
    cmask = np.packbits(cpop > 0, axis=1, bitorder="little").view(np.uint64).reshape(r, mw)
    sig = np.zeros(r, np.int64)
    for i in range(r):
        heavy = [b for b in range(BINS) if area[i] > 0 and hist[i, b] * 100 >= area[i] * 15]
        key = 0
        for s in range(5):
            key = (key << 6) | (heavy[s] if s < len(heavy) else 63)
        sig[i] = key
    return {"area": area.astype(np.int32), "mean_word": mean_word.astype(np.int32), "hist": hist.astype(np.uint32),
            "chunk_mask": cmask, "chunk_pop": cpop.astype(np.uint16), "signature": sig}


# ---- near-threshold inputs ------------------------------------------------------------------------------------------

def chained_rows(rng, r, n, p=0.31, f=0.05, chain=7, cols=None):
    """Bernoulli(p) rows over `cols` (default: all n points); inside every group of `chain` consecutive rows, row i
    takes over row i-1's value at a random fraction f of the positions.  Independent rows meet at IoU ~ p / (2 - p)
    = 0.183, chained neighbours at ~0.20-0.21: a handful of points decides every edge."""
    cols = np.arange(n) if cols is None else np.asarray(cols)
    sub = rng.random((r, cols.size)) < p
    for i in range(1, r):
        if i % chain:
            take = rng.random(cols.size) < f
            sub[i, take] = sub[i - 1, take]
    d = np.zeros((r, n), bool)
    d[:, cols] = sub
    return d


def scaled_components(inter, area, labels, thr, num, den=8):
    """Components when every off-diagonal intersection is multiplied by num / den (areas unchanged): what a kernel
    that loses (7/8) or doubles (9/8) one of eight parts of the chunk list would report."""
    g = inter * num // den
    return components(edges(g, labels, thr, area))


def check_near_threshold(inter, labels, thr, rows=None):
    """The properties every generated input must have, on the reference alone (`rows`: the rows carrying the
    near-threshold structure, default all).  Returns (components, edges)."""
    inter = np.asarray(inter)
    rows = np.arange(inter.shape[0]) if rows is None else np.asarray(rows)
    sub = inter[np.ix_(rows, rows)]
    lab = np.asarray(labels)[rows]
    area = np.diag(sub)
    e = edges(sub, lab, thr)
    comp = components(e)
    n_comp = np.unique(comp).size
    assert 1 < n_comp < rows.size / 2, n_comp
    iou = iou_f32(sub, area)
    near = np.triu(e & (iou < np.float32(thr) * np.float32(1.05)), 1).sum()
    assert near >= rows.size / 4, near
    assert not np.array_equal(scaled_components(sub, area, lab, thr, 7), comp)       # 1/8 lost
    assert not np.array_equal(scaled_components(sub, area, lab, thr, 9), comp)       # 1/8 added
    full = edges(inter, labels, thr)
    return components(full), full
