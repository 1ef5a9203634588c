"""The views of 3-D instances (bff_instance_views, bff_select_views; beyond_fixed_forms_amd/views.py) stated in NumPy.
Host only; everything is integer but one float64 product per crop side.

A visibility table over F slots (vis_mask uint64 [F][stride], vis_off uint32 [F][stride], vis_pix uint32 [pairs] holding
u | v << 16: visibility_ref.table's layout) and K instance bit rows in the table's (sorted) point order, uint64 [K][nw].
S(k, f) = the points whose bit is set in row k and in vis_mask[f]:

  visible[k][f]  |S(k, f)|
  box[k][f]      (min u, min v, max u, max v) over the pixels of S(k, f), inclusive; (W, H, -1, -1) where S is empty
  area[k]        popcount(row k)
  candidates     the slots with visible >= max(1, min_points), by visible descending, ties by ascending slot position
  top[k][t]      the t-th candidate's slot position, -1 past the candidates; top_visible its count, or 0
  crops[k][t][l] for the view's box (u0, v0, u1, v1):  ex = (int)floor((double)(u1 - u0) * r) * l, ey likewise,
                 (max(0, u0 - ex), max(0, v0 - ey), min(W - 1, u1 + ex), min(H - 1, v1 + ey)); (W, H, -1, -1) past the candidates

The product is cut at 2^15 before it becomes an integer: an image side is below 2^15, so every cut product clips to the
whole side as the uncut one would, and no r overflows."""
import numpy as np

EXPAND_CUT = 32768.0


def unpack(words, n):
    """uint64 [R][>= ceil(n / 64)] -> bool [R][n]."""
    words = np.ascontiguousarray(words).view(np.uint64)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def pack(bits, n_words=None):
    """bool [R][n] -> uint64 [R][n_words] (default ceil(n / 64)), padding bits zero."""
    r, n = bits.shape
    nw = (n + 63) // 64 if n_words is None else n_words
    full = np.zeros((r, nw * 64), bool)
    full[:, :n] = bits
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64).reshape(r, nw)


def table_from_dense(vis, u, v, stride_words):
    """vis bool [F][n], u and v int [F][n] (read where vis) -> (vis_mask, vis_off, vis_pix) in the table's layout."""
    f, n = vis.shape
    mask = pack(vis, stride_words)
    counts = unpack(mask, stride_words * 64).reshape(f, stride_words, 64).sum(axis=2).reshape(-1)
    off = (np.cumsum(counts) - counts).astype(np.uint32).reshape(f, stride_words)
    pix = [(np.asarray(u[s])[vis[s]].astype(np.int64) | (np.asarray(v[s])[vis[s]].astype(np.int64) << 16)) for s in range(f)]
    return mask, off, (np.concatenate(pix) if pix else np.zeros(0, np.int64)).astype(np.uint32)


def slot_pixels(mask, off, pix, slot, n_points):
    """One slot read as the kernels read it -> (visible bool [n], u int64 [n], v int64 [n]; 0 where not visible): the pair
    of point 64 w + l is entry off[slot][w] + (set bits of word w below l) of vis_pix."""
    words = unpack(mask[slot:slot + 1], mask.shape[1] * 64).reshape(-1, 64)
    assert not words.reshape(-1)[n_points:].any(), "bits beyond the last point"
    rank = np.cumsum(words, axis=1) - words
    at = (off[slot].astype(np.int64)[:, None] + rank)[words]
    p = pix[at].astype(np.int64)
    vis = words.reshape(-1)[:n_points]
    u, v = np.zeros(n_points, np.int64), np.zeros(n_points, np.int64)
    u[vis], v[vis] = p & 0xffff, p >> 16
    return vis, u, v


def instance_views(rows, mask, off, pix, n_points, height, width):
    """-> (visible int32 [K][F], box int32 [K][F][4], area int32 [K])."""
    bits = unpack(rows, n_points) if n_points else np.zeros((rows.shape[0], 0), bool)
    k, f = bits.shape[0], mask.shape[0]
    visible = np.zeros((k, f), np.int32)
    box = np.tile(np.array([width, height, -1, -1], np.int32), (k, f, 1))
    for s in range(f):
        vis, u, v = slot_pixels(mask, off, pix, s, n_points)
        idx = np.flatnonzero(vis)
        sel = bits[:, idx]                                              # [K][visible points of the slot]
        visible[:, s] = sel.sum(axis=1)
        if idx.size:
            us, vs = u[idx][None, :], v[idx][None, :]
            box[:, s, 0] = np.where(sel, us, width).min(axis=1)
            box[:, s, 1] = np.where(sel, vs, height).min(axis=1)
            box[:, s, 2] = np.where(sel, us, -1).max(axis=1)
            box[:, s, 3] = np.where(sel, vs, -1).max(axis=1)
    return visible, box, bits.sum(axis=1).astype(np.int32)


def instance_views_loop(rows, mask, off, pix, n_points, height, width):
    """The same, point by point and bit by bit in plain Python (the statement's check)."""
    k, f = rows.shape[0], mask.shape[0]
    visible = np.zeros((k, f), np.int32)
    box = np.tile(np.array([width, height, -1, -1], np.int32), (k, f, 1))
    for s in range(f):
        for p in range(n_points):
            w, l = divmod(p, 64)
            m = int(mask[s, w])
            if not (m >> l) & 1:
                continue
            at = int(off[s, w]) + bin(m & ((1 << l) - 1)).count("1")
            u, v = int(pix[at]) & 0xffff, int(pix[at]) >> 16
            for i in range(k):
                if (int(rows[i, w]) >> l) & 1:
                    visible[i, s] += 1
                    b = box[i, s]
                    b[0], b[1], b[2], b[3] = min(b[0], u), min(b[1], v), max(b[2], u), max(b[3], v)
    return visible, box


def expansion(extent, r, level):
    """(int)floor((double)extent * r) * level, the product cut at 2^15."""
    return int(min(np.floor(np.float64(int(extent)) * np.float64(r)), EXPAND_CUT)) * int(level)


def crop(b, height, width, r, level):
    u0, v0, u1, v1 = (int(x) for x in b)
    ex, ey = expansion(u1 - u0, r, level), expansion(v1 - v0, r, level)
    return max(0, u0 - ex), max(0, v0 - ey), min(width - 1, u1 + ex), min(height - 1, v1 + ey)


def select_views(visible, box, height, width, top_k=5, min_points=1, levels=3, expand=0.1):
    """-> (top int32 [K][T], top_visible int32 [K][T], crops int32 [K][T][L][4])."""
    k, f = visible.shape
    top = np.full((k, top_k), -1, np.int32)
    top_visible = np.zeros((k, top_k), np.int32)
    crops = np.tile(np.array([width, height, -1, -1], np.int32), (k, top_k, levels, 1))
    need = max(1, int(min_points))
    for i in range(k):
        cand = [s for s in range(f) if visible[i, s] >= need]
        cand.sort(key=lambda s: (-int(visible[i, s]), s))
        for t, s in enumerate(cand[:top_k]):
            top[i, t], top_visible[i, t] = s, visible[i, s]
            for l in range(levels):
                crops[i, t, l] = crop(box[i, s], height, width, expand, l)
    return top, top_visible, crops


def scene_views(rows, mask, off, pix, n_points, height, width, top_k=5, min_points=1, levels=3, expand=0.1):
    """Everything views.scene_views returns as arrays, by name."""
    visible, box, area = instance_views(rows, mask, off, pix, n_points, height, width)
    top, top_visible, crops = select_views(visible, box, height, width, top_k, min_points, levels, expand)
    return dict(area=area, visible=visible, boxes=box, top=top, top_visible=top_visible, crops=crops)
