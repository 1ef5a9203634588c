"""NumPy statements of bff_point_labels, bff_render_labels_u16 and the label image -> run tables step
(include/bff_hip.h).  TEST INFRASTRUCTURE ONLY.

Which points take part, their texels and millimetres are render_depth_ref.splats'; the footprints are
splat_depth_ref.footprints'; the z-buffer is np.minimum.at on the keys (m << 16) | label.
"""
import numpy as np

import render_depth_ref as rd
import splat_depth_ref as sd
from oracle import geom_fma

EMPTY = rd.EMPTY


def point_labels_ref(dense_rows, unsort=None):
    """dense_rows bool (K, N) -> uint16 (N,): 1 + the first row that holds the point, 0 = none; unsort: the value of
    point o goes to position unsort[o]."""
    dense_rows = np.asarray(dense_rows, bool)
    k, n = dense_rows.shape
    lab = np.zeros(n, np.uint16)
    for r in range(k - 1, -1, -1):
        lab[dense_rows[r]] = r + 1
    if unsort is None:
        return lab
    out = np.zeros(n, np.uint16)
    out[np.asarray(unsort, np.int64)] = lab
    return out


def taking_part(xyz, inv_pose, k33, height, width):
    """Indices of the points that take part in one frame, in the order of rd.splats / sd.footprints."""
    pts, pix, _ = geom_fma.view(xyz, np.asarray(inv_pose, np.float64).reshape(4, 4), np.asarray(k33, np.float64),
                                np.zeros((1, 1), np.float32))
    with np.errstate(all="ignore"):
        m = np.rint(pts[:, 2] * 1000.0)
        return np.flatnonzero((pix[:, 0] >= 0) & (pix[:, 0] < width) & (pix[:, 1] >= 0) & (pix[:, 1] < height) &
                              (pts[:, 2] > 0) & (m >= 1) & (m <= 65535))


def render_labels_ref(xyz, lab, inv_poses, k33, height, width, depth_h, depth_w, radius=0.0):
    """-> (labels, depth) uint16 [F][depth_h][depth_w]: the low and the high half of the minimum key of every texel, 0 in
    both where nothing was offered.  radius 0: own texels only (bff_render_depth_u16's); > 0: footprints as well."""
    xyz = np.asarray(xyz, np.float64)[:, :3]
    lab = np.asarray(lab).astype(np.uint32)
    assert lab.shape == (xyz.shape[0],) and int(lab.max(initial=0)) <= 65534
    inv_poses = np.asarray(inv_poses, np.float64).reshape(-1, 16)
    labels = np.zeros((inv_poses.shape[0], depth_h, depth_w), np.uint16)
    depth = np.zeros_like(labels)
    for f, inv in enumerate(inv_poses):
        texel, mm = rd.splats(xyz, inv, k33, height, width, depth_h, depth_w)
        part = taking_part(xyz, inv, k33, height, width)
        assert part.shape == mm.shape
        key = (mm.astype(np.uint32) << np.uint32(16)) | lab[part]
        buf = np.full(depth_h * depth_w, EMPTY, np.uint32)
        np.minimum.at(buf, texel, key)                                     # own texel
        buf = buf.reshape(depth_h, depth_w)
        if radius > 0:
            cols, rows, m = sd.footprints(xyz, inv, k33, height, width, depth_h, depth_w, radius)
            assert np.array_equal(m, mm)
            j0, nj, i0, ni = cols.argmax(1), cols.sum(1), rows.argmax(1), rows.sum(1)
            for p in np.flatnonzero((nj > 0) & (ni > 0)):
                box = buf[i0[p]:i0[p] + ni[p], j0[p]:j0[p] + nj[p]]
                np.minimum(box, key[p], out=box)
        hit = buf != EMPTY
        labels[f] = np.where(hit, buf & np.uint32(0xFFFF), 0).astype(np.uint16)
        depth[f] = np.where(hit, buf >> np.uint32(16), 0).astype(np.uint16)
    return labels, depth


def upsample(labels, height, width):
    """up[f][v][u] = labels[f][(v * dh) // height][(u * dw) // width]."""
    labels = np.asarray(labels)
    _, dh, dw = labels.shape
    return labels[:, (np.arange(height) * dh) // height][:, :, (np.arange(width) * dw) // width]


def label_runs_ref(labels, height, width, min_pixels=1):
    """-> (run_start, run_end, mask_run_offs, mask_label, frame_offs) as int32 arrays / a list: masks (f, L) in that
    order for every label L >= 1 covering at least max(1, min_pixels) pixels of frame f; runs = maximal intervals of
    the flat index with up == L."""
    up = upsample(np.asarray(labels).astype(np.int64) & 0xFFFF, height, width)
    starts, ends, offs, mask_label, frame_offs = [], [], [0], [], [0]
    for f in range(up.shape[0]):
        flat = up[f].reshape(-1)
        for lab in np.unique(flat):
            if lab < 1:
                continue
            m = flat == lab
            if int(m.sum()) < max(1, int(min_pixels)):
                continue
            d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
            s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
            starts.append(s), ends.append(e)
            offs.append(offs[-1] + len(s))
            mask_label.append(int(lab) - 1)
        frame_offs.append(len(mask_label))
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return cat(starts), cat(ends), np.asarray(offs, np.int32), np.asarray(mask_label, np.int32), frame_offs


# ------------------------------------------------------------------ the cloud the renderer's tests share
R = 0.03125                                                              # 2^-5, test_gpu_splat_depth's radius
# pixels of frame 0 (the identity pose) that hold the crafted pairs, all at z = 0.3 m: nearer than every random point
PIX_TIE, PIX_TIE_BG, PIX_BEHIND, PIX_FRONT = (10, 10), (20, 10), (10, 40), (20, 40)     # (u, v)
PAD_LABEL = 7


def label_cloud(k):
    """test_gpu_splat_depth.cloud() (1500 points in 2048 slots, 9 poses, its crafted points) with its last 8 points
    replaced by four crafted pairs, and labels in [0, k] for all of them, about half background.
    -> (xyz (N, 3), inv (F, 16), soa (3, N_PAD), lab uint16 (N_PAD,)): lab[N:] = PAD_LABEL on the padding's point, which
    would cover much of frame 0 if it were read.  The pairs, at one pixel each:
        PIX_TIE      equal m, labels 2 and min(5, k)         -> 2
        PIX_TIE_BG   equal m, background and a label         -> 0
        PIX_BEHIND   a label 1 mm behind a background point  -> 0
        PIX_FRONT    a background point 1 mm behind a label  -> the label"""
    import test_gpu_splat_depth as tg
    xyz, inv, soa = tg.cloud()
    xyz, soa = xyz.copy(), soa.copy()
    n = xyz.shape[0]
    hi = min(5, k)
    pairs = [(PIX_TIE, 0.3, 2), (PIX_TIE, 0.3, hi), (PIX_TIE_BG, 0.3, hi), (PIX_TIE_BG, 0.3, 0),
             (PIX_BEHIND, 0.3, 0), (PIX_BEHIND, 0.301, hi), (PIX_FRONT, 0.301, 0), (PIX_FRONT, 0.3, hi)]
    rng = np.random.default_rng(100 + k)
    lab = np.where(rng.random(n) < 0.5, 0, rng.integers(1, k + 1, n)).astype(np.uint16)
    for i, ((u, v), z, l) in enumerate(pairs):
        xyz[n - 8 + i] = tg.at_pixel(u, v, z)
        lab[n - 8 + i] = l
    soa[:, :n] = xyz.T
    pad = np.full(soa.shape[1], PAD_LABEL, np.uint16)
    pad[:n] = lab
    return xyz, inv, soa, pad
