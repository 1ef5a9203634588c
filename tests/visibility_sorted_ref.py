"""The pixel-sorted companion of the visibility table (bff_visibility_sorted, include/bff_hip.h) restated in NumPy, and a
brute-force statement of what the run-major sweep (bff_project_views_runs) computes.  Host only.

The companion orders the visible pairs of every depth slot by (flat pixel, point):

  spix      uint32 [pairs]            flat pixel v * W + u
  spt       uint32 [pairs]            point index
  rowstart  uint32 [n_slots][H + 1]   absolute position of the slot's first pair with pixel >= y * W; entry H is the slot's end

The pairs of visibility_ref.table come in (slot, point) order, so ONE stable sort on slot * H * W + pixel gives the order."""
import numpy as np

import visibility_ref as vr


def pairs_of(mask, off, pix, width):
    """The table's pairs in table order -> (slot int64 [pairs], point int64 [pairs], flat pixel int64 [pairs])."""
    n_slots, stride = mask.shape
    bits = np.unpackbits(mask.view(np.uint8).reshape(n_slots, -1), axis=1, bitorder="little")
    slot, point = np.nonzero(bits)                       # row-major: (slot, point) ascending = the table's order
    assert slot.size == pix.size and (off.reshape(-1)[0] == 0 if off.size else True)
    p = pix.astype(np.int64)
    return slot.astype(np.int64), point.astype(np.int64), (p >> 16) * width + (p & 0xffff)


def companion(mask, off, pix, height, width):
    """(vis_mask, vis_off, vis_pix) of visibility_ref.table -> (spix uint32, spt uint32, rowstart uint32 [S][H + 1])."""
    n_slots = mask.shape[0]
    slot, point, flat = pairs_of(mask, off, pix, width)
    hw = height * width
    key = slot * hw + flat
    order = np.argsort(key, kind="stable")
    key = key[order]
    edges = (np.arange(n_slots)[:, None] * hw + np.arange(height + 1)[None, :] * width).reshape(-1)
    rowstart = np.searchsorted(key, edges, side="left").reshape(n_slots, height + 1)
    return flat[order].astype(np.uint32), point[order].astype(np.uint32), rowstart.astype(np.uint32)


def dense_masks(runs, n_pixels):
    """runs: per mask a list of (start, end) -> bool [m][n_pixels]."""
    out = np.zeros((len(runs), n_pixels), bool)
    for m, rr in enumerate(runs):
        for a, b in rr:
            out[m, a:b] = True
    return out


def run_tables(runs):
    """-> (run_start int32, run_end int32, mask_run_offs int32 [m + 1])."""
    flat = [r for rr in runs for r in rr]
    offs = np.concatenate([[0], np.cumsum([len(rr) for rr in runs])]).astype(np.int32)
    return np.array([a for a, _ in flat], np.int32), np.array([b for _, b in flat], np.int32), offs


def membership_sweep(xyz, poses, k33, depths, thresh, depth_index, frame_mask, frame_flags, cover):
    """The sweep by brute force, one view of masks `cover` (bool [m][H * W]) on every frame with frame_mask >= 0:
    -> (rows uint64 [frames with masks * m][nw], chunk_mask uint64 [rows][mw], masked int32 [n], viewed int32 [n])."""
    n = xyz.shape[0]
    nw = (n + 63) // 64
    n_chunks = (nw + 7) // 8
    mw = (n_chunks + 63) // 64
    m = cover.shape[0]
    width = depths.shape[2]
    dense, viewed = [], np.zeros(n, np.int32)
    for f, s in enumerate(depth_index):
        vis, u, v, _why = vr.frame_visibility(xyz, poses[s], k33, depths[s], thresh)
        if frame_flags[f] & 1:
            viewed += vis
        if frame_mask[f] >= 0:
            dense.append(cover[:, v * width + u] & vis[None, :])        # [m][n]
    bits = np.zeros((len(dense) * m, n_chunks * 512), bool)
    bits[:, :n] = np.concatenate(dense, axis=0)
    rows = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)[:, :nw]
    flags = np.zeros((bits.shape[0], mw * 64), bool)
    flags[:, :n_chunks] = bits.reshape(bits.shape[0], n_chunks, 512).any(axis=2)
    cmask = np.packbits(flags, axis=1, bitorder="little").view(np.uint64)
    return np.ascontiguousarray(rows), cmask, bits[:, :n].sum(axis=0, dtype=np.int32), viewed


# ---------------------------------------------------------------------------------------------------------------
# The hand-made case over visibility_ref's 24 x 32 image: seven frames over its six slots and one view of nine masks.
HW = vr.H * vr.W
DEPTH_INDEX = np.array([2, 0, 5, 3, 1, 4, 0], np.int32)          # another order than the slots; slot 0 twice
FRAME_MASK = np.array([0, 0, 0, 0, 0, 0, -1], np.int32)          # the last frame is viewed only
FRAME_FLAGS = np.array([1, 1, 0, 1, 3, 1, 1], np.int32)          # frame 2 has masks and does not count as viewed


def hand_masks(free_pixel):
    return [[(40, 100)],                                         # crosses two row ends
            [(0, HW)],                                           # the whole image
            [(0, 1), (HW - 1, HW)],                              # one pixel at each end
            [(10, 20), (45, 50), (300, 420)],
            [],                                                  # no runs, between two masks that have some
            [(200, 260)],
            [(free_pixel, free_pixel + 1)],                      # hits no visible point
            [(500, 540), (600, 610)],
            [(500, 540), (600, 610)]]                            # identical to the one before
