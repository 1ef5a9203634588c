"""Visibility tables written directly in NumPy -- no cloud, no poses, no depth -- and what the cached sweeps
(bff_project_views_cached, bff_project_views_runs) must make of them, by brute force.  Host only.

The three entry points of the cached sweeps take the table (vis_mask, vis_off, vis_pix) as plain arrays, so a table of any
size, density and crowding can be stated here and swept by table_sweep(); visibility_sorted_ref.companion() states the
pixel-sorted companion of any table.  CASES are the tables tests/test_gpu_cached_sweeps_synth.py runs on: the sizes at
which the kernels do something the small geometric cases never reach (regime(): conditions on the input, asserted with
and without a GPU)."""
import functools

import numpy as np

import visibility_ref as vr
import visibility_sorted_ref as sr


def synthetic_table(n_points, densities, height, width, rng, hot_share=0.0, hot_pixels=4):
    """-> (vis_mask uint64 [S][stride], vis_off uint32 [S][stride], vis_pix uint32 [pairs]) in visibility_ref.table's layout.
    Slot s marks a point visible with probability densities[s] (0.0: no pair, 1.0: every point).  A pair's flat pixel is
    uniform over the image, but a share hot_share of the pairs sits on one of hot_pixels hot pixels: 0, H * W - 1, W - 1 and
    W (both sides of the first row end), then random ones.  Pixels are packed u | v << 16."""
    n_slots, stride, hw = len(densities), vr.stride_words(n_points), height * width
    assert hot_pixels >= 4 and hw > width
    hot = np.concatenate([[0, hw - 1, width - 1, width], rng.integers(0, hw, hot_pixels - 4)]).astype(np.int64)
    bits = np.zeros((n_slots, stride * 64), bool)
    pix = []
    for s, d in enumerate(densities):
        if d <= 0.0:
            continue
        vis = np.ones(n_points, bool) if d >= 1.0 else rng.random(n_points) < d
        k = int(vis.sum())
        flat = rng.integers(0, hw, k)
        is_hot = rng.random(k) < hot_share
        flat[is_hot] = hot[rng.integers(0, hot.size, int(is_hot.sum()))]
        bits[s, :n_points] = vis
        pix.append(((flat % width) | ((flat // width) << 16)).astype(np.uint32))       # ascending point order
    mask = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n_slots, stride)
    counts = bits.reshape(n_slots, stride, 64).sum(axis=2).reshape(-1)
    off = (np.cumsum(counts) - counts).astype(np.uint32).reshape(n_slots, stride)
    return mask, off, np.concatenate(pix) if pix else np.zeros(0, np.uint32)


def slot_pairs(mask, off, pix, slot, n_points, width):
    """One slot of a table read as the sweep reads it -> (visible bool [n], flat pixel int64 [n], -1 where not visible):
    the pair of point 64 w + l is entry off[slot][w] + (set bits of word w below l) of vis_pix."""
    words = np.unpackbits(mask[slot].view(np.uint8), bitorder="little").reshape(-1, 64).astype(bool)
    assert not words.reshape(-1)[n_points:].any(), "bits beyond the last point"
    rank = np.cumsum(words, axis=1) - words                                    # set bits below each lane
    at = (off[slot].astype(np.int64)[:, None] + rank)[words]
    p = pix[at].astype(np.int64)
    vis = words.reshape(-1)[:n_points]
    flat = np.full(n_points, -1, np.int64)
    flat[vis] = (p >> 16) * width + (p & 0xffff)
    return vis, flat


def frame_layout(frame_mask, covers):
    """-> (frame_rowbase int32 [F], frame_nmask int32 [F]) as membership_sweep lays rows out: the masks of a frame's view
    one after another, frames in order, nothing for a frame without masks."""
    frame_mask = np.asarray(frame_mask)
    nmask = np.array([covers[v].shape[0] if v >= 0 else 0 for v in frame_mask], np.int32)
    return (np.cumsum(nmask) - nmask).astype(np.int32), nmask


def table_sweep(mask, off, pix, n_points, width, depth_index, frame_mask, frame_flags, covers):
    """The cached sweep by brute force.  covers: per mask view a bool [m][H * W].  Point p is in the row of (frame f, mask m)
    iff p's bit is set in slot depth_index[f] and covers[frame_mask[f]][m] holds the pair's pixel.
    -> (rows uint64 [n_rows][nw], chunk_mask uint64 [n_rows][mw], masked int32 [n], viewed int32 [n]); viewed counts the slot
    bits of the frames with flag bit 0, masked is the column sum of the rows."""
    n = n_points
    nw = (n + 63) // 64
    n_chunks = (nw + 7) // 8
    mw = (n_chunks + 63) // 64
    rowbase, nmask = frame_layout(frame_mask, covers)
    n_rows = int(nmask.sum())
    bits = np.zeros((n_rows, n_chunks * 512), bool)
    viewed = np.zeros(n, np.int32)
    for f, s in enumerate(depth_index):
        vis, flat = slot_pairs(mask, off, pix, int(s), n, width)
        if frame_flags[f] & 1:
            viewed += vis
        if frame_mask[f] >= 0:
            idx = np.flatnonzero(vis)
            bits[rowbase[f]:rowbase[f] + nmask[f], idx] = covers[frame_mask[f]][:, flat[idx]]
    rows = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n_rows, -1)[:, :nw]
    flags = np.zeros((n_rows, mw * 64), bool)
    flags[:, :n_chunks] = bits.reshape(n_rows, n_chunks, 512).any(axis=2)
    cmask = np.packbits(flags, axis=1, bitorder="little").view(np.uint64).reshape(n_rows, mw)
    return np.ascontiguousarray(rows), cmask, bits[:, :n].sum(axis=0, dtype=np.int32), viewed


# ---------------------------------------------------------------------------------------------------------------
# masks
def mask_view(m, height, width, rng, noise=0.3, speckle=0.1):
    """One view of m masks, bool [m][H * W], its kinds in turn:
      0  noise of density `noise`: several runs per image row
      1  no runs at all -- between two masks that have some
      2  mask 0 again: two identical masks
      3  one run across several row ends; the image rows below it speckled with density `speckle` (a mask of few runs)
      4  a rectangle
      5  the two one-pixel runs [0, 1) and [H * W - 1, H * W)
    and from 6 on the same again with fresh noise."""
    hw = height * width
    out = np.zeros((m, hw), bool)
    for i in range(m):
        kind = i % 6
        if kind == 0:
            out[i] = rng.random(hw) < noise
        elif kind == 2:
            out[i] = out[i - 2]
        elif kind == 3:
            start = int(rng.integers(0, max(height // 4, 1))) * width + width - 3
            end = min(start + 3 * width + 7, hw)
            out[i, start:end] = True
            below = ((end - 1) // width + 2) * width                 # one clear image row under the run
            if below < hw:
                out[i, below:] = rng.random(hw - below) < speckle
        elif kind == 4:
            r0, c0 = int(rng.integers(0, height - 2)), int(rng.integers(0, width - 2))
            r1, c1 = int(rng.integers(r0 + 2, height + 1)), int(rng.integers(c0 + 2, width + 1))
            box = np.zeros((height, width), bool)
            box[r0:r1, c0:c1] = True
            if box.all():
                box[0] = False
            out[i] = box.reshape(-1)
        elif kind == 5:
            out[i, 0] = out[i, hw - 1] = True
    return out


def runs_of(dense):
    """dense bool [G][H * W] -> (run_start, run_end, mask_run_offs) int32: the maximal runs, which are sorted, disjoint and
    non-empty per mask -- what the look-up form requires and scene.runs_from_rles delivers."""
    d = np.diff(np.pad(dense.astype(np.int8), ((0, 0), (1, 1))), axis=1)
    g, start = np.nonzero(d == 1)                                     # row-major: per mask, ascending
    _g, end = np.nonzero(d == -1)
    offs = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=dense.shape[0]))])
    return start.astype(np.int32), end.astype(np.int32), offs.astype(np.int32)


def run_tables(covers):
    """The views of one mask set -> (run_start, run_end, mask_run_offs, view_mask_offs) int32 over all masks of all views."""
    rs, re, offs = runs_of(np.concatenate(covers, axis=0))
    voffs = np.concatenate([[0], np.cumsum([c.shape[0] for c in covers])]).astype(np.int32)
    return rs, re, offs, voffs


# ---------------------------------------------------------------------------------------------------------------
# The cases.  In each of them the frames read the slots in another order than the slots, one slot is read twice and one
# never, one frame has no masks (frame_mask -1) and one frame with masks lacks flag bit 0.  `sets`: word_bits -> the mask
# counts of that mask set's views; frame_mask indexes the views of whichever set is swept.
_SHARED = dict(h=30, w=50, sets={32: [6], 64: [6]}, depth_index=[1, 2, 1], frame_mask=[0, 0, -1], frame_flags=[1, 2, 1],
               hot_share=0.05, hot_pixels=6)
KEY32_SLOTS = 1032
CASES = {
    # width and pixel count that divide nothing
    "odd": dict(n=5000, h=37, w=41, densities=[0.3, 0.0, 1.0, 0.05, 0.5, 0.2, 0.01], sets={64: [3, 33, 64], 32: [1, 17, 32]},
                depth_index=[4, 2, 0, 1, 5, 2, 6], frame_mask=[0, 1, 2, 0, 1, -1, 2], frame_flags=[1, 1, 0, 3, 1, 1, 1],
                hot_share=0.2, hot_pixels=8, seed=101),
    # nw = 2050 (no multiple of 4 or 8), 257 chunks: the flush loop's second trip, a fifth word of chunk flags
    "flush2": dict(_SHARED, n=131_137, densities=[0.2, 1.0, 0.0], seed=102),
    # a row of exactly 64 KB of LDS, point indices up to 2^19 - 1, 5 x 10^5 pairs of one slot over 1500 pixels
    "bound": dict(_SHARED, n=524_288, densities=[0.1, 1.0, 0.02], sets={32: [6]}, seed=103),
    # one point more: the run-major form refuses
    "over": dict(_SHARED, n=524_289, densities=[0.1, 1.0, 0.02], sets={64: [6]}, seed=104),
    # 2^31 < slots * H * W <= 2^32 < (slots + 1) * H * W: a sort key of all 32 bits
    "key32": dict(n=1000, h=1600, w=2600, densities={0: 1.0, KEY32_SLOTS // 2: 0.5, KEY32_SLOTS - 1: 0.7}, n_slots=KEY32_SLOTS,
                  sets={32: [6]}, depth_index=[KEY32_SLOTS - 1, 0, KEY32_SLOTS // 2, 0], frame_mask=[0, 0, 0, -1],
                  frame_flags=[1, 2, 1, 1], hot_share=0.5, hot_pixels=4, seed=105),
}


class Case:
    """One case on the host: the table, its mask sets with their run tables, and the expected sweep per word size."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.n, self.h, self.w = name, c["n"], c["h"], c["w"]
        rng = np.random.default_rng(c["seed"])
        dens = c["densities"]
        if isinstance(dens, dict):
            dens = [dens.get(s, 0.0) for s in range(c["n_slots"])]
        self.densities = dens
        self.n_slots = len(dens)
        self.table = synthetic_table(self.n, dens, self.h, self.w, rng, c["hot_share"], c["hot_pixels"])
        self.pairs = int(self.table[2].size)
        self.depth_index = np.array(c["depth_index"], np.int32)
        self.frame_mask = np.array(c["frame_mask"], np.int32)
        self.frame_flags = np.array(c["frame_flags"], np.int32)
        self.covers = {wb: [mask_view(m, self.h, self.w, rng) for m in counts] for wb, counts in c["sets"].items()}
        self.runs = {wb: run_tables(cv) for wb, cv in self.covers.items()}
        self.nw = (self.n + 63) // 64
        self.n_chunks = (self.nw + 7) // 8
        self.mw = (self.n_chunks + 63) // 64

    def layout(self, wb):
        return frame_layout(self.frame_mask, self.covers[wb])

    @functools.lru_cache(maxsize=None)
    def expected(self, wb):
        """table_sweep of the case's frames over mask set wb; computed once, never written to."""
        out = table_sweep(*self.table, self.n, self.w, self.depth_index, self.frame_mask, self.frame_flags, self.covers[wb])
        for a in out:
            a.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def companion(self):
        out = sr.companion(*self.table, self.h, self.w)
        for a in out:
            a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def get(name):
    return Case(name)


def bit(rows, p):
    """bool [n_rows]: point p's bit."""
    return ((rows[:, p >> 6] >> np.uint64(p & 63)) & np.uint64(1)).astype(bool)


def regime(case, groups=True):
    """The figures that say which code a case reaches, all from the reference:
      runs_per_mask    run counts of all masks of all sets
      group_pairs      over every (frame with masks, mask) and every group of 64 consecutive runs counted from the mask's
                       first run -- what one wave of the run-major fill takes at a time: the pairs the group covers
      group_pairs_sparse  the same, of the frames whose slot has pairs, but fewer than 64
      pixel_pairs      most pairs of one slot on one pixel
      largest_key      largest slot * H * W + pixel over the pairs"""
    hw = case.h * case.w
    slot, _point, flat = sr.pairs_of(*case.table, case.w)
    counts = np.bincount(slot, minlength=case.n_slots)
    starts = np.cumsum(counts) - counts
    runs_per_mask, group_pairs, sparse, pixel_pairs = [], [], [], 0
    cum = {}
    for s in np.flatnonzero(counts):
        hist = np.bincount(flat[starts[s]:starts[s] + counts[s]], minlength=hw)
        pixel_pairs = max(pixel_pairs, int(hist.max()))
        if groups:
            cum[int(s)] = np.concatenate([[0], np.cumsum(hist)])
    for wb, (rs, re, offs, voffs) in case.runs.items():
        runs_per_mask += np.diff(offs).tolist()
        for f, view in enumerate(case.frame_mask):
            if view < 0 or not groups:
                continue
            c = cum.get(int(case.depth_index[f]), np.zeros(hw + 1, np.int64))
            for g in range(voffs[view], voffs[view + 1]):
                if offs[g] < offs[g + 1]:
                    per_run = c[re[offs[g]:offs[g + 1]]] - c[rs[offs[g]:offs[g + 1]]]
                    sums = np.add.reduceat(per_run, np.arange(0, per_run.size, 64)).tolist()
                    group_pairs += sums
                    if 0 < c[-1] < 64:
                        sparse += sums
    return dict(group_pairs_sparse=np.array(sparse), runs_per_mask=np.array(runs_per_mask), group_pairs=np.array(group_pairs), pixel_pairs=pixel_pairs,
                largest_key=int((slot * hw + flat).max()))


def assert_regime(case):
    """The conditions on the input that keep each case where it was put; none of them is a measurement."""
    name, n, h, w = case.name, case.n, case.h, case.w
    r = regime(case, groups=name != "key32")
    assert (case.frame_mask < 0).any() and ((case.frame_mask >= 0) & (case.frame_flags & 1 == 0)).any()
    read = case.depth_index.tolist()
    assert read != sorted(read) and len(set(read)) < len(read) and len(set(read)) < case.n_slots
    assert r["pixel_pairs"] >= 64, "no crowded pixel: stability of the sort decides nothing"
    if name == "key32":
        hw = h * w
        assert h < 1 << 15 and w < 1 << 15 and h & (h - 1) and w & (w - 1)
        assert 1 << 31 < case.n_slots * hw <= 1 << 32 < (case.n_slots + 1) * hw
        assert r["largest_key"] >= 1 << 31
        _slot, _point, flat = sr.pairs_of(*case.table, w)
        assert (flat == 0).any() and (flat == hw - 1).any()
        assert {s for s, d in enumerate(case.densities) if d > 0} == {0, case.n_slots // 2, case.n_slots - 1}
        return
    assert (r["runs_per_mask"] > 256).any() and ((r["runs_per_mask"] >= 65) & (r["runs_per_mask"] <= 255)).any()
    assert (r["group_pairs"] > 256).any(), "no wave of the fill deals out more than one round of pairs"
    if min(case.densities) <= 0.0:              # the case reads a slot without pairs
        assert (r["group_pairs"] == 0).any()
    if name == "odd":
        assert w & (w - 1) != 0 and (h * w) % 64 != 0
        assert (r["group_pairs_sparse"] == 0).any(), "no wave of the fill finds nothing in a slot that has pairs"
        assert {wb: [c.shape[0] for c in cv] for wb, cv in case.covers.items()} == {64: [3, 33, 64], 32: [1, 17, 32]}
    if name == "flush2":
        assert case.nw == 2050 and case.n_chunks == 257 and case.mw == 5
        for wb in case.covers:
            rows, cmask, _m, _v = case.expected(wb)
            assert rows[:, 256 * 8:].any() and (cmask[:, 4] & np.uint64(1)).any(), "chunk 256 is empty in every row"
    if name == "bound":
        assert 8 * case.n_chunks * 8 == 65536 and n - 1 == (1 << 19) - 1
        for wb in case.covers:
            rows = case.expected(wb)[0]
            assert bit(rows, n - 1).any() and rows[:, (1 << 18) // 64:].any()
    if name == "over":
        assert 8 * case.n_chunks * 8 > 65536 and n == (1 << 19) + 1
