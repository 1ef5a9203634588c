"""NumPy statement of the 2-D masks' row directory (beyond_fixed_forms_amd/csrc/mask_rows.h, bff_mask_row_directory) and
of the look-up the sweep makes in it, plus the hand-made mask views the tests of both share.

Run tables as everywhere in the project: per mask sorted, disjoint, non-empty runs [start, end) of flattened row-major
pixel indices inside [0, H * W); mask g owns runs [offs[g], offs[g + 1])."""
import numpy as np

ROW_FLAG = 1 << 31
COUNT_SHIFT = 27
COUNT_SAT = 15
FIRST_MASK = (1 << COUNT_SHIFT) - 1
LINEAR = 4
EMPTY_BOX = 0xFFFFFFFF


def runs_of(dense):
    """dense bool [G][H * W] -> (run_start, run_end, offs) int32, maximal runs."""
    rs, re, offs = [], [], [0]
    for m in dense:
        d = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
        rs += np.flatnonzero(d == 1).tolist()
        re += np.flatnonzero(d == -1).tolist()
        offs.append(len(rs))
    return np.asarray(rs, np.int32), np.asarray(re, np.int32), np.asarray(offs, np.int32)


def dense_of(rs, re, offs, hw):
    """The dense decode of run tables: bool [G][hw]."""
    out = np.zeros((len(offs) - 1, hw), bool)
    for g in range(len(offs) - 1):
        for a, b in zip(rs[offs[g]:offs[g + 1]], re[offs[g]:offs[g + 1]]):
            out[g, a:b] = True
    return out


def row_directory_ref(rs, re, offs, height, width):
    """-> (tab uint32 [G + 1][4], directory uint32 [sum of the boxes' heights])."""
    n = len(offs) - 1
    tab = np.zeros((n + 1, 4), np.uint32)
    entries = []
    for g in range(n):
        lo, hi = int(offs[g]), int(offs[g + 1])
        if hi == lo:
            tab[g] = (EMPTY_BOX, 0, len(entries), lo)
            continue
        s, e = rs[lo:hi].astype(np.int64), re[lo:hi].astype(np.int64)
        r0, r1 = int(s[0] // width), int((e[-1] - 1) // width)
        crosses = (s // width) != ((e - 1) // width)
        c0 = 0 if crosses.any() else int((s % width).min())
        c1 = width - 1 if crosses.any() else int(((e - 1) % width).max())
        tab[g] = (c0 | (r0 << 16), c1 | (r1 << 16), len(entries), lo)
        for r in range(r0, r1 + 1):
            row0, row1 = r * width, (r + 1) * width
            hit = np.flatnonzero((e > row0) & (s < row1))          # runs reaching into the row count
            if hit.size == 0:
                entries.append(0)
            elif hit.size == 1:
                k = hit[0]
                entries.append(int(max(s[k], row0) - row0) | (int(min(e[k], row1) - row0) << 15))
            else:
                first, count = int(hit[0]), min(int(hit.size), COUNT_SAT)
                if first > FIRST_MASK:
                    first, count = 0, COUNT_SAT
                entries.append(ROW_FLAG | (count << COUNT_SHIFT) | first)
    tab[n] = (EMPTY_BOX, 0, len(entries), int(offs[n]))
    return tab, np.asarray(entries, np.uint32)


def lookup_ref(tab, directory, rs, re, g, u, v, width):
    """Does mask g cover pixel (column u, row v)?  Box, then the row's entry, then -- flagged entries only -- the runs."""
    lo, hi, doff, first_run = (int(x) for x in tab[g])
    c0, r0, c1, r1 = lo & 0xFFFF, lo >> 16, hi & 0xFFFF, hi >> 16
    if not (c0 <= u <= c1 and r0 <= v <= r1):
        return False
    e = int(directory[doff + v - r0])
    if not e & ROW_FLAG:
        return (e & 0x7FFF) <= u < ((e >> 15) & 0x7FFF)
    count, a = (e >> COUNT_SHIFT) & COUNT_SAT, first_run + (e & FIRST_MASK)
    b = int(tab[g + 1][3]) if count == COUNT_SAT else a + count
    p = v * width + u
    if count <= LINEAR:
        return any(rs[i] <= p < re[i] for i in range(a, b))
    k = a + int(np.searchsorted(re[a:b], p, side="right"))         # first run that ends behind p
    return k < b and rs[k] <= p


def lookup_all_ref(tab, directory, rs, re, height, width):
    """Every pixel of every mask through lookup_ref: bool [G][H * W]."""
    n = tab.shape[0] - 1
    out = np.zeros((n, height * width), bool)
    for g in range(n):
        for v in range(height):
            for u in range(width):
                out[g, v * width + u] = lookup_ref(tab, directory, rs, re, g, u, v, width)
    return out


H, W = 23, 37           # neither a multiple of anything


def hand_view(n_masks=34, seed=5):
    """The first hand-made view: dense bool [n_masks][H * W] with every shape of row the directory distinguishes."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n_masks, H, W), bool)
    # 0: no pixel at all
    m[1, 0, 0] = True                                   # a single pixel at (0, 0)
    m[2, H - 1, W - 1] = True                           # the last pixel: run end == H * W
    m[3, 3, 30:W] = True                                # a run that ends exactly at a row end
    m[4, 5, 0:5] = True                                 # a run that starts at column 0
    m[5].reshape(-1)[7 * W + 20:11 * W + 10] = True     # three full rows and a partial row at both ends
    m[6, 2, 3:7] = m[6, 2, 10:16] = True                # a row with 2 runs
    m[6, 3, 1:4] = True
    for k in range(6):                                  # a row with 6 runs, a one-run row above and below
        m[7, 9, 5 * k:5 * k + 2] = True
    m[7, 8, 4:20] = m[7, 10, 0:W] = True
    m[8, 12, 0:W:2] = True                              # every other pixel: 19 runs, past the saturated count
    m[8, 13, 1:W:2] = True
    m[8, 11, 2:9] = True
    m[9, 14:19, 5:26] = m[10, 14:19, 5:26] = True       # two masks sharing every pixel
    for g in range(11, n_masks):                        # blobs with holes and speckle, several overlapping per pixel
        r0, c0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
        r1, c1 = int(rng.integers(r0 + 1, H + 1)), int(rng.integers(c0 + 1, W + 1))
        blob = rng.random((r1 - r0, c1 - c0)) < rng.choice([1.0, 0.9, 0.5])
        m[g, r0:r1, c0:c1] = blob
    return m.reshape(n_masks, -1)


def second_view(seed=6):
    """Three masks: a full-width band that crosses row ends, a column, speckle."""
    rng = np.random.default_rng(seed)
    m = np.zeros((3, H, W), bool)
    m[0].reshape(-1)[2 * W + 5:6 * W] = True
    m[1, :, 17] = True
    m[2] = rng.random((H, W)) < 0.3
    return m.reshape(3, -1)


def full_box_view(n_masks=64, seed=7):
    """Every mask's box is the whole image (it holds the first and the last pixel): every mask is a candidate everywhere."""
    rng = np.random.default_rng(seed)
    m = rng.random((n_masks, H * W)) < rng.choice([0.05, 0.5, 0.95], size=(n_masks, 1))
    m[:, 0] = m[:, -1] = True
    m[:, 1] = False                                     # the first pixel is a run of its own: no run crosses a row end there
    return m
