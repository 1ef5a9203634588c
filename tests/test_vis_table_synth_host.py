"""The table-level reference of the cached sweeps (tests/vis_table_synth.py), without a GPU.

(a) On the small geometric case table_sweep(), fed with visibility_ref.table(), equals the geometric brute force
    (visibility_sorted_ref.membership_sweep) for the hand-made masks and frames of tests/test_gpu_sweep_runs.py.
(b) Every synthetic case is built, its regime conditions hold, and its parts fit together: the generator does what it
    says, the mask views hold every kind, the run tables are what the look-up form requires."""
import numpy as np
import pytest

import vis_table_synth as vs
import visibility_ref as vr
import visibility_sorted_ref as sr


@pytest.mark.parametrize("n", [1500, 1100])
def test_table_sweep_equals_the_geometric_brute_force(n):
    case = vr.build_case()
    xyz = case["xyz"][:n]
    seen = np.zeros(sr.HW, bool)
    for s in range(vr.N_SLOTS):
        vis, u, v, _why = vr.frame_visibility(xyz, case["poses"][s], vr.K, case["depth"][s], vr.THRESH)
        seen[(v * vr.W + u)[vis]] = True
    cover = sr.dense_masks(sr.hand_masks(int(np.flatnonzero(~seen)[0])), sr.HW)
    exp = sr.membership_sweep(xyz, case["poses"], vr.K, case["depth"], vr.THRESH, sr.DEPTH_INDEX, sr.FRAME_MASK, sr.FRAME_FLAGS,
                              cover)
    tab = vr.table(xyz, case["poses"], vr.K, case["depth"], vr.THRESH)
    got = vs.table_sweep(*tab, n, vr.W, sr.DEPTH_INDEX, sr.FRAME_MASK, sr.FRAME_FLAGS, [cover])
    assert exp[0].any() and exp[2].any() and exp[3].any()
    for g, e, what in zip(got, exp, ("rows", "chunk_mask", "masked", "viewed")):
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), what
    rowbase, nmask = vs.frame_layout(sr.FRAME_MASK, [cover])
    m = cover.shape[0]
    assert np.array_equal(nmask, np.where(sr.FRAME_MASK >= 0, m, 0)) and np.array_equal(rowbase, np.cumsum(nmask) - nmask)
    # the maximal runs of the dense masks decode to the same masks as the hand-written runs
    rs, re, offs = vs.runs_of(cover)
    again = sr.dense_masks([list(zip(rs[offs[g]:offs[g + 1]], re[offs[g]:offs[g + 1]])) for g in range(m)], sr.HW)
    assert np.array_equal(again, cover)


def test_generator_takes_zero_and_one_literally_and_keeps_the_hot_pixels():
    h, w, n = 7, 13, 2000
    mask, off, pix = vs.synthetic_table(n, [0.0, 1.0, 0.25], h, w, np.random.default_rng(3), hot_share=0.5, hot_pixels=5)
    assert mask.shape == off.shape == (3, vr.stride_words(n)) and mask.dtype == np.uint64 and off.dtype == np.uint32
    slot, point, flat = sr.pairs_of(mask, off, pix, w)
    counts = np.bincount(slot, minlength=3)
    assert counts[0] == 0 and counts[1] == n and 0.2 * n < counts[2] < 0.3 * n and pix.size == counts.sum()
    assert np.array_equal(point[slot == 1], np.arange(n)) and point.max() < n
    assert np.array_equal(off.reshape(-1)[::vr.stride_words(n)], np.cumsum(counts) - counts)
    u, v = pix & 0xffff, pix >> 16
    assert u.max() == w - 1 and v.max() == h - 1 and np.array_equal(v.astype(np.int64) * w + u, flat)
    hist = np.bincount(flat, minlength=h * w)
    hot = np.argsort(hist)[-5:]
    assert {0, h * w - 1, w - 1, w} <= set(hot.tolist())
    assert 0.4 * pix.size < hist[hot].sum() < 0.6 * pix.size and (hist > 0).sum() > 0.9 * h * w        # the rest is spread out
    empty = vs.synthetic_table(100, [0.0, 0.0], h, w, np.random.default_rng(0))
    assert not empty[0].any() and not empty[1].any() and empty[2].size == 0


@pytest.mark.parametrize("m", [1, 3, 6, 17, 64])
def test_mask_view_holds_every_kind(m):
    h, w = 37, 41
    hw = h * w
    view = vs.mask_view(m, h, w, np.random.default_rng(m))
    rs, re, offs = vs.runs_of(view)
    n_runs = np.diff(offs)
    assert view.shape == (m, hw) and offs[-1] == rs.size == re.size
    for g in range(m):                                    # sorted, disjoint, non-empty, maximal
        a, b = rs[offs[g]:offs[g + 1]].astype(np.int64), re[offs[g]:offs[g + 1]].astype(np.int64)
        assert (a < b).all() and (b[:-1] < a[1:]).all() and (a >= 0).all() and (b <= hw).all()
        assert int((b - a).sum()) == int(view[g].sum())
    assert n_runs[0] > max(256, 2 * h)                    # noise: several runs per image row, more than 256 in all
    if m >= 3:
        assert n_runs[1] == 0 and n_runs[0] > 0 and np.array_equal(view[2], view[0])
    if m >= 6:
        a, b = rs[offs[3]], re[offs[3]]
        assert b - a > 3 * w and (b - 1) // w - a // w >= 3 and 65 <= n_runs[3] <= 255          # the long run; few runs
        box = view[4].reshape(h, w)
        rr, cc = np.flatnonzero(box.any(axis=1)), np.flatnonzero(box.any(axis=0))
        assert box[rr[0]:rr[-1] + 1, cc[0]:cc[-1] + 1].all() and box.sum() == rr.size * cc.size < hw
        assert list(zip(rs[offs[5]:offs[6]], re[offs[5]:offs[6]])) == [(0, 1), (hw - 1, hw)]
    if m >= 13:
        assert not np.array_equal(view[6], view[0])       # fresh noise the second time round


@pytest.mark.parametrize("name", list(vs.CASES))
def test_case_is_in_its_regime(name):
    case = vs.get(name)
    vs.assert_regime(case)
    mask, off, pix = case.table
    assert mask.shape == off.shape == (case.n_slots, vr.stride_words(case.n)) and pix.size == case.pairs > 0
    for wb, covers in case.covers.items():
        rows, cmask, masked, viewed = case.expected(wb)
        rowbase, nmask = case.layout(wb)
        assert rows.shape == (int(nmask.sum()), case.nw) and cmask.shape == (rows.shape[0], case.mw)
        assert max(c.shape[0] for c in covers) <= wb and rows.any() and masked.any() and viewed.any()
        assert int(masked.sum()) == int(np.unpackbits(rows.view(np.uint8)).sum())          # every row bit is one vote
        # rows of a mask without runs are empty, identical masks give identical rows
        for f in np.flatnonzero(case.frame_mask >= 0):
            if nmask[f] >= 3:
                assert not rows[rowbase[f] + 1].any() and np.array_equal(rows[rowbase[f]], rows[rowbase[f] + 2])
    spix, spt, rowstart = case.companion()
    assert spix.size == spt.size == case.pairs and rowstart.shape == (case.n_slots, case.h + 1)
    assert rowstart[-1, -1] == case.pairs and (np.diff(rowstart.reshape(-1).astype(np.int64)) >= 0).all()


def test_frames_without_bit_zero_do_not_count_as_viewed():
    case = vs.get("odd")
    _rows, _cmask, _masked, viewed = case.expected(64)
    exp = np.zeros(case.n, np.int64)
    for f, s in enumerate(case.depth_index):
        if case.frame_flags[f] & 1:
            exp += vs.slot_pairs(*case.table, int(s), case.n, case.w)[0]
    assert np.array_equal(viewed, exp) and viewed.max() >= 2
    assert (case.frame_flags & 1 == 0).any()
