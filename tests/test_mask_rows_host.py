"""The row directory of the 2-D masks as NumPy states it (tests/mask_rows_ref.py) against a dense decode of the same run
tables: all pixels of all masks of the hand-made views the GPU tests use (no GPU needed)."""
import numpy as np
import pytest

import mask_rows_ref as mr

VIEWS = {
    "hand34": lambda: mr.hand_view(34),
    "hand30": lambda: mr.hand_view(30),
    "second": mr.second_view,
    "full64": mr.full_box_view,
    "none": lambda: np.zeros((0, mr.H * mr.W), bool),
}


@pytest.mark.parametrize("name", list(VIEWS))
def test_lookup_equals_dense_decode(name):
    dense = VIEWS[name]()
    rs, re, offs = mr.runs_of(dense)
    assert np.array_equal(mr.dense_of(rs, re, offs, mr.H * mr.W), dense)
    # the contract the look-up is defined on: sorted, disjoint, non-empty runs inside the image
    for g in range(len(offs) - 1):
        s, e = rs[offs[g]:offs[g + 1]], re[offs[g]:offs[g + 1]]
        assert (s < e).all() and (s[1:] >= e[:-1]).all() and (s.size == 0 or (s[0] >= 0 and e[-1] <= mr.H * mr.W))
    tab, directory = mr.row_directory_ref(rs, re, offs, mr.H, mr.W)
    assert np.array_equal(mr.lookup_all_ref(tab, directory, rs, re, mr.H, mr.W), dense)
    # dir_offs is the exclusive scan of the boxes' heights, closed by the total
    heights = [0 if t[0] == mr.EMPTY_BOX else (int(t[1]) >> 16) - (int(t[0]) >> 16) + 1 for t in tab[:-1]]
    assert np.array_equal(tab[:, 2], np.concatenate([[0], np.cumsum(heights)]).astype(np.uint32))
    assert int(tab[-1, 2]) == directory.size <= max(len(offs) - 1, 0) * mr.H and int(tab[-1, 3]) == rs.size


def test_hand_view_has_every_kind_of_row():
    dense = mr.hand_view(34)
    rs, re, offs = mr.runs_of(dense)
    tab, directory = mr.row_directory_ref(rs, re, offs, mr.H, mr.W)
    W, H = mr.W, mr.H

    def entry(g, r):
        return int(directory[int(tab[g, 2]) + r - (int(tab[g, 0]) >> 16)])

    assert tab[0, 0] == mr.EMPTY_BOX and tab[0, 1] == 0 and tab[0, 2] == tab[1, 2]          # no runs: no rows
    assert tuple(tab[1, :2]) == (0, 0) and entry(1, 0) == (0 | 1 << 15)                       # pixel (0, 0)
    assert tuple(tab[2, :2]) == (W - 1 | (H - 1) << 16,) * 2 and entry(2, H - 1) == (W - 1 | W << 15) and re[offs[3] - 1] == H * W
    assert entry(3, 3) == (30 | W << 15) and entry(4, 5) == (0 | 5 << 15)
    # three full rows between two partial ones; the box is full width because the run crosses row ends
    assert tuple(tab[5, :2]) == (0 | 7 << 16, W - 1 | 11 << 16)
    assert [entry(5, r) for r in range(7, 12)] == [20 | W << 15] + [0 | W << 15] * 3 + [0 | 10 << 15]
    assert entry(6, 2) == mr.ROW_FLAG | 2 << mr.COUNT_SHIFT | 0 and entry(6, 3) == (1 | 4 << 15)
    assert entry(7, 9) == mr.ROW_FLAG | 6 << mr.COUNT_SHIFT | 1 and 6 > mr.LINEAR            # past the linear scan
    assert entry(8, 12) == mr.ROW_FLAG | mr.COUNT_SAT << mr.COUNT_SHIFT | 1 and 19 > mr.COUNT_SAT
    assert np.array_equal(dense[9], dense[10]) and np.array_equal(tab[9, :2], tab[10, :2])
    # some pixel is covered by more than one mask, and some mask has a hole inside its box
    assert dense.sum(0).max() >= 4 and (directory == 0).any()
