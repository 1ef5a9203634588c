"""The NumPy statement of the visibility table's pixel-sorted companion (tests/visibility_sorted_ref.py) against a literal
per-slot np.lexsort on the small case of tests/visibility_ref.py: 1500 points, 6 slots of 24 x 32 pixels, two of which see
nothing.  Host only."""
import numpy as np
import pytest

import visibility_ref as vr
import visibility_sorted_ref as sr


@pytest.fixture(scope="module")
def small():
    case = vr.build_case()
    tab = vr.table(case["xyz"], case["poses"], vr.K, case["depth"], vr.THRESH)
    return dict(case=case, tab=tab, got=sr.companion(*tab, vr.H, vr.W))


def test_statement_equals_a_per_slot_lexsort(small):
    mask, off, pix = small["tab"]
    spix, spt, rowstart = small["got"]
    slot, point, flat = sr.pairs_of(mask, off, pix, vr.W)
    assert spix.dtype == spt.dtype == rowstart.dtype == np.uint32
    assert spix.shape == spt.shape == pix.shape and rowstart.shape == (vr.N_SLOTS, vr.H + 1)
    at = 0
    for s in range(vr.N_SLOTS):
        px, pt = flat[slot == s], point[slot == s]
        order = np.lexsort((pt, px))                     # last key first: by pixel, ties by point
        assert np.array_equal(spix[at:at + px.size], px[order]), f"slot {s}: pixels"
        assert np.array_equal(spt[at:at + px.size], pt[order]), f"slot {s}: points"
        exp = at + np.array([(px < y * vr.W).sum() for y in range(vr.H + 1)])
        assert np.array_equal(rowstart[s], exp), f"slot {s}: row starts"
        assert rowstart[s, vr.H] == at + px.size
        at += px.size
    assert at == pix.size


def test_case_holds_pixels_with_several_points(small):
    """The tie order (ascending point inside one pixel) is exercised."""
    spix, spt, rowstart = small["got"]
    ties = 0
    for s in range(vr.N_SLOTS):
        a, b = int(rowstart[s, 0]), int(rowstart[s, vr.H])
        same = spix[a + 1:b] == spix[a:b - 1] if b - a > 1 else np.zeros(0, bool)
        ties += int(same.sum())
        assert (spt[a + 1:b][same] > spt[a:b - 1][same]).all()
    assert ties >= 1


def test_empty_slot_has_equal_row_starts(small):
    mask, _off, _pix = small["tab"]
    _spix, _spt, rowstart = small["got"]
    for s in (vr.SLOT_NO_DEPTH, vr.SLOT_AWAY):
        assert not mask[s].any()
        assert (rowstart[s] == rowstart[s, 0]).all()
    assert rowstart[0, 0] == 0 and rowstart[-1, vr.H] == small["tab"][2].size
