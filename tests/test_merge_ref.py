"""The NumPy reference of the merge tile pass (tests/merge_ref.py) against the oracle, on the CPU."""
import numpy as np
import torch

import merge_ref as mr
from oracle import projection_ref as pref


def small_case(seed=3, r=37, n=2100):
    rng = np.random.default_rng(seed)
    d = np.zeros((r, n), bool)
    for i in range(r):
        c = int(rng.integers(0, 4)) * (n // 5)
        d[i, c:c + int(rng.integers(n // 50, n // 4))] = True
        d[i] &= rng.random(n) < 0.8
    d[4] = False
    d[min(20, r - 1)] = False
    labels = rng.integers(0, 2, r)
    return d, labels


def test_gram_edges_components_match_oracle():
    from beyond_fixed_forms_amd.projection import groups_from_labels
    d, labels = small_case()
    g = mr.gram(d, block=512)                                   # several blocks
    assert np.array_equal(g, d.astype(np.int64) @ d.astype(np.int64).T)
    for thr in (0.0, 0.1, 0.3):
        iou = pref.pairwise_iou(torch.from_numpy(d))
        merge = (pref.label_equality([str(x) for x in labels]) & (iou > thr)).numpy()
        e = mr.edges(g, labels, thr)
        off = ~np.eye(len(labels), dtype=bool)
        assert np.array_equal(e, merge & off)
        assert e.any() and not e[4].any() and not e[20].any()
        comp = mr.components(e)
        assert comp[4] == 4 and comp[20] == 20
        assert np.array_equal(comp[comp], comp) and (comp <= np.arange(len(comp))).all()
        assert groups_from_labels(comp, np.diag(merge)) == pref.connected_groups(torch.from_numpy(merge).float())


def test_components_with_links_and_chain():
    e = np.zeros((9, 9), bool)
    for a, b in ((8, 7), (7, 6), (6, 5), (1, 3)):
        e[a, b] = True                                          # one direction is enough
    assert mr.components(e).tolist() == [0, 1, 2, 1, 4, 5, 5, 5, 5]
    assert mr.components(e, links=[(0, 8), (2, 4)]).tolist() == [0, 1, 2, 1, 2, 0, 0, 0, 0]


def test_exact_threshold_is_no_edge():
    # nested rows: I = a_j = k, a_i = 4 k -> IoU = 0.25 exactly; I = k, union = 5 k -> the float32 quotient is f32(0.2)
    for thr, (inter, ai, aj) in ((0.25, (100, 400, 100)), (0.2, (100, 400, 200))):
        g = np.array([[ai, inter], [inter, aj]])
        assert not mr.edges(g, [0, 0], thr).any()
        g1 = np.array([[ai, inter + 1], [inter + 1, aj + 1]])  # one more common point
        assert mr.edges(g1, [0, 0], thr)[0, 1]


def test_row_stats_ref_and_bounds():
    d, labels = small_case(seed=5, r=12, n=40_000)
    n = d.shape[1]
    nw = (n + 63) // 64
    st = mr.row_stats_ref(d, nw)
    bw = -(-nw // 64)
    exp_hist = np.add.reduceat(np.pad(d, ((0, 0), (0, 64 * 64 * bw - n))), np.arange(0, 64 * 64 * bw, 64 * bw), axis=1)
    assert np.array_equal(st["hist"], exp_hist)
    assert np.array_equal(st["area"], d.sum(1))
    occ = np.add.reduceat(np.pad(d, ((0, 0), (0, (-n) % 512))), np.arange(0, n, 512), axis=1)
    mw = st["chunk_mask"].shape[1]
    assert mw == -(-occ.shape[1] // 64) and st["chunk_pop"].shape == (12, 64 * mw)
    assert np.array_equal(st["chunk_pop"][:, :occ.shape[1]], occ) and not st["chunk_pop"][:, occ.shape[1]:].any()
    bits = np.unpackbits(st["chunk_mask"].view(np.uint8), axis=1, bitorder="little")[:, :occ.shape[1]]
    assert np.array_equal(bits.astype(bool), occ > 0)
    assert st["mean_word"][4] == 0x7fffffff and st["signature"][4] == 0x3FFFFFFF
    n_heavy = 0
    for i in np.flatnonzero(st["area"]):
        words = np.flatnonzero(d[i]) // 64
        assert st["mean_word"][i] == int(words.sum()) // int(d[i].sum())
        heavy = [b for b in range(64) if exp_hist[i, b] * 100 >= d[i].sum() * 15]
        key = 0
        for s in range(5):
            key = key * 64 + (heavy[s] if s < len(heavy) else 63)
        assert st["signature"][i] == key
        n_heavy += len(heavy)
    assert n_heavy > 0
    # both are upper bounds of the intersection (bins and chunks do not nest: neither bound dominates the other)
    g = mr.gram(d)
    hb, cb = mr.hist_bound(d, nw), mr.chunk_bound(d, nw)
    assert (hb >= g).all() and (cb >= g).all() and (hb > g).any() and (cb > g).any()
    assert np.array_equal(np.diag(cb), st["area"])


def test_generator_has_near_threshold_structure():
    rng = np.random.default_rng(1)
    d = mr.chained_rows(rng, 64, 20_000)
    g = mr.gram(d)
    comp, e = mr.check_near_threshold(g, np.zeros(64, int), 0.2)
    assert np.array_equal(comp, mr.components(e))
