"""bff_merge_components path by path, and bff_row_stats, against the NumPy reference of tests/merge_ref.py.

Every path of the tile pass (merge.hip: tile_masks_kernel -> tile_pair_filter_kernel -> tile_pair_rows_kernel ->
merge_components_kernel / merge_tile_pair) is reached at a size that takes seconds: the pair-list and the dense 4x4
accumulation, split mode (several blocks per tile pair that meet in a scratch slot), the "out of slots" fallback, the
chunk-level bound, a sampled order and a continued forest.  The inputs put many pairs within a few points of the
threshold, so one miscounted word, stage or part changes the components; each input asserts that on the reference
before the GPU is asked.  Bar: comp == merge_ref.components(...), no tolerance, for the production kernel and for the
counting one (a zeroed `diag` buffer selects merge_components_kernel<1>), whose counters prove which path ran.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import merge_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Restated from merge.hip (kSplitStages, kKW, kCW, kMaxSlots, kSparse); used only for preconditions on the inputs.
PART_CHUNKS = 12 * (32 // 8)        # kSplitStages * (kKW / kCW): chunks per part of a split tile pair
SPLIT_MIN = 2 * PART_CHUNKS         # tile pairs that share >= 96 chunks are split
MAX_SLOTS = 512                     # kMaxSlots: tile pairs that can be split in one call
DENSE_MIN = 7 * 256                 # more candidate pairs than kSparse * 256 take the dense 4x4 path
THR = 0.2


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def pack_np(dense):
    n = dense.shape[1]
    nw = (n + 63) // 64
    pad = np.zeros((dense.shape[0], nw * 64), bool)
    pad[:, :n] = dense
    return np.packbits(pad, axis=-1, bitorder="little").view(np.int64).copy()


# ---- inputs ---------------------------------------------------------------------------------------------------------

class Case:
    """One input: dense rows, labels, the reference Gram / edges / components (computed once, never changed)."""

    def __init__(self, d, labels, near_rows=None, cols=None, thr=THR):
        self.d, self.labels, self.thr = d, np.asarray(labels, np.int32), thr
        self.r, self.n = d.shape
        self.nw = (self.n + 63) // 64
        self.inter = mr.gram(d if cols is None else d[:, cols])        # columns outside `cols` are empty
        self.area = np.diag(self.inter).copy()
        assert cols is None or np.array_equal(self.area, d.sum(axis=1))
        self.comp, self.edges = mr.check_near_threshold(self.inter, self.labels, thr, near_rows)
        self.occ = mr.chunk_counts(d, self.nw) > 0                     # (R, n_chunks) chunk occupancy
        self._dev = None

    def device(self, lib):
        """rows + row statistics on the device (once per case); area and chunk masks checked on the way."""
        if self._dev is None:
            rows = torch.from_numpy(pack_np(self.d)).to(DEV)
            lid = torch.from_numpy(self.labels).to(DEV)
            area, mean_word, cmask, hist, sig = lib.row_stats(rows)
            assert np.array_equal(area.cpu().numpy(), self.area)
            self._dev = dict(rows=rows, lid=lid, area=area, cmask=cmask, hist=hist, sig=sig)
        return self._dev

    def orders(self, lib, seed=0):
        """label-then-signature (production) and a random permutation, so that edges cross tiles."""
        dv = self.device(lib)
        prod = torch.argsort((dv["lid"].long() << 32) | dv["sig"], stable=True).to(torch.int32)
        perm = np.random.default_rng(seed).permutation(self.r).astype(np.int32)
        return [("label-signature", prod), ("random", torch.from_numpy(perm).to(DEV))]

    def shared_chunks(self, order):
        """(n_tiles, n_tiles) number of chunks the tiles of `order` share, in NumPy."""
        o = np.asarray(order)
        tiles = [self.occ[o[t:t + 64]].any(axis=0) for t in range(0, len(o), 64)]
        return np.array([[int((a & b).sum()) for b in tiles] for a in tiles])


def exact_threshold_rows(n, lo, k=100):
    """Four rows inside points [lo, lo + 10 k): big (5 k points) and small (every 5th of them, k points): IoU = k / 5k,
    whose float32 quotient IS f32(0.2) -> no edge; big2 / small2 the same with one more common point -> an edge."""
    rows = np.zeros((4, n), bool)
    rows[0, lo:lo + 5 * k] = True
    rows[1, lo:lo + 5 * k:5] = True
    lo2 = lo + 5 * k
    rows[2, lo2:lo2 + 5 * k] = True
    rows[3, lo2:lo2 + 5 * k:5] = True
    rows[3, lo2 + 1] = True
    return rows


def case_pair_list(r, seed):
    """(a): ~20 near-threshold rows per tile, four exact-threshold rows, three empty rows, the rest on disjoint
    supports; two labels."""
    rng = np.random.default_rng(seed)
    n = 40_000 + 77
    n_near = 21 * ((r + 63) // 64)
    near = np.sort(rng.choice(r, n_near, replace=False))
    d = np.zeros((r, n), bool)
    d[near] = mr.chained_rows(rng, n_near, n)
    labels = np.zeros(r, np.int64)
    labels[near] = (np.arange(n_near) // 7) % 2                       # a chain of 7 keeps one label
    rest = np.setdiff1d(np.arange(r), near)
    exact, empty, plain = rest[:4], rest[4:7], rest[7:]
    d[exact] = exact_threshold_rows(n, 1000)
    labels[exact] = 1
    width = (n - 3000) // max(len(plain), 1)
    for k, i in enumerate(plain):                                     # disjoint supports, behind the exact rows
        lo = 3000 + k * width
        d[i, lo:lo + width] = rng.random(width) < 0.6
        labels[i] = k % 2
    c = Case(d, labels, near_rows=near)
    assert (c.area[empty] == 0).all() and (c.comp[empty] == empty).all()
    iou = mr.iou_f32(c.inter, c.area)
    assert iou[exact[0], exact[1]] == np.float32(THR) and not c.edges[exact[0], exact[1]]
    assert c.edges[exact[2], exact[3]] and c.inter[exact[2], exact[3]] == c.inter[exact[0], exact[1]] + 1
    return c


def case_bernoulli(r, n, seed, labels=None):
    """(b), (c i): every row Bernoulli over the whole cloud, chained by sevens; one label."""
    rng = np.random.default_rng(seed)
    return Case(mr.chained_rows(rng, r, n), np.zeros(r, np.int64) if labels is None else labels)


def case_thin_fillers(r, n, seed):
    """(c ii): every fourth row is a near-threshold row; the others are thin rows with 1, 6 or 31 points in every chunk
    (in turn), in couples of near-duplicates (an edge per couple).  One label, no heavy bin anywhere: the production
    order is the row order, and every tile holds ~16 rows of each kind.  Rows of different kinds differ in area by more
    than 5x, so the bin bound rejects those pairs and every tile pair keeps ~4 * 16 * 16 candidates: the pair list."""
    rng = np.random.default_rng(seed)
    near = np.arange(0, r, 4)
    d = np.zeros((r, n), bool)
    d[near] = mr.chained_rows(rng, near.size, n)
    n_chunks = -(-n // 512)
    for kind, per_chunk in ((1, 1), (2, 6), (3, 31)):
        thin = np.arange(kind, r, 4)
        for k, i in enumerate(thin):
            if k % 2 == 0:
                for c in range(n_chunks):
                    hi = min(512, n - c * 512)
                    d[i, c * 512 + rng.choice(hi, min(per_chunk, hi), replace=False)] = True
            else:                                                      # its partner: the same but for a few chunks
                d[i] = d[thin[k - 1]]
                d[i, :512 * 9] = False
    c = Case(d, np.zeros(r, np.int64), near_rows=near)
    assert c.edges[1, 5] and c.edges[2, 6] and c.edges[3, 7] and c.occ[1].all()
    c.hist_pass = mr.bound_passes(mr.hist_bound(d, c.nw), c.area, c.labels, THR)
    return c


def case_slots_exhausted(seed):
    """(d): 2112 rows = 33 tiles = 561 tile pairs, every row in every chunk; points only in the first two words of every
    chunk (the chunk counts, and with them the split decisions, are those of fully populated rows)."""
    rng = np.random.default_rng(seed)
    r, n = 2112, 49_152 + 77
    pts = np.arange(n)
    cols = pts[(pts // 64) % 8 < 2]
    # 12 416 populated points: independent pairs sit at IoU p / (2 - p) = 0.163, 6 sigma below the threshold (2.2 M
    # pairs), chained neighbours at 0.205 +- 0.006
    d = mr.chained_rows(rng, r, n, p=0.28, f=0.084, cols=cols)
    return Case(d, np.zeros(r, np.int64), cols=cols)


def nested_family(rng, cols, n):
    """Eight rows over the points `cols`: X (90 % of them, a multiple of 5) and seven subsets of X holding 1/5 of it
    (IoU exactly f32(0.2): no edge), one point more (edge), four more sizes up to 4.5 % above the threshold (edges)
    and one at ~0.19 (no edge).  Nested inside every chunk: the chunk bound equals the intersection."""
    x = rng.permutation(cols)[:max(5, int(0.9 * cols.size) // 5 * 5)]
    rows = np.zeros((8, n), bool)
    rows[0, x] = True
    k = x.size // 5
    sizes = [k, k + 1] + [k + max(2 + j, int(x.size * t)) for j, t in enumerate((0.002, 0.004, 0.006))] + \
            [k + max(6, int(x.size * 0.009)), k - max(2, int(x.size * 0.01))]
    for j, s in enumerate(sizes):
        rows[1 + j, rng.permutation(x)[:s]] = True
    return rows


def case_chunk_bound(r, s, seed):
    """(e): every row lives in the same `s` of the cloud's 265 chunks (the last, partly filled one among them), so every
    tile pair shares exactly s chunks whatever the order.  Nested families (a label each) + couples that the bin bound
    passes and the chunk bound rejects (alternating chunks), couples that pass both and fail the exact test
    (interleaved points), two empty rows and independent rows."""
    rng = np.random.default_rng(seed)
    n = 131_072 + 4_096 + 77
    n_chunks = -(-n // 512)
    chosen = np.sort(np.concatenate([rng.choice(n_chunks - 1, s - 1, replace=False), [n_chunks - 1]])) if s > 1 else \
        rng.choice(n_chunks - 1, 1)                                    # (a full chunk when there is only one)
    pts = np.arange(n)
    cols = pts[np.isin(pts // 512, chosen)]
    n_fam = 6 * (r // 64)
    d = np.zeros((r, n), bool)
    labels = np.zeros(r, np.int64)
    for g in range(n_fam):
        d[8 * g:8 * g + 8] = nested_family(rng, cols, n)
        labels[8 * g:8 * g + 8] = g
    fam_rows = np.arange(8 * n_fam)
    kind = {"alternating": [], "interleaved": []}
    i = 8 * n_fam
    for q in range(r // 64):
        for _ in range(2):
            if s > 1:                                                  # same bins, alternating chunks
                par = np.searchsorted(chosen, cols // 512) % 2
                d[i, cols[par == 0]] = True
                d[i + 1, cols[par == 1]] = True
                kind["alternating"].append((i, i + 1))
            else:                                                      # one chunk cannot alternate: quarters of it
                d[i, cols[(np.arange(cols.size) // 2) % 2 == 0]] = True
                d[i + 1, cols[(np.arange(cols.size) // 2) % 2 == 1]] = True
                kind["interleaved"].append((i, i + 1))
            labels[i:i + 2] = 1000 + i
            i += 2
        for _ in range(2):                                             # same chunks, interleaved points
            d[i, cols[0::2]] = True
            d[i + 1, cols[1::2]] = True
            kind["interleaved"].append((i, i + 1))
            labels[i:i + 2] = 1000 + i
            i += 2
        i += 2                                                         # two empty rows
        while i < 64 * (q + 1):
            d[i, cols] = rng.random(cols.size) < 0.31
            labels[i] = 2000
            i += 1
    c = Case(d, labels, near_rows=fam_rows, cols=cols)
    c.s, c.kind = s, kind
    chunk_ub = mr.chunk_bound(d, c.nw)
    hb = mr.bound_passes(mr.hist_bound(d, c.nw), c.area, labels, THR)
    cb = hb & mr.bound_passes(chunk_ub, c.area, labels, THR)          # the chunk bound sees what the bin bound passed
    assert not (c.edges & ~cb).any()                                  # both bounds are sound
    for a, b in kind["alternating"]:
        assert hb[a, b] and not cb[a, b]
    for a, b in kind["interleaved"]:
        assert hb[a, b] and cb[a, b] and not c.edges[a, b] and c.inter[a, b] == 0
    c.n_chunk_rejected = int(np.triu(hb & ~cb, 1).sum())
    c.n_exact_rejected = int(np.triu(cb & ~c.edges, 1).sum())
    iou = mr.iou_f32(c.inter, c.area)
    tight = np.triu(c.edges & (chunk_ub == c.inter) & (iou < np.float32(THR) * np.float32(1.05)), 1)
    c.n_tight = int(tight.sum())
    assert c.n_tight >= 4 * n_fam and c.n_exact_rejected >= len(kind["interleaved"])
    assert c.n_chunk_rejected >= len(kind["alternating"])
    # one shared chunk lies inside one or two bins: the chunk bound is no tighter than the bin bound there
    assert c.n_chunk_rejected > 0 if s > 1 else c.n_chunk_rejected == 0
    for g in range(n_fam):                                             # exact threshold: no edge; one point more: edge
        assert iou[8 * g, 8 * g + 1] == np.float32(THR) and not c.edges[8 * g, 8 * g + 1] and c.edges[8 * g, 8 * g + 2]
    return c


_cases = {}


def get_case(name, *args):
    key = (name,) + args
    if key not in _cases:
        _cases[key] = globals()["case_" + name](*args)
    return _cases[key]


# ---- running the kernel -----------------------------------------------------------------------------------------------

def run_merge(lib, c, order, diag=False, chunk_pop=None, parent=None, init_parent=1, n_order=None, scratch=None):
    """bff_merge_components called directly -> (comp, diag counters or None)."""
    dv = c.device(lib)
    i32, i64 = torch.int32, torch.int64
    tmask = torch.empty(((c.r + 63) // 64, dv["cmask"].shape[1]), dtype=i64, device=DEV)
    if scratch is None:
        scratch = torch.empty(int(lib.load().bff_merge_scratch_words(c.r)), dtype=i32, device=DEV)
    parent = torch.empty(c.r, dtype=i32, device=DEV) if parent is None else parent
    comp = torch.full((c.r,), -7, dtype=i32, device=DEV)
    dg = torch.zeros(16, dtype=i32, device=DEV) if diag else None
    p = lib._ptr
    lib.call("bff_merge_components", p(dv["rows"], i64), c.r, c.nw, p(order, i32),
             order.shape[0] if n_order is None else n_order, p(dv["cmask"], i64), p(tmask), p(dv["hist"], i32),
             p(scratch), p(dv["area"], i32), p(dv["lid"], i32), float(c.thr), p(parent), int(init_parent), p(comp),
             p(dg, i32), p(chunk_pop, torch.int16))
    torch.cuda.synchronize()
    return comp.cpu().numpy(), (dg.cpu().numpy() if diag else None)


def check_paths(lib, c, expect, chunk_pop=None, record=None):
    """Production kernel and counting kernel against the reference for every order; `expect(diag, shared, order)` asserts
    the path.  -> list of diag arrays."""
    out = []
    for name, order in c.orders(lib):
        shared = c.shared_chunks(order.cpu().numpy())
        comp, _ = run_merge(lib, c, order, chunk_pop=chunk_pop)
        assert np.array_equal(comp, c.comp), name
        comp, dg = run_merge(lib, c, order, diag=True, chunk_pop=chunk_pop)
        assert np.array_equal(comp, c.comp), name
        print(f"{record or ''} R={c.r} N={c.n} order={name}: diag[0]={dg[0]} [1]={dg[1]} [2]={dg[2]} [3]={dg[3]} "
              f"[9]={dg[9]} [10]={dg[10]} shared={shared.min()}..{shared.max()}")
        expect(dg, shared, order.cpu().numpy())
        out.append(dg)
    return out


def n_tile_pairs(r):
    t = (r + 63) // 64
    return t * (t + 1) // 2


# ---- (a) - (e) --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [64, 130])
def test_pair_list_path(lib, r):
    c = get_case("pair_list", r, 11)

    def expect(dg, shared, order):
        assert shared.max() < SPLIT_MIN and not lib.load().bff_merge_uses_chunk_bound(c.nw)
        assert dg[9] > 0 and dg[10] == 0
    check_paths(lib, c, expect, record="(a) pair list")


@pytest.mark.parametrize("r", [64, 128, 192])
def test_dense_path(lib, r):
    c = get_case("bernoulli", r, 40_000 + 77, 12)
    if r == 64:                       # one tile pair that starts from singletons: its candidates are the bound's pairs
        hb = mr.bound_passes(mr.hist_bound(c.d, c.nw), c.area, c.labels, THR)
        assert np.triu(hb, 1).sum() > DENSE_MIN

    def expect(dg, shared, order):
        assert shared.max() < SPLIT_MIN
        assert dg[10] > 0
    check_paths(lib, c, expect, record="(b) dense")


@pytest.mark.parametrize("variant", ["bernoulli", "thin_fillers"])
@pytest.mark.parametrize("r,n", [(64, 65_536 + 77), (128, 65_536 + 77), (200, 65_536 + 77), (128, 49_152 + 77)])
def test_split_mode(lib, r, n, variant):
    c = get_case(variant, r, n, 13)
    assert not lib.load().bff_merge_uses_chunk_bound(c.nw)
    if n == 49_152 + 77:              # two parts over an odd number of stages: parts of unequal length
        assert -(-c.occ.shape[1] // 4) % 2 == 1 and c.occ.shape[1] // PART_CHUNKS == 2

    def expect(dg, shared, order):
        assert shared.min() >= SPLIT_MIN                            # every tile pair is split
        assert dg[0] > n_tile_pairs(c.r)                            # parts ran
        if variant == "bernoulli":
            assert dg[10] > 0
        else:
            # every tile pair keeps some pairs after the bin bound, and few enough for the pair list (split mode takes
            # its candidates from the bounds alone)
            for ta in range(0, c.r, 64):
                for tb in range(ta, c.r, 64):
                    cnt = c.hist_pass[np.ix_(order[ta:ta + 64], order[tb:tb + 64])].sum() // (2 if ta == tb else 1)
                    assert 0 < cnt <= DENSE_MIN, (ta, tb, cnt)
            assert dg[9] > 0 and dg[10] == 0
    check_paths(lib, c, expect, record=f"(c) split, {variant}")


def test_split_slots_exhausted(lib):
    c = get_case("slots_exhausted", 14)
    assert n_tile_pairs(c.r) == 561 > MAX_SLOTS

    def expect(dg, shared, order):
        assert shared.min() >= SPLIT_MIN
        assert dg[0] > 561
    check_paths(lib, c, expect, record="(d) slots exhausted")


@pytest.mark.parametrize("s", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("r", [64, 128])
def test_chunk_bound(lib, r, s):
    c = get_case("chunk_bound", r, s, 15 + s)
    assert lib.load().bff_merge_uses_chunk_bound(c.nw) and c.occ.shape[1] == 265
    dv = c.device(lib)
    ref = mr.row_stats_ref(c.d, c.nw)
    dense_pop = dv["hist"].chunk_pop
    given = lib.row_stats(dv["rows"], dv["cmask"].clone())[3].chunk_pop
    for pop in (dense_pop, given):
        assert np.array_equal(pop.cpu().numpy().view(np.uint16), ref["chunk_pop"])

    def expect(dg, shared, order):
        assert (shared == s).all()
        assert dg[0] > 0
    off = check_paths(lib, c, expect, chunk_pop=None, record=f"(e) chunk bound off, s={s}")
    on = check_paths(lib, c, expect, chunk_pop=dense_pop, record=f"(e) chunk bound on, s={s}")
    check_paths(lib, c, expect, chunk_pop=given, record=f"(e) chunk bound on (given mask), s={s}")
    # candidates are fixed by the bounds alone where the forest cannot interfere: in split mode, and in a single tile
    # pair that starts from singletons.  Elsewhere (128 rows sharing fewer than SPLIT_MIN chunks) a block drops the
    # pairs its forest has joined already, so the two counts are not comparable and only comp is checked.
    if s >= SPLIT_MIN or r == 64:
        for a, b in zip(on, off):
            if s > 1:
                assert c.n_chunk_rejected > 0 and a[2] < b[2]
            else:                                                      # the chunk bound has nothing to reject (see the
                assert c.n_chunk_rejected == 0 and a[2] <= b[2]        # case): it may not add candidates either


# ---- (f) sampled order, continued forest -----------------------------------------------------------------------------

def f_cases():
    return [get_case("bernoulli", 128, 65_536 + 77, 13), get_case("pair_list", 130, 11),
            get_case("bernoulli", 512, 40_000 + 77, 12)]


# the wrapper samples only from 64 * stride rows on: with 128 and 130 rows stride 8 is the plain call (kept: the same
# arguments must give the same answer), stride 2 takes the coarse route; with 512 rows both strides take it
@pytest.mark.parametrize("which,stride", [(0, 8), (1, 8), (0, 2), (1, 2), (2, 8), (2, 2)])
def test_coarse_stride_through_lib(lib, which, stride):
    """_lib.merge_components with a coarse pass first: a sampled order, then the full order from that forest."""
    c = f_cases()[which]
    assert (c.r >= 64 * stride) == ((which, stride) != (0, 8) and (which, stride) != (1, 8))
    dv = c.device(lib)
    for name, order in c.orders(lib):
        comp = lib.merge_components(dv["rows"], dv["area"], dv["lid"], c.thr, order, dv["cmask"], dv["hist"],
                                    coarse_stride=stride)
        assert np.array_equal(comp.cpu().numpy(), c.comp), name


@pytest.mark.parametrize("which", [0, 1])
def test_sampled_order(lib, which):
    c = f_cases()[which]
    rng = np.random.default_rng(21)
    for diag in (False, True):
        sub = rng.permutation(c.r)[:c.r // 2].astype(np.int32)
        keep = np.zeros(c.r, bool)
        keep[sub] = True
        exp = mr.components(c.edges & keep[:, None] & keep[None, :])
        assert (exp[~keep] == np.flatnonzero(~keep)).all() and (exp != np.arange(c.r)).any()
        comp, _ = run_merge(lib, c, torch.from_numpy(sub).to(DEV), diag=diag)
        assert np.array_equal(comp, exp)
        # the same sample as the head of a longer order buffer
        full = np.concatenate([sub, np.setdiff1d(np.arange(c.r), sub)]).astype(np.int32)
        comp, _ = run_merge(lib, c, torch.from_numpy(full).to(DEV), diag=diag, n_order=c.r // 2)
        assert np.array_equal(comp, exp)


@pytest.mark.parametrize("which", [0, 1])
def test_continued_forest(lib, which):
    c = f_cases()[which]
    rng = np.random.default_rng(22)
    # links to the smaller index between rows of different components (not adjacent), chains among them
    parent = np.arange(c.r, dtype=np.int32)
    links = []
    for b in rng.permutation(np.arange(1, c.r))[:c.r // 6]:
        a = int(rng.integers(0, b))
        if c.comp[a] != c.comp[b]:
            parent[b] = a
            links.append((a, int(b)))
    assert len(links) >= 4 and (parent <= np.arange(c.r)).all()
    exp = mr.components(c.edges, links=links)
    assert not np.array_equal(exp, c.comp) and np.unique(exp).size > 1
    for name, order in c.orders(lib):
        for diag in (False, True):
            comp, _ = run_merge(lib, c, order, diag=diag, parent=torch.from_numpy(parent).to(DEV), init_parent=0)
            assert np.array_equal(comp, exp), name


# ---- (g) BFF_MERGE_SPLIT=0 ---------------------------------------------------------------------------------------------

_CHILD = """
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_merge_paths as t
from beyond_fixed_forms_amd import _lib
_lib.load()
c = t.get_case("bernoulli", 128, 65_536 + 77, 13)
out = {{}}
for name, order in c.orders(_lib):
    comp, dg = t.run_merge(_lib, c, order, diag=True)
    out[name] = dict(comp=comp.tolist(), diag=dg.tolist(), prod=t.run_merge(_lib, c, order)[0].tolist())
print("RESULT " + json.dumps(out))
"""


def test_split_switched_off_in_a_fresh_process(lib):
    """BFF_MERGE_SPLIT is read once per process: a child runs case (c)-128 with it set to 0."""
    c = get_case("bernoulli", 128, 65_536 + 77, 13)
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BFF_MERGE_SPLIT="0")
    res = subprocess.run([sys.executable, "-c", _CHILD.format(root=os.path.dirname(tests), tests=tests)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert set(out) == {"label-signature", "random"}
    for name, got in out.items():
        assert np.array_equal(np.array(got["comp"]), c.comp), name
        assert np.array_equal(np.array(got["prod"]), c.comp), name
        assert 0 < got["diag"][0] <= n_tile_pairs(c.r)              # one block per tile pair: nothing was split
        print(f"(g) split off order={name}: diag[0]={got['diag'][0]} [2]={got['diag'][2]} [9]={got['diag'][9]} "
              f"[10]={got['diag'][10]}")


# ---- scratch layout: nothing is written behind bff_merge_scratch_words ------------------------------------------------

GUARD_WORDS, GUARD = 256, 0x5A5A5A5A


@pytest.mark.parametrize("which", ["split", "pair_list"])
def test_scratch_guard_words_untouched(lib, which):
    """The scratch buffer is exactly bff_merge_scratch_words(n_rows) words, followed by guard words: the call leaves the
    guard alone and finds the reference's components.  Split mode is the one path that writes the regions at the end of
    the layout (arrival counters, partial counts); the pair-list input is the plain path."""
    c = get_case("bernoulli", 128, 65_536 + 77, 13) if which == "split" else get_case("pair_list", 130, 11)
    words = int(lib.load().bff_merge_scratch_words(c.r))
    for name, order in c.orders(lib):
        for diag in (False, True):
            buf = torch.full((words + GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
            comp, dg = run_merge(lib, c, order, diag=diag, scratch=buf[:words])
            assert np.array_equal(comp, c.comp), name
            assert (buf[words:] == GUARD).all().item(), name
            if diag and which == "split":
                assert dg[0] > n_tile_pairs(c.r), name                  # parts ran: the end regions were in use


# ---- (h) bff_row_stats -------------------------------------------------------------------------------------------------

def spread(d, i, lo_bin, counts, bin_pts, n):
    """counts[k] points into bin lo_bin + k of row i (clipped to what the bin holds)."""
    for k, cnt in enumerate(counts):
        lo = (lo_bin + k) * bin_pts
        hi = min(lo + bin_pts, n)
        if hi > lo and cnt > 0:
            d[i, lo:lo + min(cnt, hi - lo)] = True


def stats_rows(nw, seed, full=True):
    rng = np.random.default_rng(seed)
    n = nw * 64 - 13                                   # the last word is partly valid
    bin_pts = -(-nw // 64) * 64
    n_bins = -(-n // bin_pts)
    d = np.zeros((9 if full else 3, n), bool)
    d[1, 0] = True
    d[2, n - 1] = True
    if not full:
        return d, n
    d[3] = True
    d[4] = rng.random(n) < 0.3
    others = max(n_bins - 1, 1)
    # 15 of 100 points in bin 0 (heavy: 15 * 100 >= 100 * 15), the rest spread over the other bins; then 14 of 100
    for row, k in ((5, 15), (6, 14)):
        rest = [(100 - k) // others + (1 if q < (100 - k) % others else 0) for q in range(others)]
        spread(d, row, 0, [k] + rest, bin_pts, n)
    spread(d, 7, max(n_bins - 6, 0), [16] * min(6, n_bins), bin_pts, n)        # six heavy bins: five enter the key
    d[8, max((n_bins - 1) * bin_pts, (n - 1) // 512 * 512):] = True            # last, partly filled bin and chunk
    return d, n


def check_row_stats(lib, d, nw):
    ref = mr.row_stats_ref(d, nw)
    rows = torch.from_numpy(pack_np(d)).to(DEV)
    assert rows.shape[1] == nw
    r, mw = d.shape[0], ref["chunk_mask"].shape[1]
    i32, i64 = torch.int32, torch.int64
    p = lib._ptr
    for given in (0, 1):
        area = torch.full((r,), -1, dtype=i32, device=DEV)
        mean_word = torch.full((r,), -1, dtype=i32, device=DEV)
        hist = torch.full((r, 64), -1, dtype=i32, device=DEV)
        sig = torch.full((r,), -1, dtype=i64, device=DEV)
        cpop = torch.full((r, 64 * mw), -1, dtype=torch.int16, device=DEV)       # 0xFFFF everywhere
        cmask = torch.from_numpy(ref["chunk_mask"].view(np.int64)).to(DEV) if given else \
            torch.full((r, mw), -1, dtype=i64, device=DEV)
        lib.call("bff_row_stats", p(rows, i64), r, nw, p(area), p(mean_word), p(cmask, i64), given, p(hist), p(sig),
                 p(cpop))
        torch.cuda.synchronize()
        what = f"nw={nw} mask {'given' if given else 'computed'}"
        assert np.array_equal(area.cpu().numpy(), ref["area"]), what
        assert np.array_equal(mean_word.cpu().numpy(), ref["mean_word"]), what
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), ref["hist"]), what
        assert np.array_equal(cmask.cpu().numpy().view(np.uint64), ref["chunk_mask"]), what
        assert np.array_equal(sig.cpu().numpy(), ref["signature"]), what
        assert np.array_equal(cpop.cpu().numpy().view(np.uint16), ref["chunk_pop"]), what
    return ref


@pytest.mark.parametrize("nw", [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2048, 4097])
def test_row_stats_against_numpy(lib, nw):
    d, n = stats_rows(nw, 30 + nw)
    ref = check_row_stats(lib, d, nw)
    assert ref["area"][0] == 0 and ref["signature"][0] == 0x3FFFFFFF and ref["mean_word"][0] == 0x7fffffff
    assert ref["mean_word"][1] == 0 and ref["mean_word"][2] == nw - 1 and ref["area"][3] == n
    if nw >= 8:                                        # eight bins or more hold the constructed rows: check the intent
        assert ref["area"][5] == 100 and ref["hist"][5, 0] == 15 and ref["signature"][5] == (0 << 24) | 0xFFFFFF
        assert ref["area"][6] == 100 and ref["hist"][6, 0] == 14 and ref["signature"][6] == 0x3FFFFFFF
        heavy = np.flatnonzero(ref["hist"][7] * 100 >= ref["area"][7] * 15)
        assert heavy.size == 6 and ref["signature"][7] & 63 == heavy[4]
    assert ref["chunk_mask"][8, -1] != 0 and np.count_nonzero(ref["chunk_pop"][8]) == 1


def test_row_stats_at_the_chunk_limit(lib):
    nw = 32_768                                        # 4096 chunks: mw = 64, the most a call accepts
    d, n = stats_rows(nw, 31, full=False)
    d[0, ::3] = True
    ref = check_row_stats(lib, d, nw)
    assert ref["chunk_mask"].shape[1] == 64 and ref["chunk_pop"][2, -1] == 1
