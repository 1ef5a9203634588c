"""GPU parity of the scene call's tail (csrc/groups.hip, resolve.hip, rows.hip), entry point by entry point: groups formed on the device
(bff_group_components), their OR and confidence means (bff_or_reduce_grouped), the arena clear
(bff_clear_flagged_chunks_unless), and the steps that read the group count on the device (bff_resolve_overlaps_dev,
bff_scatter_bits, bff_cross_popcount_dev) -- against plain NumPy / the oracle, at the sizes and counts where their
index arithmetic changes regime.  Bar: bit-exact tables, masks and counts; confidence means equal to the reference's
sequential sum in the confidence dtype."""
import os

import numpy as np
import pytest
import torch

from group_tables_ref import build_components, group_tables_ref
from oracle import projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
i32, i64 = torch.int32, torch.int64
GARBAGE = -0x21524111                                          # 0xDEADBEEF as int32


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def unpack(rows, n):
    b = rows.cpu().numpy().view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[:, :n].astype(bool)


def pack_np(dense):
    n = dense.shape[1]
    nw = (n + 63) // 64
    pad = np.zeros((dense.shape[0], nw * 64), bool)
    pad[:, :n] = dense
    return torch.from_numpy(np.packbits(pad, axis=-1, bitorder="little").view(np.int64).copy()).to(DEV)


def dev(a, dtype=i32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def or_sparse_min_nw():
    """BFF_OR_SPARSE_MIN_NW as the library reads it (atoll, default 1024)."""
    e = os.environ.get("BFF_OR_SPARSE_MIN_NW")
    if e is None:
        return 1024
    digits = e.strip().split()[0] if e.strip() else ""
    try:
        return int(digits)
    except ValueError:
        return 0


def sparse_rows(rng, r, nw, picks=3, p_empty=0.1):
    """uint64 (r, nw): a few occupied 8-word chunks per row (some rows empty)."""
    d = np.zeros((r, nw), np.uint64)
    nc = (nw + 7) // 8
    for _ in range(picks):
        w = rng.integers(0, nc, r)[:, None] * 8 + np.arange(8)
        ok = (w < nw) & (rng.random(r) >= p_empty)[:, None]
        ri = np.broadcast_to(np.arange(r)[:, None], w.shape)
        d[ri[ok], w[ok]] |= rng.integers(0, 2 ** 63, int(ok.sum()), dtype=np.uint64) * (rng.random(int(ok.sum())) < 0.7)
    return d


# ------------------------------------------------------------------ thin helpers over the C ABI
def group_components(lib, comp, parent, area, thr, mm, cap, count_is_zero):
    n = comp.shape[0]
    slice_cap = int(lib.load().bff_group_slice_cap(n, cap))
    out = {"info": torch.full((4,), GARBAGE, dtype=i32, device=DEV),
           "sizes": torch.full((cap,), GARBAGE, dtype=i32, device=DEV),
           "first": torch.full((cap,), GARBAGE, dtype=i32, device=DEV),
           "offs": torch.full((cap + 1,), GARBAGE, dtype=i32, device=DEV),
           "members": torch.full((n,), GARBAGE, dtype=i32, device=DEV),
           "slices": torch.full((3 * slice_cap,), GARBAGE, dtype=i32, device=DEV)}
    count = (torch.zeros(n, dtype=i32, device=DEV) if count_is_zero
             else torch.randint(-1000, 1000, (n,), dtype=i32, device=DEV))
    p = lib._ptr
    lib.call("bff_group_components", p(comp, i32), p(parent, i32), p(area, i32), n, float(thr), int(mm), int(cap),
             p(count), int(count_is_zero), p(out["info"]), p(out["sizes"]), p(out["first"]), p(out["offs"]),
             p(out["members"]), p(out["slices"]))
    out["slice_cap"] = slice_cap
    return out


def or_reduce_grouped(lib, rows, n_rows, t, cap, conf=None, chunk_mask=None):
    nw = rows.shape[1]
    out = torch.full((cap, nw), GARBAGE, dtype=i64, device=DEV)
    mean = None if conf is None else torch.full((cap,), float("nan"), dtype=conf.dtype, device=DEV)
    p = lib._ptr
    lib.call("bff_or_reduce_grouped", p(rows, i64), nw, n_rows, p(t["info"]), cap, p(t["offs"]), p(t["members"]),
             p(t["slices"]), p(out), p(conf), 1 if (conf is not None and conf.dtype == torch.float16) else 0, p(mean),
             p(chunk_mask, i64))
    return out, mean


def check_tables(t, ref, cap, n):
    info = t["info"].cpu().numpy()
    assert info.tolist() == ref["info"].tolist()
    k = min(ref["K"], cap)
    assert np.array_equal(t["sizes"].cpu().numpy()[:k], ref["sizes"])
    assert np.array_equal(t["first"].cpu().numpy()[:k], ref["first"])
    offs = t["offs"].cpu().numpy()
    assert np.array_equal(offs[:k + 1], ref["offs"])
    assert (offs[k + 1:] == ref["offs"][k]).all()                  # offs[g] == offs[K] for K < g <= cap
    assert np.array_equal(t["members"].cpu().numpy()[:ref["offs"][k]], ref["members"])
    sl = t["slices"].cpu().numpy().reshape(3, t["slice_cap"])[:, :info[3]].T
    assert np.array_equal(sl, ref["slices"])
    if sl.size:                                                    # the triples partition the members, <= 32 in order
        g, lo, hi = sl.T
        assert np.array_equal(np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]), np.arange(offs[k]))
        assert ((hi - lo) <= 32).all() and (offs[g] <= lo).all() and (hi <= offs[g + 1]).all()


# ------------------------------------------------------------------ bff_group_components
# (n_rows, cap, K, special group sizes, iou_thres, min_members, singletons with area > 0)
GROUP_CASES = [
    (0, 256, 0, [], 0.5, 1, 0),
    (1, 1, 1, [], 0.5, 1, 1),                          # one kept singleton, K == cap
    (1, 256, 0, [], 1.0, 1, 1),                        # thr >= 1: no self loops, the singleton is void
    (63, 256, 12, [31], 0.5, 1, 5),
    (64, 1, 1, [32], 1.5, 1, 3),                       # K == cap, live singletons void
    (65, 1, 2, [33, 31], 0.5, 2, 0),                   # K == cap + 1
    (65, 256, 0, [], 1.0, 0, 40),                      # only voids, min_members 0: flag bit 1
    (1000, 1, 300, [64, 65], -1.0, -1, 100),           # K >> cap, negative min_members: both flags
    (1000, 256, 40, [2, 3, 4, 31], 0.5, 5, 20),        # groups below min_members are dropped
    (4096, 256, 255, [31, 32, 33, 64, 65], 0.5, 1, 40),
    (4097, 256, 256, [31, 32, 33, 64, 65], 0.5, 2, 40),
    (4097, 256, 257, [31, 32, 33, 64, 65], 0.5, 1, 40),
    (9000, 512, 512, [1100, 65, 64, 33, 32, 31], 0.5, 5, 0),
    (9000, 512, 511, [2100], 1.0, 1, 50),
    (38400, 512, 513, [1025, 1100, 5000, 65, 33], 0.5, 1, 200),
    (38400, 256, 2000, [1500, 64], -1.0, 0, 300),
    (38400, 512, 300, [20000, 2048, 32], 0.5, 1, 0),
]
FORMS = [("forest", "chain", True), ("forest", "random", False), ("comp", "random", False), ("comp", "chain", True)]


@pytest.mark.parametrize("form,tree,count_is_zero", FORMS, ids=[f"{f}-{t}-{'zeroed' if z else 'garbage'}" for f, t, z in FORMS])
@pytest.mark.parametrize("case", GROUP_CASES, ids=[f"n{c[0]}-cap{c[1]}-K{c[2]}-thr{c[4]}-mm{c[5]}" for c in GROUP_CASES])
def test_group_components_tables(lib, case, form, tree, count_is_zero):
    n, cap, k_goal, special, thr, mm, alive = case
    rng = np.random.default_rng(n * 7 + cap + k_goal)
    parent, comp, area = build_components(rng, n, k_goal, special, thr, mm, alive, tree)
    ref = group_tables_ref(comp, area, thr, mm, cap)
    assert ref["K"] == k_goal
    if form == "forest":
        comp_d = torch.full((n,), GARBAGE, dtype=i32, device=DEV)    # an output here
        t = group_components(lib, comp_d, dev(parent), dev(area), thr, mm, cap, count_is_zero)
        assert np.array_equal(comp_d.cpu().numpy(), comp)            # the forest flattened on the way
    else:
        t = group_components(lib, dev(comp), None, dev(area), thr, mm, cap, count_is_zero)
    check_tables(t, ref, cap, n)


# ------------------------------------------------------------------ bff_or_reduce_grouped
@pytest.mark.parametrize("flags", [False, True], ids=["dense", "chunk_mask"])
@pytest.mark.parametrize("nw", [1, 15, 1023, 1024, 1024 + 77, 8192 + 77])
def test_or_reduce_grouped(lib, nw, flags):
    """OR of the member rows for g < min(K, cap), zero rows after that (out pre-filled with garbage), sequential
    confidence means in f16 and f32 -- including a group of > 2048 members whose f16 running sum passes 512."""
    rng = np.random.default_rng(nw + flags)
    if nw == 15:                                            # K > cap: the first cap groups only
        r, cap, k_goal, special = 3000, 64, 90, [2100, 65]
    elif nw <= 1024 + 77:
        r, cap, k_goal, special = 3000, 256, 120, [2100, 64, 65, 33, 32, 31]
    else:
        r, cap, k_goal, special = 400, 256, 40, [65, 64, 33, 32, 31]
    _, comp, area = build_components(rng, r, k_goal, special, 0.5, 1, 10)
    ref = group_tables_ref(comp, area, 0.5, 1, cap)
    t = group_components(lib, dev(comp), None, dev(area), 0.5, 1, cap, 1)
    check_tables(t, ref, cap, r)
    dense = sparse_rows(rng, r, nw)
    dense[rng.integers(0, r, 3), -1] = np.uint64(7)          # the ragged last chunk
    rows = dev(dense.view(np.int64), i64)
    k = min(ref["K"], cap)
    exp = np.zeros((cap, nw), np.uint64)
    for g in range(k):
        exp[g] = np.bitwise_or.reduce(dense[ref["members"][ref["offs"][g]:ref["offs"][g + 1]]], axis=0)
    cm = None
    if flags:
        cm = lib.row_stats(rows)[2]
        if nw >= or_sparse_min_nw():                        # flagged path: unflagged chunks are never read
            fl = np.unpackbits(cm.cpu().numpy().view(np.uint8), axis=-1, bitorder="little")[:, :(nw + 7) // 8].astype(bool)
            poisoned = dense.copy()
            poisoned[~np.repeat(fl, 8, axis=1)[:, :nw]] = np.uint64(0xDEADBEEF)
            rows = dev(poisoned.view(np.int64), i64)
    for dtype in (torch.float16, torch.float32):
        conf = torch.from_numpy(rng.uniform(0.2, 1.0, r)).to(dtype)
        out, mean = or_reduce_grouped(lib, rows, r, t, cap, conf.to(DEV), cm)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), exp), dtype
        groups = [ref["members"][ref["offs"][g]:ref["offs"][g + 1]].tolist() for g in range(k)]
        want = torch.stack([sum([conf[i] for i in g]) / len(g) for g in groups])      # P:225, sequential in dtype
        got = mean.cpu()[:k]
        assert got.dtype == dtype and torch.equal(got, want), (dtype, (got != want).nonzero()[:5].flatten().tolist())
        if dtype == torch.float16 and nw != 8192 + 77:
            big = max(range(k), key=lambda g: len(groups[g]))
            assert len(groups[big]) > 2048 and float(sum([conf[i] for i in groups[big]])) > 512
    out, mean = or_reduce_grouped(lib, rows, r, t, cap, None, cm)       # without confidences
    assert mean is None and np.array_equal(out.cpu().numpy().view(np.uint64), exp)


def test_or_reduce_grouped_rejects_too_many_slices_before_touching_out(lib):
    """slice_cap + 1 > 65535 (grid limit): BFF_E_LIMIT, and the output is not cleared first."""
    cap, nw = 512, 3
    n_rows = 32 * (65535 - cap)                                # bff_group_slice_cap = n_rows / 32 + cap + 1
    assert lib.load().bff_group_slice_cap(n_rows, cap) + 1 > 65535
    out = torch.full((cap, nw), 0x5EED, dtype=i64, device=DEV)
    small = torch.zeros(16, dtype=i32, device=DEV)             # never read: the call fails before any launch
    rows = torch.zeros((1, nw), dtype=i64, device=DEV)
    p = lib._ptr
    rc = lib.load().bff_or_reduce_grouped(p(rows), nw, n_rows, p(small), cap, p(small), p(small), p(small), p(out),
                                          None, 0, None, None, None)
    torch.cuda.synchronize()
    assert rc == -2 and b"member slices" in lib.load().bff_last_error()
    assert bool((out == 0x5EED).all())


# ------------------------------------------------------------------ bff_clear_flagged_chunks_unless
@pytest.mark.parametrize("veto", [0, 1, 2, 3])
def test_clear_flagged_chunks_unless(lib, veto):
    rng = np.random.default_rng(veto)
    r, nw = 37, (5 * 512 + 77 + 63) // 64                      # ragged last chunk
    dense = sparse_rows(rng, r, nw)
    dense[5, -1] = np.uint64(1)
    rows = dev(dense.view(np.int64), i64)
    cm = lib.row_stats(rows)[2]
    v = torch.tensor([veto], dtype=i32, device=DEV)
    lib.call("bff_clear_flagged_chunks_unless", lib._ptr(rows, i64), r, nw, lib._ptr(cm, i64), lib._ptr(v))
    if veto == 0:
        assert int(rows.count_nonzero()) == 0
    else:
        assert np.array_equal(rows.cpu().numpy().view(np.uint64), dense) and dense.any()


# ------------------------------------------------------------------ bff_resolve_overlaps_dev
@pytest.mark.parametrize("with_keep", [False, True], ids=["no_keep", "keep"])
@pytest.mark.parametrize("cap", [256, 512])
def test_resolve_overlaps_dev(lib, cap, with_keep):
    rng = np.random.default_rng(cap + with_keep)
    n = 2000
    d = rng.random((cap, n)) < 0.01
    sizes = rng.integers(1, 6, cap).astype(np.int32)            # many ties
    keep_np = rng.random(n) < 0.7
    keep = pack_np(keep_np[None])[0] if with_keep else None
    sizes_d = dev(sizes)
    p = lib._ptr
    for kd in (0, 1, 2, 63, 65, cap // 2 + 3, cap, cap + 1):
        rows = pack_np(d)                                      # rows >= *k_dev hold data too: they must stay as they are
        before = torch.full((cap,), GARBAGE, dtype=i32, device=DEV)
        after = torch.full((cap,), GARBAGE, dtype=i32, device=DEV)
        kdev = torch.tensor([kd], dtype=i32, device=DEV)
        lib.call("bff_resolve_overlaps_dev", p(rows, i64), cap, rows.shape[1], p(sizes_d), p(keep, i64), p(before),
                 p(after), p(kdev))
        got = unpack(rows, n)
        if kd == 0 or kd > cap:
            assert np.array_equal(got, d), kd
            continue
        assert np.array_equal(got[kd:], d[kd:]), kd
        ref = pack_np(d[:kd])
        b2, a2 = lib.resolve_overlaps_filtered(ref, dev(sizes[:kd]), keep)
        assert np.array_equal(got[:kd], unpack(ref, n)), kd
        assert torch.equal(before[:kd], b2) and torch.equal(after[:kd], a2), kd
        assert np.array_equal(before[:kd].cpu().numpy(), d[:kd].sum(1))
        assert np.array_equal(after[:kd].cpu().numpy(), got[:kd].sum(1))
        if kd <= 300:
            exp = pref.resolve_overlaps(torch.from_numpy(d[:kd].copy()), [list(range(s)) for s in sizes[:kd]]).numpy()
            if with_keep:
                exp &= keep_np
            assert np.array_equal(got[:kd], exp), kd


# ------------------------------------------------------------------ bff_scatter_bits
@pytest.mark.parametrize("n", [1, 63, 64, 65, 10_001, 200_003])
def test_scatter_bits(lib, n):
    rng = np.random.default_rng(n)
    r = 70
    d = rng.random((r, n)) < 0.05
    d[3] = True
    perm = rng.permutation(n).astype(np.int32)                 # sorted position s holds original point perm[s]
    rows_in = pack_np(d)
    nw = rows_in.shape[1]
    if n % 64:                                                 # set bits past n in the last word are ignored
        rows_in[:, -1] |= torch.tensor(-1 << (n % 64), dtype=i64, device=DEV)
    exp = np.zeros((r, n), bool)
    exp[:, perm] = d
    perm_d = dev(perm)
    p = lib._ptr
    for kd in (None, 0, 1, 65, r, r + 1):
        out = torch.zeros((r, nw), dtype=i64, device=DEV)
        kdev = None if kd is None else torch.tensor([kd], dtype=i32, device=DEV)
        lib.call("bff_scatter_bits", p(rows_in, i64), r, nw, p(perm_d), n, nw, p(out), p(kdev))
        lim = r if kd is None else min(kd, r)
        want = exp.copy()
        want[lim:] = False
        assert np.array_equal(unpack(out, n), want), kd
        assert torch.equal(out, pack_np(want)), kd                 # nothing past n either


# ------------------------------------------------------------------ bff_cross_popcount_dev
def cross_ref(a, b):
    return np.stack([np.bitwise_count(a[i][None] & b).sum(1, dtype=np.int64) for i in range(a.shape[0])]) \
        if a.shape[0] else np.zeros((0, b.shape[0]), np.int64)


@pytest.mark.parametrize("na,nw", [(1, 1), (5, 100), (70, 100), (1, 3125), (5, 3125), (70, 3125), (1, 15625), (5, 15625)])
def test_cross_popcount_dev_scene_shape(lib, na, nw):
    """a = stage-1 rows, b = [cap group rows, the first *k_dev non-zero ; the stage-1 rows], lead = cap, limit_a = 0."""
    rng = np.random.default_rng(na * 100_000 + nw)
    cap = 256
    s1 = rng.integers(0, 2 ** 63, (na, nw), dtype=np.uint64) & rng.integers(0, 2 ** 63, (na, nw), dtype=np.uint64)
    agg = rng.integers(0, 2 ** 63, (cap, nw), dtype=np.uint64) * (rng.random((cap, nw)) < 0.3)
    full = cross_ref(s1, np.concatenate([agg, s1]))
    p = lib._ptr
    a = dev(s1.view(np.int64), i64)
    for kd in (0, 1, 63, 64, 65, cap):
        b_np = np.concatenate([agg, s1])
        b_np[kd:cap] = 0
        b = dev(b_np.view(np.int64), i64)
        inter = torch.full((na, cap + na), GARBAGE, dtype=i32, device=DEV)
        kdev = torch.tensor([kd], dtype=i32, device=DEV)
        lib.call("bff_cross_popcount_dev", p(a, i64), na, p(b, i64), cap + na, nw, p(inter), p(kdev), 0, cap)
        exp = full.copy()
        exp[:, kd:cap] = 0
        assert np.array_equal(inter.cpu().numpy(), exp), kd


@pytest.mark.parametrize("nw", [1, 100, 3125])
def test_cross_popcount_dev_limit_a(lib, nw):
    """limit_a = 1: a = the cap group rows, zero past *k_dev; b = [those rows ; 5 more rows], lead = cap."""
    rng = np.random.default_rng(nw + 1)
    cap, extra = 256, 5
    agg = rng.integers(0, 2 ** 63, (cap, nw), dtype=np.uint64) * (rng.random((cap, nw)) < 0.3)
    tail = rng.integers(0, 2 ** 63, (extra, nw), dtype=np.uint64)
    full = cross_ref(agg, np.concatenate([agg, tail]))
    p = lib._ptr
    for kd in (0, 1, 63, 64, 65, cap):
        a_np = agg.copy()
        a_np[kd:] = 0
        a = dev(a_np.view(np.int64), i64)
        b = dev(np.concatenate([a_np, tail]).view(np.int64), i64)
        inter = torch.full((cap, cap + extra), GARBAGE, dtype=i32, device=DEV)
        kdev = torch.tensor([kd], dtype=i32, device=DEV)
        lib.call("bff_cross_popcount_dev", p(a, i64), cap, p(b, i64), cap + extra, nw, p(inter), p(kdev), 1, cap)
        exp = full.copy()
        exp[kd:] = 0
        exp[:, kd:cap] = 0
        assert np.array_equal(inter.cpu().numpy(), exp), kd


# ------------------------------------------------------------------ the chain, as the scene call runs it
def test_scene_tail_chain_against_the_oracle(lib):
    """row_stats -> (label, signature) order -> merge_components leaving the forest -> bff_group_components (forest) ->
    bff_or_reduce_grouped -> bff_resolve_overlaps_dev (keep) -> bff_scatter_bits, on random raw rows in a permuted
    point order == the oracle's aggregate + solve_overlapping + & keep on the rows in the original order."""
    rng = np.random.default_rng(2024)
    r, n, thr, mm, cap = 1500, 20_000, 0.2, 1, 512
    centres = rng.integers(0, n, 60)
    d = np.zeros((r, n), bool)
    for i in range(r):
        c = int(centres[rng.integers(0, centres.size)])
        w = int(rng.integers(20, 600))
        d[i, max(0, c - w):c + w] = True
        d[i] &= rng.random(n) < 0.8
    d[rng.integers(0, r, 6)] = False                                 # empty rows: void singletons
    label_names = ["chair", "table", "lamp"]
    lab = rng.integers(0, 3, r)
    labels = [label_names[x] for x in lab]
    conf = torch.from_numpy(rng.uniform(0.2, 1.0, r)).to(torch.float16)
    keep_np = rng.random(n) < 0.9
    perm = rng.permutation(n).astype(np.int32)                       # sorted position s holds original point perm[s]

    rows = pack_np(d[:, perm])
    nw = rows.shape[1]
    lid = dev(lab)
    area, mean_word, cmask, hist, sig = lib.row_stats(rows)
    order = lib.argsort_i64((lid.long() << lib.SIGNATURE_BITS) | sig)
    parent = torch.empty(r, dtype=i32, device=DEV)
    tmask = torch.empty(((r + 63) // 64, cmask.shape[1]), dtype=i64, device=DEV)
    scratch = torch.empty(int(lib.load().bff_merge_scratch_words(r)), dtype=i32, device=DEV)
    cpop = hist.chunk_pop if lib.load().bff_merge_uses_chunk_bound(nw) else None
    p = lib._ptr
    lib.call("bff_merge_components", p(rows, i64), r, nw, p(order, i32), r, p(cmask, i64), p(tmask), p(hist, i32),
             p(scratch), p(area, i32), p(lid), float(thr), p(parent), 1, None, None, p(cpop, torch.int16))
    comp = torch.empty(r, dtype=i32, device=DEV)
    t = group_components(lib, comp, parent, area, thr, mm, cap, 1)
    agg, mean = or_reduce_grouped(lib, rows, r, t, cap, conf.to(DEV), cmask)
    before = torch.empty(cap, dtype=i32, device=DEV)
    after = torch.empty(cap, dtype=i32, device=DEV)
    keep = pack_np(keep_np[perm][None])[0]
    lib.call("bff_resolve_overlaps_dev", p(agg, i64), cap, nw, p(t["sizes"]), p(keep, i64), p(before), p(after),
             p(t["info"]))
    both = torch.zeros((cap, nw), dtype=i64, device=DEV)
    perm_d = dev(perm)
    lib.call("bff_scatter_bits", p(agg, i64), cap, nw, p(perm_d), n, nw, p(both), p(t["info"]))

    raw = {"ins": torch.from_numpy(d), "conf": conf, "final_class": labels}
    res, groups = pref.aggregate(raw, thr, mm)
    k = len(groups)
    assert 20 < k <= cap
    info = t["info"].cpu().numpy()
    assert info[0] == k and info[1] == 0
    check_tables(t, group_tables_ref(comp.cpu().numpy(), area.cpu().numpy(), thr, mm, cap), cap, r)
    offs, members = t["offs"].cpu().numpy(), t["members"].cpu().numpy()
    assert [members[offs[g]:offs[g + 1]].tolist() for g in range(k)] == groups
    assert torch.equal(mean.cpu()[:k], res["conf"])
    agg_ref = res["ins"].clone()
    assert np.array_equal(before.cpu().numpy()[:k], agg_ref.sum(1).numpy())
    pref.resolve_overlaps(agg_ref, groups)
    agg_ref &= torch.from_numpy(keep_np)
    got = unpack(both, n)
    assert np.array_equal(got[:k], agg_ref.numpy()) and not got[k:].any()
    assert np.array_equal(after.cpu().numpy()[:k], agg_ref.sum(1).numpy())
