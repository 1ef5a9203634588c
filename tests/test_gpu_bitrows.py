"""The bit-row primitives every later subsystem stands on, C entry point by entry point and path by path, against the
plain NumPy statements of tests/bitrows_ref.py: csrc/rows.hip (popcount, cross popcount, clearing flagged chunks, bit
gather, row programs, AND, row gather), csrc/row_codec.hip (dense bytes and ids to rows and back), csrc/graph.hip
(components by label propagation), the ordered pair list of csrc/resolve.hip and the OR of host-formed groups of
csrc/groups.hip.  These are also the paths production falls back to: the general path after bff_scene_project, more
than 4096 groups, host-formed groups, evaluation.

Every call goes through the C ABI with buffers the test owns: outputs are pre-filled with a poison pattern and followed
by guard elements that must come back untouched, inputs lie inside larger allocations, and whole words are compared,
the zero padding of a row's last word included.  Everything is integers and bits: no tolerances.

Not covered here, on purpose:
  * the one-thread walk of overlap_ops_kernel for k > 8192 rows: the intersection matrix alone is 268 MB and the walk
    takes seconds; no scene comes near it;
  * the rocPRIM sorts (bff_sort_f32, bff_argsort_i64), bff_row_stats, the RLE codec (bff_rle_*) and the `_dev`
    variants that read a count on the device: tests/test_gpu_kernels.py, test_gpu_merge_paths.py and
    test_gpu_device_groups.py have them."""
import numpy as np
import pytest
import torch

import bitrows_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
i32, i64, u8 = torch.int32, torch.int64, torch.uint8
POISON64 = 0x5A5AA5A5C3C33C3C                                  # outputs before a call, guards after it
POISON32 = -0x21524111                                         # 0xDEADBEEF as int32
POISON8 = 0xA5
GUARD = 64                                                     # elements after every buffer
E_LIMIT = -2


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


_POISON = {i64: POISON64, i32: POISON32, u8: POISON8, torch.float16: 77.0, torch.float32: 77.0}


class Buf:
    """n elements inside a larger poisoned allocation: `t` is the view a kernel gets, `intact()` whether the elements
    behind it still hold the poison."""

    def __init__(self, n, dtype, data=None, lead=0):
        self.n, self.lead = int(n), int(lead)
        self.whole = torch.full((self.lead + self.n + GUARD,), _POISON[dtype], dtype=dtype, device=DEV)
        self.t = self.whole[self.lead:self.lead + self.n]
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(dtype))

    def ptr(self, lib):
        return lib._ptr(self.t) if self.n else None

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        out = torch.cat([self.whole[:self.lead], self.whole[self.lead + self.n:]])
        return bool((out == _POISON[self.whole.dtype]).all())


def words_buf(words):
    """uint64 (R, nw) -> device int64 copy inside a guarded allocation."""
    words = np.ascontiguousarray(words, np.uint64)
    return Buf(words.size, i64, words.view(np.int64))


def out_words(r, nw):
    return Buf(r * nw, i64)


def as_u64(buf, r, nw):
    return buf.np().view(np.uint64).reshape(r, nw)


def rand_words(rng, r, nw, p_word=1.0):
    """uint64 (r, nw): random words, each kept with probability p_word."""
    w = rng.integers(0, 2 ** 64, (r, nw), dtype=np.uint64)
    if p_word < 1.0:
        w *= (rng.random((r, nw)) < p_word).astype(np.uint64)
    return w


def rand_rows(rng, r, n, p=0.5):
    """bool (r, n) and its words (padding zero)."""
    d = rng.random((r, n)) < p
    return d, br.pack_words(d)


# ------------------------------------------------------------------ bff_popcount_rows
@pytest.mark.parametrize("nw", [0, 1, 63, 64, 255, 256, 257, 1000])
def test_popcount_rows(lib, nw):
    rng = np.random.default_rng(nw)
    r = 6
    words = rand_words(rng, r, nw)
    if nw:
        words[2] = np.uint64(2 ** 64 - 1)                          # the largest count a row of this width has
        words[4] = 0
    dense = br.unpack_words(words, nw * 64)
    rows = words_buf(words)
    for name, idx in (("none", None), ("repeats", [0, 0, 5, 2, 2, 4, 1]), ("descending", [5, 4, 3, 2, 1, 0])):
        n = r if idx is None else len(idx)
        area = Buf(n, i32)
        ib = None if idx is None else Buf(n, i32, np.array(idx, np.int32))
        lib.call("bff_popcount_rows", rows.ptr(lib), None if ib is None else ib.ptr(lib), n, nw, area.ptr(lib))
        want = br.popcount_rows(dense, idx)
        assert np.array_equal(area.np(), want) and area.intact() and rows.intact(), name
        if nw:
            assert want.max() == 64 * nw and want.min() == 0
    assert np.array_equal(as_u64(rows, r, nw), words)


# ------------------------------------------------------------------ bff_cross_popcount
CROSS_CASES = br.CROSS_CASES                                 # (na, nb, nw, z extent of the launch)
CROSS_INDEXED = [(65, 129, 33), (5, 70, 65)]


def run_cross(lib, a, ia, na, b, ib, nb, nw):
    inter = Buf(na * nb, i32)
    lib.call("bff_cross_popcount", a.ptr(lib), None if ia is None else ia.ptr(lib), na, b.ptr(lib),
             None if ib is None else ib.ptr(lib), nb, nw, inter.ptr(lib))
    assert inter.intact() and a.intact() and b.intact()
    return inter.np().reshape(na, nb)


@pytest.mark.parametrize("na,nb,nw,slices", CROSS_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CROSS_CASES])
def test_cross_popcount(lib, na, nb, nw, slices):
    assert lib.load().bff_cross_popcount_slices(na, nb, nw) == slices
    rng = np.random.default_rng(na * 7919 + nb * 31 + nw)
    wa, wb = rand_words(rng, na, nw, 0.8), rand_words(rng, nb, nw, 0.8)
    wa[na // 2] = np.uint64(2 ** 64 - 1)
    wb[nb // 2] = np.uint64(2 ** 64 - 1)                           # one entry reaches 64 nw
    da, db = br.unpack_words(wa, nw * 64), br.unpack_words(wb, nw * 64)
    a, b = words_buf(wa), words_buf(wb)
    want = br.cross_popcount(da, db)
    assert want[na // 2, nb // 2] == 64 * nw
    assert np.array_equal(run_cross(lib, a, None, na, b, None, nb, nw), want)
    if (na, nb, nw) in CROSS_INDEXED:
        # index vectors pick na / nb rows, out of order and with repeats, out of sources of another size
        sa, sb = na + 9, nb + 5
        wa, wb = rand_words(rng, sa, nw, 0.8), rand_words(rng, sb, nw, 0.8)
        da, db = br.unpack_words(wa, nw * 64), br.unpack_words(wb, nw * 64)
        a, b = words_buf(wa), words_buf(wb)
        ia, ib = rng.integers(0, sa, na).astype(np.int32), rng.integers(0, sb, nb).astype(np.int32)
        ia[:2], ib[:3] = sa - 1, (sb - 1, 0, sb - 1)
        iad, ibd = Buf(na, i32, ia), Buf(nb, i32, ib)
        assert np.array_equal(run_cross(lib, a, iad, na, b, None, sb, nw), br.cross_popcount(da, db, ia, None))
        assert np.array_equal(run_cross(lib, a, None, sa, b, ibd, nb, nw), br.cross_popcount(da, db, None, ib))
        assert np.array_equal(run_cross(lib, a, iad, na, b, ibd, nb, nw), br.cross_popcount(da, db, ia, ib))
        assert lib.load().bff_cross_popcount_slices(sa, sb, nw) == slices       # the larger calls stay on the path


@pytest.mark.parametrize("na,nb", [(5, 70), (1500, 1400)], ids=["few_tiles", "many_tiles"])
def test_cross_popcount_zero_width(lib, na, nb):
    """nw == 0: OK and an all-zero matrix, with NULL row pointers, below and above the 512-tile limit."""
    assert lib.load().bff_cross_popcount_slices(na, nb, 0) == 0
    inter = Buf(na * nb, i32)
    lib.call("bff_cross_popcount", None, None, na, None, None, nb, 0, inter.ptr(lib))
    assert not inter.np().any() and inter.intact()
    empty = torch.empty((na, 0), dtype=i64, device=DEV)            # the wrapper hands the NULL of an empty tensor on
    got = lib.cross_popcount(empty, torch.empty((nb, 0), dtype=i64, device=DEV))
    assert got.shape == (na, nb) and not bool(got.any())
    assert not bool(lib.popcount_rows(empty).any())


# ------------------------------------------------------------------ bff_clear_flagged_chunks(_unless)
def flagged_case(rng, r, nw):
    """Fairly dense rows (about 2 of 3 chunks occupied) and flags drawn independently of occupancy over the real chunks;
    row 0's ragged last chunk is occupied and flagged while row 1 starts occupied.  -> (words, flags bool (r, chunks))."""
    nc = (nw + 7) // 8
    occ = np.repeat(rng.random((r, nc)) < 0.66, 8, axis=1)[:, :nw]
    words = (rand_words(rng, r, nw) | np.uint64(1)) * occ.astype(np.uint64)
    flags = rng.random((r, nc)) < 0.5
    flags[0, nc - 1] = True
    words[0, nw - 1] |= np.uint64(1 << 63)
    if r > 1:
        words[1, :min(nw, 8)] |= np.uint64(0x8000000000000001)
        flags[1, 0] = False
    return words, flags


def flag_words(flags, mw):
    pad = np.zeros((flags.shape[0], mw * 64), bool)
    pad[:, :flags.shape[1]] = flags
    return np.packbits(pad, axis=-1, bitorder="little").view(np.uint64).reshape(flags.shape[0], mw)


@pytest.mark.parametrize("entry", ["bff_clear_flagged_chunks", "bff_clear_flagged_chunks_unless"])
@pytest.mark.parametrize("nw", [1, 8, 9, 77, 513, 1029])
def test_clear_flagged_chunks(lib, nw, entry):
    mw = int(lib.load().bff_chunk_mask_words(nw))
    nc = (nw + 7) // 8
    assert mw == (nc + 63) // 64 and (mw > 1) == (nw > 512)
    veto = Buf(1, i32, np.zeros(1, np.int32))
    seen = np.zeros(3, bool)
    for r in (1, 4, 5, 37):
        rng = np.random.default_rng(nw * 100 + r)
        words, flags = flagged_case(rng, r, nw)
        dense = br.unpack_words(words, nw * 64)
        occupied = np.pad(dense, ((0, 0), (0, nc * 512 - nw * 64))).reshape(r, nc, 512).any(axis=2)
        seen |= [(occupied & flags).any(), (occupied & ~flags).any(), (~occupied & flags).any()]
        rows, cm = words_buf(words), words_buf(flag_words(flags, mw))
        if entry.endswith("unless"):
            lib.call(entry, rows.ptr(lib), r, nw, cm.ptr(lib), veto.ptr(lib))
        else:
            lib.call(entry, rows.ptr(lib), r, nw, cm.ptr(lib))
        want = br.pack_words(br.clear_flagged_chunks(dense, flags))
        got = as_u64(rows, r, nw)
        assert np.array_equal(got, want), r                        # the flagged chunks are zero, every other word is as it was
        assert rows.intact() and cm.intact(), r
        assert not got[0, 8 * (nc - 1):].any() and (r == 1 or np.array_equal(got[1, :min(nw, 8)], words[1, :min(nw, 8)]))
    assert seen[0] and (nw == 1 or seen.all())                     # occupied+flagged, occupied+unflagged, empty+flagged
    assert veto.intact()


# ------------------------------------------------------------------ bff_permute_bits
@pytest.mark.parametrize("r", [1, 5])
@pytest.mark.parametrize("n_in,n_out", [(1, 1), (64, 63), (65, 64), (1000, 257), (70, 1000), (10_007, 10_007)])
def test_permute_bits(lib, n_in, n_out, r):
    rng = np.random.default_rng(n_in * 3 + n_out + r)
    d, words = rand_rows(rng, r, n_in)
    d[0, n_in - 1] = True
    words = br.pack_words(d)
    if n_in == n_out:
        idx = rng.permutation(n_in)
    elif n_out < n_in:
        idx = rng.permutation(n_in)[:n_out]
    else:
        idx = rng.integers(0, n_in, n_out)                         # a gather with repeats
        assert np.unique(idx).size < n_out
    idx[0] = n_in - 1
    nw_in, nw_out = words.shape[1], (n_out + 63) // 64
    rows_in, idx_d, out = words_buf(words), Buf(n_out, i32, idx.astype(np.int32)), out_words(r, nw_out)
    lib.call("bff_permute_bits", rows_in.ptr(lib), r, nw_in, idx_d.ptr(lib), n_out, nw_out, out.ptr(lib))
    assert np.array_equal(as_u64(out, r, nw_out), br.pack_words(br.permute_bits(d, idx)))
    assert out.intact() and rows_in.intact() and idx_d.intact()


# ------------------------------------------------------------------ bff_apply_row_ops
ROW_OPS = [(br.OR, 1, 2), (br.ANDNOT, 1, 3), (br.COPY, 4, 1), (br.ANDNOT, 2, 2), (br.OR, 3, 3), (br.COPY, 0, 0),
           (br.OR, 1, 4), (br.ANDNOT, 3, 1)]                   # every opcode, every opcode with dst == src; row 5 unnamed


@pytest.mark.parametrize("nw", [1, 256, 257, 600])
def test_apply_row_ops(lib, nw):
    rng = np.random.default_rng(nw)
    r, n = 6, nw * 64
    d, words = rand_rows(rng, r, n)
    want = br.apply_row_ops(d, ROW_OPS)
    assert not np.array_equal(want, br.apply_row_ops(d, ROW_OPS[::-1]))      # the order of this list matters
    assert np.array_equal(want[5], d[5]) and not want[2].any() and np.array_equal(want[3], d[3] & ~want[1])
    flat = np.array(ROW_OPS, np.int32).reshape(-1)
    host_list = Buf(flat.size, i32, flat)
    dev_list = Buf(1 + flat.size, i32, np.concatenate([[len(ROW_OPS)], flat]).astype(np.int32))
    empty_list = Buf(1 + flat.size, i32, np.concatenate([[0], flat]).astype(np.int32))
    for name, ops, n_ops, exp in (("host count", host_list, len(ROW_OPS), want), ("device list", dev_list, -1, want),
                                  ("device list, count 0", empty_list, -1, d), ("host count 0", host_list, 0, d),
                                  ("host count 3", host_list, 3, br.apply_row_ops(d, ROW_OPS[:3]))):
        rows = words_buf(words)
        lib.call("bff_apply_row_ops", rows.ptr(lib), nw, ops.ptr(lib), n_ops)
        assert np.array_equal(as_u64(rows, r, nw), br.pack_words(exp)), name
        assert rows.intact() and ops.intact(), name


# ------------------------------------------------------------------ bff_and_rows, bff_gather_rows
@pytest.mark.parametrize("r", [1, 70])
@pytest.mark.parametrize("nw", [1, 256, 257])
def test_and_rows(lib, nw, r):
    rng = np.random.default_rng(nw + r)
    d, words = rand_rows(rng, r, nw * 64)
    kd, kw = rand_rows(rng, 1, nw * 64)
    rows, keep = words_buf(words), words_buf(kw)
    lib.call("bff_and_rows", rows.ptr(lib), r, nw, keep.ptr(lib))
    assert np.array_equal(as_u64(rows, r, nw), br.pack_words(br.and_rows(d, kd[0])))
    assert rows.intact() and keep.intact() and np.array_equal(as_u64(keep, 1, nw), kw)


@pytest.mark.parametrize("r", [1, 70])
@pytest.mark.parametrize("nw", [1, 256, 257])
def test_gather_rows(lib, nw, r):
    rng = np.random.default_rng(nw * 2 + r)
    src = 9
    d, words = rand_rows(rng, src, nw * 64)
    idx = rng.integers(0, src, r)
    idx[0] = src - 1
    if r > 1:
        idx[1] = src - 1                                           # a repeat, for certain
    rows, idx_d, out = words_buf(words), Buf(r, i32, idx.astype(np.int32)), out_words(r, nw)
    lib.call("bff_gather_rows", rows.ptr(lib), idx_d.ptr(lib), r, nw, out.ptr(lib))
    assert np.array_equal(as_u64(out, r, nw), br.pack_words(br.gather_rows(d, idx)))
    assert out.intact() and rows.intact() and np.array_equal(as_u64(rows, src, nw), words)


# ------------------------------------------------------------------ bff_unpack_rows, bff_pack_rows
CODEC_N = [1, 7, 8, 9, 63, 64, 65, 1001, 2049]


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("n", CODEC_N)
def test_unpack_rows(lib, n, r):
    """Byte offset 0: row 0 is 8-aligned, later rows are iff n % 8 == 0.  Byte offset 3: no row is when n % 8 == 0, so
    every thread takes the byte-by-byte path; odd n mixes both."""
    rng = np.random.default_rng(n * 4 + r)
    d, words = rand_rows(rng, r, n)
    d[:, :min(n, 16)] = np.resize([True, False, False, True, True, True, False, True, False, False], (r, min(n, 16)))
    words = br.pack_words(d)
    nw = words.shape[1]
    rows = words_buf(words)
    for off in (0, 3):
        dense = Buf(r * n, u8, lead=off)
        assert dense.whole.data_ptr() % 8 == 0 and dense.t.data_ptr() % 8 == off
        lib.call("bff_unpack_rows", rows.ptr(lib), r, nw, n, dense.ptr(lib))
        assert np.array_equal(dense.np().reshape(r, n), br.unpack_bytes(d)), off
        assert dense.intact() and rows.intact(), off                # the bytes before and after the rows


@pytest.mark.parametrize("kind", ["bool", "bytes"])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("n", CODEC_N)
def test_pack_rows(lib, n, r, kind):
    rng = np.random.default_rng(n * 8 + r)
    if kind == "bool":
        byts = (rng.random((r, n)) < 0.5).astype(np.uint8)
    else:
        byts = rng.choice(np.array([0, 0, 0, 1, 2, 128, 255], np.uint8), size=(r, n))      # not 0 means set
        byts[0, :min(n, 5)] = [0, 1, 2, 128, 255][:min(n, 5)]
    nw = (n + 63) // 64
    want = br.pack_words(br.pack_bytes(byts))
    for off in (0, 3):
        dense, rows = Buf(r * n, u8, byts, lead=off), out_words(r, nw)
        src = dense.t.view(torch.bool) if kind == "bool" else dense.t
        lib.call("bff_pack_rows", lib._ptr(src), r, n, nw, rows.ptr(lib))
        assert np.array_equal(as_u64(rows, r, nw), want), off
        assert rows.intact() and dense.intact() and np.array_equal(dense.np().reshape(r, n), byts), off


# ------------------------------------------------------------------ bff_ids_to_rows
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_ids_to_rows(lib, n):
    """Ids equal in their low 32 bits (5 and 2^32 + 5; -7 and 2^32 - 7) are different ids."""
    rng = np.random.default_rng(n)
    pool = np.array([5, (1 << 32) + 5, -7, (1 << 32) - 7, 3, 0, (1 << 40) + 3], np.int64)
    values = np.array([5, (1 << 32) + 5, -7, 3, 3, 99, 0], np.int64)            # a duplicate (3) and an absent id (99)
    ids = pool[rng.integers(0, pool.size, n)]
    ids[0] = (1 << 32) + 5                                         # n == 1: the row of 5 must stay empty
    ids[-1] = (1 << 32) + 5
    nw = (n + 63) // 64
    ids_d, val_d, rows = Buf(n, i64, ids), Buf(values.size, i64, values), out_words(values.size, nw)
    lib.call("bff_ids_to_rows", ids_d.ptr(lib), n, val_d.ptr(lib), values.size, nw, rows.ptr(lib))
    want = br.ids_to_rows(ids, values)
    assert np.array_equal(as_u64(rows, values.size, nw), br.pack_words(want))
    assert rows.intact() and ids_d.intact() and val_d.intact()
    assert not want[0, 0] and want[1, 0] and not want[5].any()
    if n >= 64:
        assert want[0].any() and want[2].any() and not (want[0] & want[1]).any()


# ------------------------------------------------------------------ bff_components_round through lib.components
def component_graphs(n, rng):
    i = np.arange(n)
    eye = np.eye(n, dtype=bool)
    chain = np.zeros((n, n), bool)
    chain[i[:-1], i[:-1] + 1] = True
    star = np.zeros((n, n), bool)
    star[n - 1, :n - 1] = True
    two = np.zeros((n, n), bool)
    two[i[:-2], i[:-2] + 2] = True
    sparse = np.triu(rng.random((n, n)) < 1.2 / max(n, 2), 1)
    return {"no edges, self loops": eye, "no edges, no self loops": np.zeros((n, n), bool),
            "complete": np.ones((n, n), bool), "chain": chain | chain.T | eye, "star, hub n - 1": star | star.T | eye,
            "evens and odds": two | two.T | eye, "sparse random": sparse | sparse.T | eye,
            "sparse random, no self loops": sparse | sparse.T}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 3000])
def test_components_labels_are_the_component_minima(lib, n):
    rng = np.random.default_rng(n)
    for name, adj in component_graphs(n, rng).items():
        want = br.component_minima(adj)
        bits = words_buf(br.pack_words(adj))
        got = lib.components(bits.t.view(n, (n + 63) // 64))
        assert got.dtype == i32 and np.array_equal(got.cpu().numpy(), want), name
        assert bits.intact(), name
        if name == "evens and odds" and n >= 2:
            assert np.array_equal(want, np.arange(n) % 2)
        if name in ("complete", "chain", "star, hub n - 1"):
            assert not want.any()


# ------------------------------------------------------------------ bff_overlap_ops
def overlap_case(rng, k):
    """Sparse symmetric intersections: about 6 partners per row, a hub row that overlaps every row but the isolated
    ones, every 7th row isolated (no overlap at all), sizes 1..3 (ties everywhere)."""
    m = np.triu(rng.random((k, k)) < min(0.5, 6.0 / k), 1)
    inter = ((m | m.T) * rng.integers(1, 100, (k, k))).astype(np.int32)
    inter = np.maximum(inter, inter.T)
    hub = k // 2
    inter[hub, :] = inter[:, hub] = 1
    alone = np.arange(3, k, 7)
    alone = alone[alone != hub]
    inter[alone, :] = 0
    inter[:, alone] = 0
    inter[np.arange(k), np.arange(k)] = 50                         # a row overlaps itself; the list has i < j only
    return inter, rng.integers(1, 4, k).astype(np.int32)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128, 129, 1024, 1025, 2049])
def test_overlap_ops_is_the_ordered_list(lib, k):
    """k > 1024: a thread of the scan owns more than one row; the column loop starts at (i + 1) & ~63."""
    rng = np.random.default_rng(k)
    inter, size = overlap_case(rng, k)
    want = br.overlap_ops(inter, size)
    cap = 1 + 3 * (k * (k - 1) // 2)
    inter_d, size_d, ops = Buf(k * k, i32, inter), Buf(k, i32, size), Buf(cap, i32)
    lib.call("bff_overlap_ops", inter_d.ptr(lib), size_d.ptr(lib), k, ops.ptr(lib))
    got = ops.np()
    assert got[0] == len(want)
    assert np.array_equal(got[1:1 + 3 * len(want)].reshape(-1, 3), want)
    assert (got[1 + 3 * len(want):] == POISON32).all() and ops.intact() and inter_d.intact() and size_d.intact()
    if k >= 63:
        i, j = want[:, 1], want[:, 2]
        assert len(want) > k and (size[i] == size[j]).any() and (size[i] < size[j]).any() and (i > j).any() and (i < j).any()
        assert not np.isin(np.arange(3, k, 7)[:1], want[:, 1:]).any()


# ------------------------------------------------------------------ bff_or_reduce_groups
OR_GROUPS = {"direct": ([1, 31, 0, 32], 32),                   # max_group_size 32: one z slice, stored directly
             "sliced": ([33, 64, 0, 65, 1025], 1025)}          # z slices meet through atomics in a zeroed output


@pytest.mark.parametrize("path", list(OR_GROUPS))
@pytest.mark.parametrize("nw", [1, 255, 256, 257])
def test_or_reduce_groups(lib, nw, path):
    """An empty group in the middle gets an all-zero row on both paths and the mean 0 / 0 = NaN."""
    sizes, max_size = OR_GROUPS[path]
    rng = np.random.default_rng(nw + max_size)
    r, k = 1300, len(sizes)
    words = rand_words(rng, r, nw, 0.02)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    members = rng.permutation(r)[:offs[-1]].astype(np.int32)
    words[members[0]] = 0                                          # direct: group 0 is this row alone, and all-zero rows are stored too
    words[members[offs[1]], 0] |= np.uint64(1)
    words[members[-1], nw - 1] |= np.uint64(1 << 63)
    dense = br.unpack_words(words, nw * 64)
    want = br.pack_words(br.or_reduce_groups(dense, offs, members))
    assert not want[2].any() and want[1].any() and want[-1].any() and (path == "sliced" or not want[0].any())
    rows, offs_d, mem_d = words_buf(words), Buf(k + 1, i32, offs), Buf(members.size, i32, members)
    for dtype in (None, torch.float16, torch.float32):
        out = out_words(k, nw)
        conf = mean = conf_np = None
        if dtype is not None:
            conf_np = rng.uniform(0.2, 1.0, r).astype(np.float16 if dtype == torch.float16 else np.float32)
            conf, mean = Buf(r, dtype, conf_np), Buf(k, dtype)
        lib.call("bff_or_reduce_groups", rows.ptr(lib), nw, offs_d.ptr(lib), mem_d.ptr(lib), k, max_size, out.ptr(lib),
                 None if conf is None else conf.ptr(lib), 1 if dtype == torch.float16 else 0,
                 None if mean is None else mean.ptr(lib), None)
        assert np.array_equal(as_u64(out, k, nw), want), dtype
        assert out.intact() and rows.intact() and offs_d.intact() and mem_d.intact(), dtype
        if dtype is not None:
            want_mean = br.or_reduce_groups(dense, offs, members, conf_np)[1]
            got = mean.np()
            assert got.dtype == want_mean.dtype and np.isnan(got[2]) and np.isnan(want_mean[2]), dtype
            keep = np.array(sizes) > 0
            assert np.array_equal(got[keep].view(np.uint8), want_mean[keep].view(np.uint8)), dtype      # bit for bit
            assert mean.intact() and conf.intact(), dtype


# ------------------------------------------------------------------ host limits: refused before any launch
def test_row_counts_beyond_the_grid_are_refused_before_anything_is_touched(lib):
    """n_rows becomes the launch's y extent (<= 65535): BFF_E_LIMIT, a message, and no output written.  The buffers are
    tiny and never read: nothing is launched."""
    n = 65536
    mark = 0x5EED
    out = torch.full((16,), mark, dtype=i64, device=DEV)
    small = torch.zeros(16, dtype=i64, device=DEV)
    o, s = lib._ptr(out), lib._ptr(small)
    L = lib.load()
    calls = {
        "bff_pack_rows": lambda: L.bff_pack_rows(s, n, 1, 1, o, None),
        "bff_unpack_rows": lambda: L.bff_unpack_rows(s, n, 1, 1, o, None),
        "bff_and_rows": lambda: L.bff_and_rows(o, n, 1, s, None),
        "bff_gather_rows": lambda: L.bff_gather_rows(s, s, n, 1, o, None),
        "bff_permute_bits": lambda: L.bff_permute_bits(s, n, 1, s, 1, 1, o, None),
        "bff_rle_to_rows": lambda: L.bff_rle_to_rows(s, s, s, n, 1, 1, o, None),
    }
    for name, fn in calls.items():
        rc = fn()
        torch.cuda.synchronize()
        msg = L.bff_last_error()
        assert rc == E_LIMIT and name.encode() in msg and b"too many rows" in msg, (name, rc, msg)
        assert bool((out == mark).all()) and not bool(small.any()), name
