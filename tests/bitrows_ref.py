"""Plain statements of the bit-row primitives (csrc/rows.hip, row_codec.hip, graph.hip, the pair list of resolve.hip and
the host-group OR of groups.hip) on dense boolean arrays and Python integers.  NumPy only: nothing here touches the GPU
or the library.  tests/test_bitrows_ref_host.py pins every function to the oracle where the oracle has the operation
and to a literal per-bit loop where it has not; tests/test_gpu_bitrows.py compares the kernels with them.

A row over n points is a bool vector; its packed form is ceil(n / 64) uint64 words, point p = bit (p & 63) of word
p >> 6, padding bits zero.  A chunk is 8 words = 512 points (the granularity of the occupancy flags)."""
import numpy as np

CHUNK_POINTS = 512                                           # 8 words of 64 points

ANDNOT, OR, COPY = 0, 1, 2                                   # opcodes of bff_apply_row_ops


# ------------------------------------------------------------------ packed form
def pack_words(dense):
    """bool (R, n) -> uint64 (R, ceil(n / 64)), padding bits zero."""
    dense = np.asarray(dense, bool)
    r, n = dense.shape
    nw = (n + 63) // 64
    pad = np.zeros((r, nw * 64), bool)
    pad[:, :n] = dense
    return np.packbits(pad, axis=-1, bitorder="little").view(np.uint64).reshape(r, nw)


def unpack_words(words, n):
    """uint64 (R, nw) -> bool (R, n): the first n points of every row."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], 8 * words.shape[1]), axis=-1, bitorder="little")
    return bits[:, :n].astype(bool)


# ------------------------------------------------------------------ counts
def popcount_rows(dense, idx=None):
    """area[r] = number of points of row idx[r] (idx None: row r)."""
    dense = np.asarray(dense, bool)
    if idx is not None:
        dense = dense[np.asarray(idx, np.int64)]
    return dense.sum(axis=1, dtype=np.int64)


def cross_popcount(a, b, ia=None, ib=None):
    """inter[i][j] = |a[ia[i]] & b[ib[j]]|, int64.  The {0, 1} product in float64 is exact: every count is < 2^53."""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    if ia is not None:
        a = a[np.asarray(ia, np.int64)]
    if ib is not None:
        b = b[np.asarray(ib, np.int64)]
    return np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def cross_popcount_slices(na, nb, nw):
    """bff_cross_popcount_slices restated (include/bff_hip.h): the z extent of bff_cross_popcount's launch.  Fewer than
    512 tiles of 64 x 64 pairs: the words are cut into slices of ceil(nw * tiles / 512) words, rounded up to a multiple of
    32 and at least 64; otherwise one slice.  0: nothing to launch."""
    if na <= 0 or nb <= 0 or nw <= 0:
        return 0
    tiles = ((na + 63) // 64) * ((nb + 63) // 64)
    if tiles >= 512:
        return 1
    per = max(64, (((nw * tiles + 511) // 512 + 31) // 32) * 32)
    return (nw + per - 1) // per


# (na, nb, nw, z extent): the shapes tests/test_gpu_bitrows.py runs.  1 = direct store, > 1 = atomics into a zeroed matrix
CROSS_CASES = [
    (1, 1, 1, 1),
    (63, 65, 31, 1),
    (64, 64, 32, 1),
    (65, 129, 33, 1),
    (5, 70, 65, 2),                                          # the smallest atomic case
    (130, 3, 1000, 16),                                      # 3 tiles: 64-word slices
    (1500, 1400, 3, 1),                                      # 528 tiles >= 512: unsplit
]


# ------------------------------------------------------------------ edits
def clear_flagged_chunks(dense, flags):
    """Points [512 c, 512 c + 512) of row r are cleared iff flags[r][c]; everything else stays.  flags: bool (R, chunks)
    with chunks = ceil(n / 512)."""
    out = np.array(dense, dtype=bool, copy=True)
    flags = np.asarray(flags, bool)
    assert flags.shape == (out.shape[0], (out.shape[1] + CHUNK_POINTS - 1) // CHUNK_POINTS)
    for r, c in zip(*np.nonzero(flags)):
        out[r, c * CHUNK_POINTS:(c + 1) * CHUNK_POINTS] = False
    return out


def permute_bits(dense, idx):
    """out[r][o] = dense[r][idx[o]]: a gather, so len(idx) need not be n and indices may repeat."""
    return np.asarray(dense, bool)[:, np.asarray(idx, np.int64)]


def apply_row_ops(dense, ops):
    """The (opcode, dst, src) triples in list order: 0 dst &= ~src, 1 dst |= src, 2 dst = src."""
    out = np.array(dense, dtype=bool, copy=True)
    for op, d, s in np.asarray(ops, np.int64).reshape(-1, 3).tolist():
        src = out[s].copy()
        if op == ANDNOT:
            out[d] &= ~src
        elif op == OR:
            out[d] |= src
        elif op == COPY:
            out[d] = src
        else:
            raise ValueError(f"opcode {op}")
    return out


def and_rows(dense, keep):
    return np.asarray(dense, bool) & np.asarray(keep, bool)[None, :]


def gather_rows(dense, idx):
    return np.asarray(dense, bool)[np.asarray(idx, np.int64)]


# ------------------------------------------------------------------ codecs
def pack_bytes(dense_bytes):
    """uint8 / bool (R, n) -> bool (R, n): a point is set iff its byte is not 0 (2, 128, 255 count as set)."""
    return np.asarray(dense_bytes) != 0


def unpack_bytes(dense):
    """bool (R, n) -> uint8 (R, n) holding exactly 0 or 1 (the layout of torch.bool)."""
    return np.asarray(dense, bool).astype(np.uint8)


def ids_to_rows(ids, values):
    """rows[v][p] = ids[p] == values[v], compared as Python integers (all 64 bits)."""
    ids = [int(x) for x in ids]
    return np.array([[x == int(v) for x in ids] for v in values], dtype=bool).reshape(len(values), len(ids))


# ------------------------------------------------------------------ components
def component_minima(adj):
    """label[i] = smallest index of the connected component of node i of the undirected graph with an edge i -- j
    wherever adj[i][j] or adj[j][i].  Self loops change nothing: a node without edges is its own component.
    Union-find in its quick-find form: label[] always holds every node's set representative (the set's minimum), and
    joining node i with its neighbours relabels the sets involved to the smallest representative among them."""
    adj = np.asarray(adj, bool)
    n = adj.shape[0]
    label = np.arange(n, dtype=np.int64)
    for i in range(n):
        reps = np.unique(label[np.flatnonzero(adj[i] | adj[:, i])])
        reps = reps[reps != label[i]]
        if reps.size:
            m = min(int(reps.min()), int(label[i]))
            label[np.isin(label, reps) | (label == label[i])] = m
    return label


# ------------------------------------------------------------------ overlap resolution
def overlap_ops(inter, size):
    """The ordered and-not list of solve_overlapping (P:285-299): pairs i ascending, then j > i ascending, with
    inter[i][j] > 0; the loser is i unless size[i] > size[j] (ties: i loses).  -> int64 (n, 3) of (0, loser, winner)."""
    inter = np.asarray(inter)
    size = np.asarray(size, np.int64)
    i, j = np.nonzero(np.triu(inter > 0, 1))                  # row-major: i ascending, j ascending within i
    i_wins = size[i] > size[j]
    return np.stack([np.zeros_like(i), np.where(i_wins, j, i), np.where(i_wins, i, j)], axis=1).astype(np.int64)


# ------------------------------------------------------------------ groups formed on the host
def or_reduce_groups(dense, offs, members, conf=None):
    """out[g] = OR of dense[members[offs[g]:offs[g + 1]]] (an empty group: all False).  conf (float16 or float32 per
    row): also mean[g] = (((c0 + c1) + c2) ...) / len with every addition rounded to conf's dtype (P:225, Python's
    sum over 0-dim tensors), the division done in float32 and rounded to the dtype; an empty group is 0 / 0 = NaN."""
    dense = np.asarray(dense, bool)
    offs = [int(x) for x in offs]
    members = np.asarray(members, np.int64)
    k = len(offs) - 1
    out = np.zeros((k, dense.shape[1]), bool)
    mean = None if conf is None else np.zeros(k, np.asarray(conf).dtype)
    for g in range(k):
        mem = members[offs[g]:offs[g + 1]]
        for m in mem:
            out[g] |= dense[m]
        if conf is not None:
            dt = mean.dtype.type
            s = dt(0)
            for m in mem:
                s = dt(s + conf[m])
            with np.errstate(invalid="ignore", divide="ignore"):
                mean[g] = dt(np.float32(s) / np.float32(len(mem)))
    return out if conf is None else (out, mean)
