"""Hand-built inputs of the density clustering, shared by the host tests (the statement by hand)
and the GPU tests (the device against the statement).  Every coordinate is a binary fraction: differences, squares and
sums of a distance are exact, so "at exactly eps" means it."""
import numpy as np

from density_ref import pack

EPS = 0.25


def all_set(n, k=1):
    return pack(np.ones((k, n), bool))


def line(*xs):
    return np.array([[x, 0.0, 0.0] for x in xs])


def exact_boundary():
    """A(0), B(eps) are neighbours: d2 == eps^2.  C(-nextafter(eps, 1)) is not A's: d2 rounds to eps^2 + 2^-55."""
    return line(0.0, EPS, -np.nextafter(EPS, 1.0))


def two_clusters(tie):
    """min_samples = 5.  Two cores of four duplicates each with one more core point beside them, P_A and P_B, and a point
    X between those that only has X, P_A and P_B within eps: a border point.
    tie: X is equidistant from P_A (index 9) and P_B (index 8): it follows the smaller index, P_B, into the cluster with
    the larger anchor.  -> (points, index of X, anchor of X's cluster).
    not tie: P_A (index 4) is X's lowest-indexed core neighbour at d = eps, P_B (index 9) its nearest at d = eps / 2: it
    joins P_B's cluster, where a traversal in index order reaches it from P_A's first."""
    if tie:                                                                  # A at 0, P_A 0.25, X 0.5, P_B 0.75, B at 1
        return line(0, 0, 0, 0, 1, 1, 1, 1, 0.75, 0.25, 0.5), 10, 4
    return line(0, 0, 0, 0, 0.25, 0.875, 0.875, 0.875, 0.875, 0.625, 0.5), 10, 5


def all_directions():
    """27 points on a 3 x 3 x 3 lattice of step 9/64 around (1, 1, 1) -- every one within eps of the centre, sqrt(3) * 9/64
    = 0.2436 -- and a far corner at 0.625 that puts the grid's origin 1.5 cells below the centre: the 27 sit in 27
    different cells, the corners of the lattice in the grid's first and last cell on every axis.  -> (points, the
    centre's index).  With min_samples = 27 the centre is the only core point, and only if all 26 are found."""
    d = 9.0 / 64
    pts = [[1 + d * i, 1 + d * j, 1 + d * k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    return np.array(pts + [[0.625, 0.625, 0.625]]), 13


def chain(n=2000):
    """n points spaced exactly eps apart on a line, in a shuffled index order: one cluster at min_samples <= 2."""
    rng = np.random.default_rng(5)
    return line(*(EPS * rng.permutation(n)))


def duplicates(n=200):
    """n copies of one point (more than a wave in one cell), a neighbour at eps / 2 and a far point."""
    return np.concatenate([np.full((n, 3), 0.5), [[0.625, 0.5, 0.5]], [[3.0, 3.0, 3.0]]])


def five_groups():
    """70 points (two words a row) in six groups of (14, 10, 12, 12, 12, 10) points: a group sits within eps / 2 of its
    centre and the centres are 4 apart, so at eps or at a cell of EPS a group is one part and no two groups touch.  The
    point order is shuffled: every group has points in both words.  Row 0 holds the first five groups -- five kept parts,
    three of them tied in points -- and row 1 the sixth.  -> (points, rows int64 [2][2])."""
    rng = np.random.default_rng(9)
    sizes = (14, 10, 12, 12, 12, 10)
    group = np.repeat(np.arange(6), sizes)
    pts = np.array([[4.0 * g, 0.0, 0.0] for g in group]) + rng.integers(0, 8, (70, 3)) / 64.0
    perm = rng.permutation(70)
    pts, group = pts[perm], group[perm]
    return pts, pack(np.stack([group < 5, group == 5]))


def garbage(rows, n):
    """The rows with a spare word, every bit at a position >= n set."""
    rows = np.concatenate([rows, np.zeros((rows.shape[0], 1), np.int64)], axis=1)
    if n % 64:
        rows[:, n // 64] |= np.int64(-1) << np.int64(n % 64)
    rows[:, (n + 63) // 64:] = -1
    return rows


def random_rows(n, sizes, seed):
    rng = np.random.default_rng(seed)
    dense = np.zeros((len(sizes), n), bool)
    for k, m in enumerate(sizes):
        dense[k, rng.choice(n, m, replace=False)] = True
    return pack(dense)
