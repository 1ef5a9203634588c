"""3-D instances split into spatially connected parts, the parts that need no GPU: the NumPy statement of
tests/spatial_ref.py against hand-made cases and scipy's labelling; the config keys; the header, the binding table, the
library's exports and host-side argument checks; the tool's parser.  Every comparison is for equality."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spatial_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bff_voxel_bounds", "bff_voxel_keys", "bff_voxel_heads", "bff_voxel_ranks", "bff_voxel_neighbours",
         "bff_split_occupancy", "bff_split_union", "bff_split_count", "bff_split_emit")


def cells(*qs, c=1.0, per=1):
    """`per` points in the middle of each cell q = (q0, q1, q2)."""
    return np.repeat((np.array(qs, dtype=np.float64) + 0.5) * c, per, axis=0)


def test_forward_offsets():
    assert len(sr.FORWARD) == 13 and sr.FORWARD[0] == (0, 0, 1) and sr.FORWARD[1:4] == [(0, 1, -1), (0, 1, 0), (0, 1, 1)]
    assert sr.FORWARD[4] == (1, -1, -1) and sr.FORWARD[-1] == (1, 1, 1) and sr.FORWARD == sorted(sr.FORWARD)
    both = set(sr.FORWARD) | {(-a, -b, -c) for a, b, c in sr.FORWARD}
    assert len(both) == 26 and (0, 0, 0) not in both


def test_grid_by_hand():
    pts = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 1.0, 2.0],
                    [0.0, np.inf, 0.0], [-np.inf, 0.0, 0.0]])
    lo, vox, keys, nbr = sr.grid_ref(pts, 1.0)
    assert lo.tolist() == [0.0, 0.0, 0.0]
    assert keys.tolist() == [0, 1, (1 << 21) + (2 << 42)] and vox.tolist() == [0, 0, 1, -1, 2, -1, -1]
    assert nbr[0].tolist() == [1] + [-1] * 12                     # (0, 0, +1) on axis 0 is the first forward offset
    assert (nbr[1:] == -1).all()
    assert vox.dtype == np.int32 and keys.dtype == np.int64 and nbr.dtype == np.int32 and nbr.shape == (3, 13)
    # a corner neighbour: (d2, d1, d0) = (1, 1, 1) is the last offset, (1, -1, 1) the seventh
    _, vox, keys, nbr = sr.grid_ref(cells((0, 1, 0), (1, 2, 1), (5, 0, 5), (1, 0, 1)), 1.0)
    assert keys[vox].tolist() == [1 << 21, 1 + (2 << 21) + (1 << 42), 5 + (5 << 42), 1 + (1 << 42)]
    assert vox.tolist() == [0, 2, 3, 1] and nbr[0].tolist() == [-1] * 6 + [1] + [-1] * 5 + [2] and (nbr[1:] == -1).all()
    _, vox, _, nbr = sr.grid_ref(np.full((5, 3), np.nan), 0.1)
    assert (vox == -1).all() and nbr.shape == (0, 13)
    with pytest.raises(ValueError):
        sr.grid_ref(np.array([[0.0, 0, 0], [float(1 << 21), 0, 0]]), 1.0)


def test_boundary_floor_is_numpys():
    """Exact multiples of a cell that is no binary fraction: the statement is np.floor((x - lo) / c), nothing cleverer."""
    c = 0.1
    x = -0.7 + c * np.arange(50)
    pts = np.stack([x, np.zeros(50), np.zeros(50)], 1)
    _, vox, keys, _ = sr.grid_ref(pts, c)
    assert np.array_equal(keys[vox], np.floor((x - x.min()) / c).astype(np.int64))
    assert len(keys) < 50                                          # some multiples fall below their boundary


def test_pack_unpack():
    rng = np.random.default_rng(1)
    dense = rng.random((3, 130)) < 0.5
    rows = sr.pack(dense)
    assert rows.shape == (3, 3) and rows.dtype == np.int64 and np.array_equal(sr.unpack(rows, 130), dense)
    rows[:, 2] |= np.int64(-1) << np.int64(2)                       # garbage in the pad bits
    assert np.array_equal(sr.unpack(rows, 130), dense)


def test_adjacency_by_hand():
    one = lambda pts, row=None, **kw: sr.split_ref(pts, 1.0, sr.pack(np.ones((1, len(pts)), bool) if row is None else row),
                                                   len(pts), **kw)
    _, parent, points = one(cells((0, 0, 0), (1, 1, 1)))             # corner contact: linked
    assert parent.tolist() == [0] and points.tolist() == [2]
    rows, parent, points = one(cells((0, 0, 0), (2, 0, 0)))          # one empty cell between: not linked
    assert parent.tolist() == [0, 0] and points.tolist() == [1, 1]
    assert sr.unpack(rows, 2).tolist() == [[True, False], [False, True]]
    # the same two cells in row 0, bridged only by a cell of row 1: not linked in row 0
    pts = cells((0, 0, 0), (1, 0, 0), (2, 0, 0))
    rows, parent, points = one(pts, np.array([[1, 0, 1], [0, 1, 0]], bool))
    assert parent.tolist() == [0, 0, 1] and points.tolist() == [1, 1, 1]
    rows, parent, points = one(pts, np.array([[1, 1, 1]], bool))
    assert points.tolist() == [3]


def test_selection_by_hand():
    # cells 0 | 2,3 | 5 | 7 along x: components of 3, 4 (2 + 2), 3 and 2 points; equal sizes order by anchor
    pts = np.concatenate([cells((0, 0, 0), per=3), cells((2, 0, 0), (3, 0, 0), per=2), cells((5, 0, 0), per=3),
                          cells((7, 0, 0), per=2)])
    n = len(pts)
    rows = sr.pack(np.ones((1, n), bool))
    out, parent, points = sr.split_ref(pts, 1.0, rows, n)
    assert points.tolist() == [4, 3, 3, 2] and parent.tolist() == [0] * 4
    dense = sr.unpack(out, n)
    assert dense[1, :3].all() and dense[2, 7:10].all() and dense.sum(0).tolist() == [1] * n
    assert sr.split_ref(pts, 1.0, rows, n, min_points=3)[2].tolist() == [4, 3, 3]      # exactly min_points is kept
    assert sr.split_ref(pts, 1.0, rows, n, min_points=4)[2].tolist() == [4]            # min_points - 1 is dropped
    out, parent, points = sr.split_ref(pts[3:], 1.0, sr.pack(np.ones((1, n - 3), bool)), n - 3, min_points=5)
    assert out.shape == (0, 1) and len(parent) == 0
    tie = np.concatenate([cells((5, 0, 0), per=3), cells((0, 0, 0), per=3)])            # the later points hold the anchor
    out, _, points = sr.split_ref(tie, 1.0, sr.pack(np.ones((1, 6), bool)), 6, mode="largest")
    assert points.tolist() == [3] and sr.unpack(out, 6)[0].tolist() == [False] * 3 + [True] * 3


def blobs_cloud(seed=3):
    """The issue's random case: 3 300 points -- three blobs, a thin bridge, uniform noise -- and 6 rows."""
    rng = np.random.default_rng(seed)
    blob = lambda c, s, n: rng.normal(c, s, (n, 3))
    pts = np.concatenate([blob((0, 0, 0), 0.25, 1000), blob((2.0, 0.3, 0.1), 0.2, 1000), blob((-1.0, 2.0, 0.5), 0.3, 900),
                          np.linspace((0, 0, 0), (2.0, 0.3, 0.1), 100) + rng.normal(0, 0.01, (100, 3)),
                          rng.uniform(-2.5, 3.5, (300, 3))])
    pts = pts[rng.permutation(len(pts))]
    dense = np.stack([rng.random(len(pts)) < d for d in (0.9, 0.5, 0.2, 0.05, 0.01, 0.0)])
    return pts, dense


@pytest.mark.parametrize("cell", [0.05, 0.1, 0.3])
def test_statement_equals_scipy_label(cell):
    ndi = pytest.importorskip("scipy.ndimage")
    pts, dense = blobs_cloud()
    n = len(pts)
    assert n == 3300
    lo, vox, keys, _ = sr.grid_ref(pts, cell)
    q = np.stack([keys & (sr.AXIS - 1), (keys >> 21) & (sr.AXIS - 1), keys >> 42], 1)
    out, parent, points = sr.split_ref(pts, cell, sr.pack(dense), n)
    got = sr.unpack(out, n)
    for k in range(dense.shape[0]):
        vol = np.zeros(q.max(0) + 1, bool)
        vol[tuple(q[vox[dense[k]]].T)] = True
        lab, ncomp = ndi.label(vol, structure=np.ones((3, 3, 3)))
        mine = got[parent == k]
        assert len(mine) == ncomp
        of_point = lab[tuple(q[vox].T)]
        want = {frozenset(np.flatnonzero(dense[k] & (of_point == c)).tolist()) for c in range(1, ncomp + 1)}
        assert {frozenset(np.flatnonzero(m).tolist()) for m in mine} == want
        sizes = points[parent == k].tolist()
        assert sizes == sorted(sizes, reverse=True) and sum(sizes) == dense[k].sum()
    assert (parent == 5).sum() == 0 and (parent == 0).sum() >= 2


def test_config_keys():
    from beyond_fixed_forms_amd import spatial as sp
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    assert (DEFAULTS["split_voxel"], DEFAULTS["split_min_points"], DEFAULTS["split_mode"], DEFAULTS["split_output_dir"]) == \
        (None, 1, "split", None)
    assert sp.split_min_points(Config()) == 1 and sp.split_mode(Config()) == "split"
    cfg = Config.with_defaults(split_voxel=0.1, split_min_points=10, split_mode="largest")
    assert (sp.split_voxel(cfg), sp.split_min_points(cfg), sp.split_mode(cfg)) == (0.1, 10, "largest")
    assert sp.split_voxel(Config(split_voxel=1)) == 1.0
    for bad in (None, 0, -0.1, True, float("nan"), float("inf"), "0.1"):
        with pytest.raises(ValueError, match="split_voxel"):
            sp.split_voxel(Config(split_voxel=bad))
    with pytest.raises(ValueError, match="split_voxel"):
        sp.split_voxel(Config())
    for bad in (0, -1, 1.5, True, float("nan"), "3"):
        with pytest.raises(ValueError, match="split_min_points"):
            sp.split_min_points(Config(split_min_points=bad))
    for bad in ("dbscan", True, 1):
        with pytest.raises(ValueError, match="split_mode"):
            sp.split_mode(Config(split_mode=bad))
    text = open(os.path.join(ROOT, "configs", "config.yaml")).read()
    for key in ("split_voxel", "split_min_points", "split_mode", "split_output_dir"):
        assert re.search(rf"^# {key}:", text, re.M), key                # documented, commented out


def header_args(header, name):
    m = re.search(rf"int {name}\(([^;]*)\);", header)
    assert m, f"{name} is not declared"
    from beyond_fixed_forms_amd import _lib
    kinds, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        kinds.append(_lib._P if "*" in arg else {"int64_t": _lib._L, "int32_t": _lib._I, "double": _lib._D,
                                                 "float": _lib._F}[arg.split()[0]])
    return kinds, names


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name in NAMES:
        kinds, names = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
        assert names[-1] == "stream"
    _, names = header_args(header, "bff_voxel_keys")
    assert names[3:6] == ["lo_host", "hi_host", "cell"]
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bspatial\.hip\b", makefile, re.M)
    assert re.search(r"^_obj/.*spatial\.o.*:.*rows\.h", makefile, re.M)


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU."""
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION
    N = None
    # (points, n_points, stride, box, stream)
    assert lib.bff_voxel_bounds(N, 0, 3, N, N) == 0
    assert lib.bff_voxel_bounds(N, 5, 3, N, N) == -1 and b"null" in lib.bff_last_error()
    assert lib.bff_voxel_bounds(N, 5, 2, N, N) == -1 and lib.bff_voxel_bounds(N, 1 << 31, 3, N, N) == -2
    # (points, n_points, stride, lo_host, hi_host, cell, key, stream)
    box = lambda *v: ctypes.cast((ctypes.c_double * 3)(*v), ctypes.c_void_p)
    lo, hi = box(0.0, 0.0, 0.0), box(1.0, 2.0, 3.0)
    assert lib.bff_voxel_keys(N, 0, 3, N, N, 0.1, N, N) == 0
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert lib.bff_voxel_keys(N, 0, 3, N, N, bad, N, N) == -1 and b"cell" in lib.bff_last_error()
        assert lib.bff_voxel_keys(N, 5, 3, lo, hi, bad, N, N) == -1
    assert lib.bff_voxel_keys(N, 5, 3, lo, hi, 0.1, N, N) == -1 and b"null" in lib.bff_last_error()
    assert lib.bff_voxel_keys(N, 5, 3, N, N, 0.1, N, N) == -1
    assert lib.bff_voxel_keys(N, 5, 3, lo, box(1.0, 2.0, float(1 << 21)), 1.0, N, N) == -2 and b"2^21" in lib.bff_last_error()
    assert lib.bff_voxel_keys(N, 5, 3, lo, box(1.0, 2.0, float(1 << 21) - 0.5), 1.0, N, N) == -1      # q = 2^21 - 1 passes the limit
    assert lib.bff_voxel_keys(N, 5, 3, lo, box(1.0, 2.0, 1e300), 1e-300, N, N) == -2                  # (hi - lo) / c = inf
    assert lib.bff_voxel_keys(N, 5, 3, lo, box(1.0, float("nan"), 3.0), 1.0, N, N) == -1
    # (sorted_keys, n_points, head, stream); (sorted_keys, order, heads_incl, n_points, n_voxels, vox, keys, stream)
    assert lib.bff_voxel_heads(N, 0, N, N) == 0 and lib.bff_voxel_heads(N, 5, N, N) == -1
    assert lib.bff_voxel_ranks(N, N, N, 0, 0, N, N, N) == 0 and lib.bff_voxel_ranks(N, N, N, 5, 2, N, N, N) == -1
    assert lib.bff_voxel_ranks(N, N, N, 5, 6, N, N, N) == -1                                         # more cells than points
    # (keys, n_voxels, nbr, stream)
    assert lib.bff_voxel_neighbours(N, 0, N, N) == 0 and lib.bff_voxel_neighbours(N, 5, N, N) == -1
    assert lib.bff_voxel_neighbours(N, -1, N, N) == -1
    # (rows, n_rows, nw, n_points, vox, n_voxels, occ, prefix, row_total, stream)
    fn = lib.bff_split_occupancy
    assert fn(N, 0, 4, 200, N, 50, N, N, N, N) == 0 and fn(N, 3, 4, 200, N, 0, N, N, N, N) == 0
    assert fn(N, 3, 3, 200, N, 50, N, N, N, N) == -1                                                 # 200 points need 4 words
    assert fn(N, 3, 4, 200, N, 50, N, N, N, N) == -1 and b"null" in lib.bff_last_error()
    assert fn(N, 1 << 12, 4, 200, N, 1 << 19, N, N, N, N) == -2 and b"2^31" in lib.bff_last_error()   # K * V = 2^31 bits
    # (occ, prefix, elem_offs, n_rows, n_voxels, nbr, n_elems, parent, stream)
    assert lib.bff_split_union(N, N, N, 3, 50, N, 0, N, N) == 0 and lib.bff_split_union(N, N, N, 3, 50, N, 7, N, N) == -1
    assert lib.bff_split_union(N, N, N, 1 << 12, 1 << 19, N, 7, N, N) == -2
    # (rows, n_rows, nw, n_points, vox, n_voxels, occ, prefix, elem_offs, parent, n_elems, min_points, count, kept, stream)
    fn = lib.bff_split_count
    assert fn(N, 3, 4, 200, N, 50, N, N, N, N, 0, 1, N, N, N) == 0 and fn(N, 3, 4, 200, N, 50, N, N, N, N, 7, 1, N, N, N) == -1
    assert fn(N, 3, 4, 200, N, 50, N, N, N, N, 0, 0, N, N, N) == -1 and b"min_points" in lib.bff_last_error()
    # (rows, n_rows, nw, n_points, vox, n_voxels, occ, prefix, elem_offs, parent, n_elems, table, n_out, out, stream)
    fn = lib.bff_split_emit
    assert fn(N, 3, 4, 200, N, 50, N, N, N, N, 7, N, 0, N, N) == 0 and fn(N, 3, 4, 200, N, 50, N, N, N, N, 7, N, 2, N, N) == -1
    assert fn(N, 3, 3, 200, N, 50, N, N, N, N, 7, N, 2, N, N) == -1 and fn(N, -1, 4, 200, N, 50, N, N, N, N, 7, N, 2, N, N) == -1


def test_no_cpu_path():
    from beyond_fixed_forms_amd import spatial as sp
    with pytest.raises(ValueError, match="no CPU"):
        sp.voxel_grid(np.zeros((5, 3)), 0.1, device="cpu")
    with pytest.raises(ValueError, match="no CPU"):
        sp.voxel_grid(torch.zeros((5, 3), dtype=torch.float64), 0.1)
    with pytest.raises(ValueError, match="cell"):
        sp.voxel_grid(np.zeros((5, 3)), 0.0)
    grid = sp.VoxelGrid(0.1, np.zeros(3), 200, 0, None, None, None)
    with pytest.raises(ValueError, match="no CPU"):
        sp.split_rows(grid, torch.zeros((2, 4), dtype=torch.int64), 200)
    from types import SimpleNamespace
    empty = SimpleNamespace(rows=None, conf=[], final_class=[])
    assert sp.split_instances(grid, empty, {}) is empty                 # nothing to split: back as it is


def test_tool_parser_and_missing_directory(tmp_path, capsys):
    from beyond_fixed_forms_amd import cli
    args = cli._split_parser().parse_args(["--config", "c.yaml", "--cls", "office chair"])
    assert (args.config, args.cls, args.stage) == ("c.yaml", "office chair", "final")
    assert cli._split_parser().parse_args(["--config", "c", "--cls", "x", "--stage", "mask_3d"]).stage == "mask_3d"
    with pytest.raises(SystemExit):
        cli._split_parser().parse_args(["--config", "c", "--cls", "x", "--stage", "stage1"])
    cfg = tmp_path / "config.yaml"
    cfg.write_text(f"final_output_dir: {tmp_path}/final\nmask_3d_dir: {tmp_path}/mask_3d\nsplit_output_dir: {tmp_path}/split\n"
                   "split_voxel: 0.1\n")
    assert cli.split_main(["--config", str(cfg), "--cls", "table"]) == 1
    assert "not a directory" in capsys.readouterr().err
    tool = open(os.path.join(ROOT, "tools", "split_instances_3d.py")).read()
    assert "split_main" in tool
