"""3-D instances split into spatially connected parts on the GPU: the voxel grid (bff_voxel_*) and the split
(bff_split_*) against their NumPy statement (tests/spatial_ref.py), spatial.split_instances and the command-line tool
against the same.  Everything is compared for equality."""
import functools
import os

import numpy as np
import pytest
import torch

import density_cases as dc
import spatial_ref as sr
import test_spatial_host as th

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# what one step of the implementation covers: the prefix wave scans 64 occ words (4096 cells) a step, a block of the
# union kernel owns 256 occ words (16384 cells), a block of the element kernels 256 elements
BIG_CELLS = 16384


@pytest.fixture(scope="module")
def sp():
    from beyond_fixed_forms_amd import _lib, spatial
    _lib.load()
    assert torch.cuda.is_available()
    return spatial


def dev_rows(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(DEV)


def check_grid(sp, pts, cell):
    lo, vox, keys, nbr = sr.grid_ref(pts, cell)
    g = sp.voxel_grid(pts, cell, DEV)
    assert (g.n_points, g.n_voxels, g.cell) == (len(pts), len(keys), cell)
    assert g.vox.dtype == torch.int32 and g.keys.dtype == torch.int64 and g.nbr.dtype == torch.int32
    assert np.array_equal(g.vox.cpu().numpy(), vox) and np.array_equal(g.keys.cpu().numpy(), keys)
    assert tuple(g.nbr.shape) == (len(keys), 13) and np.array_equal(g.nbr.cpu().numpy(), nbr)
    assert np.array_equal(g.lo, lo, equal_nan=True)
    return g, vox, keys, nbr


def check_split(sp, pts, cell, rows, min_points=1, mode="split", grid=None):
    """rows: int64 [K][nw] (NumPy).  The device's rows, parent and points against the statement's; -> the statement's."""
    n = len(pts)
    exp = sr.split_ref(pts, cell, rows, n, min_points, mode)
    grid = grid or sp.voxel_grid(pts, cell, DEV)
    out, parent, points = sp.split_rows(grid, dev_rows(rows), n, min_points, mode)
    assert out.dtype == torch.int64 and out.is_cuda and parent.dtype == points.dtype == torch.int64
    assert tuple(out.shape) == exp[0].shape
    assert np.array_equal(parent.numpy(), exp[1]) and np.array_equal(points.numpy(), exp[2])
    assert np.array_equal(out.cpu().numpy(), exp[0])
    return exp


# ------------------------------------------------------------------ the grid
def grid_cloud():
    """N = 1000 (15.6 words): coordinates on both sides of zero, exact multiples of 0.1 from lo, one NaN, +inf, -inf point."""
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.3, 1.1, (1000, 3))
    pts[0] = (-1.5, -1.5, -1.5)                                          # lo
    k = rng.integers(0, 30, (300, 3))
    pts[1:301] = pts[0] + 0.1 * k                                        # on cell boundaries, as computed in float64
    pts[400] = (np.nan, 0.0, 0.0)
    pts[500] = (0.0, np.inf, 0.0)
    pts[999] = (0.0, 0.0, -np.inf)
    return pts


def test_grid_equals_numpy(sp):
    pts = grid_cloud()
    _, vox, keys, nbr = check_grid(sp, pts, 0.1)
    assert (vox == -1).sum() == 3 and vox[0] == 0 and len(keys) > 500
    assert (nbr >= 0).any() and (nbr[0] == -1).sum() >= 6                # the corner cell: its q - 1 faces leave the grid
    check_grid(sp, pts[:, [2, 0, 1]], 0.25)
    check_grid(sp, np.concatenate([pts, np.ones((1000, 3))], 1), 0.1)    # the (N, 6) array of <scene>.npy


def test_grid_one_cell_and_large_cell(sp):
    rng = np.random.default_rng(8)
    pts = rng.uniform(0.0, 0.09, (130, 3))
    _, vox, keys, nbr = check_grid(sp, pts, 0.1)                         # all points in one cell
    assert len(keys) == 1 and (vox == 0).all() and (nbr == -1).all()
    _, _, keys, _ = check_grid(sp, grid_cloud(), 50.0)                   # a cell larger than the scene
    assert len(keys) == 1
    g, _, _, _ = check_grid(sp, np.full((70, 3), np.nan), 0.1)           # no finite point at all
    assert g.n_voxels == 0
    g = sp.voxel_grid(np.zeros((0, 3)), 0.1, DEV)
    assert (g.n_points, g.n_voxels) == (0, 0)
    with pytest.raises(RuntimeError, match="2\\^21"):
        sp.voxel_grid(np.array([[0.0, 0, 0], [3.0e6, 0, 0]]), 1.0, DEV)
    dev_pts = torch.from_numpy(grid_cloud()).to(DEV)
    assert torch.equal(sp.voxel_grid(dev_pts, 0.1).vox, sp.voxel_grid(grid_cloud(), 0.1, DEV).vox)


# ------------------------------------------------------------------ adjacency
def test_adjacency(sp):
    full = lambda n: sr.pack(np.ones((1, n), bool))
    assert check_split(sp, th.cells((0, 0, 0), (1, 1, 1)), 1.0, full(2))[2].tolist() == [2]            # corner: linked
    assert check_split(sp, th.cells((0, 0, 0), (2, 0, 0)), 1.0, full(2))[2].tolist() == [1, 1]         # a gap: not linked
    pts = th.cells((0, 0, 0), (1, 0, 0), (2, 0, 0))
    exp = check_split(sp, pts, 1.0, sr.pack(np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1]], bool)))        # bridged by row 1 only
    assert exp[1].tolist() == [0, 0, 1, 2] and exp[2].tolist() == [1, 1, 1, 3]


# ------------------------------------------------------------------ rows
def test_row_edge_cases(sp):
    pts, _ = th.blobs_cloud(5)
    pts = pts[:1000]
    n, nw = 1000, 16
    grid = sp.voxel_grid(pts, 0.2, DEV)
    out, parent, points = sp.split_rows(grid, torch.zeros((0, nw), dtype=torch.int64, device=DEV), n)  # K = 0
    assert tuple(out.shape) == (0, nw) and len(parent) == 0 and len(points) == 0
    g0 = sp.voxel_grid(np.zeros((0, 3)), 0.2, DEV)                                                      # N = 0
    out, parent, _ = sp.split_rows(g0, torch.zeros((3, 0), dtype=torch.int64, device=DEV), 0)
    assert tuple(out.shape) == (0, 0) and len(parent) == 0
    dense = np.zeros((4, n), bool)
    dense[1] = True                                                      # rows: all zero, full, one point, all zero
    dense[2, 777] = True
    rows = sr.pack(dense)
    exp = check_split(sp, pts, 0.2, rows, grid=grid)
    assert set(exp[1].tolist()) == {1, 2} and exp[2][-1] == 1
    rows[:, -1] |= np.int64(-1) << np.int64(n - 64 * (nw - 1))           # garbage in the pad bits of the last word
    garbage = check_split(sp, pts, 0.2, rows, grid=grid)
    assert all(np.array_equal(a, b) for a, b in zip(exp, garbage))
    wide = np.concatenate([rows, np.full((4, 2), -1, np.int64)], 1)      # and in whole words past the cloud
    assert np.array_equal(check_split(sp, pts, 0.2, wide, grid=grid)[0][:, :nw], exp[0])
    assert check_split(sp, pts, 0.2, sr.pack(np.zeros((2, n), bool)), grid=grid)[0].shape == (0, nw)


def test_seventy_rows(sp):
    pts, _ = th.blobs_cloud(6)
    pts = pts[:1500]
    rng = np.random.default_rng(70)
    dense = rng.random((70, 1500)) < np.linspace(0.0, 0.6, 70)[:, None]
    exp = check_split(sp, pts, 0.15, sr.pack(dense), min_points=2)
    assert exp[1].max() == 69 and len(exp[1]) > 140


# ------------------------------------------------------------------ union-find depth
def spiral(n_cells):
    """A one-cell-wide square spiral in the plane z = 0, one empty cell between its arms (arms of 2, 2, 4, 4, 6, ... cells)."""
    x = y = 0
    out = [(0, 0, 0)]
    step, d = 2, 0
    while len(out) < n_cells:
        for _ in range(2):
            dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d % 4]
            for _ in range(step):
                x, y = x + dx, y + dy
                out.append((x, y, 0))
            d += 1
        step += 2
    return out


def test_spiral_snake(sp):
    path = spiral(320)
    assert len(path) >= 300 and len(set(path)) == len(path)
    rng = np.random.default_rng(11)
    pts = th.cells(*path, c=0.5, per=2)
    pts = pts[rng.permutation(len(pts))]
    n = len(pts)
    dense = np.ones((2, n), bool)
    cut = np.all(pts == (np.array(path[150]) + 0.5) * 0.5, axis=1)       # row 1: the snake without one of its cells
    dense[1, cut] = False
    exp = check_split(sp, pts, 0.5, sr.pack(dense))
    assert exp[1].tolist() == [0, 1, 1] and exp[2].tolist() == [n, n - 2 - 2 * 150, 2 * 150]


def test_two_blobs_and_a_bridge(sp):
    rng = np.random.default_rng(12)
    a, b = rng.uniform(0.0, 1.0, (400, 3)), rng.uniform(0.0, 1.0, (400, 3)) + (1.3, 0.0, 0.0)
    bridge = np.array([[1.1, 0.5, 0.5]])                                 # cell 5 on x at c = 0.2: the blobs end at 4, start at 6
    pts = np.concatenate([a, b, bridge])
    dense = np.ones((2, 801), bool)
    dense[1, 800] = False
    exp = check_split(sp, pts, 0.2, sr.pack(dense))
    assert exp[1].tolist()[:1] == [0] and exp[2][0] > 700 and (exp[1] == 1).sum() >= 2


def test_more_cells_than_one_block_covers(sp):
    """V > 16 384 = BIG_CELLS: the prefix wave takes several steps, the union kernel several blocks, T several element blocks."""
    rng = np.random.default_rng(13)
    pts = rng.uniform(0.0, 1.0, (40000, 3)) * (48, 48, 12)
    dense = np.stack([np.ones(40000, bool), rng.random(40000) < 0.25])
    grid = sp.voxel_grid(pts, 1.0, DEV)
    assert grid.n_voxels > BIG_CELLS
    exp = check_split(sp, pts, 1.0, sr.pack(dense), min_points=3, grid=grid)
    assert (exp[1] == 0).sum() >= 1 and (exp[1] == 1).sum() >= 1 and exp[2][0] > 30000


# ------------------------------------------------------------------ selection
def test_selection(sp):
    pts = np.concatenate([th.cells((0, 0, 0), per=3), th.cells((2, 0, 0), (3, 0, 0), per=2), th.cells((5, 0, 0), per=3),
                          th.cells((7, 0, 0), per=2), [[np.nan, 0.0, 0.0]]])
    n = len(pts)
    rows = sr.pack(np.ones((2, n), bool))
    grid = sp.voxel_grid(pts, 1.0, DEV)
    exp = check_split(sp, pts, 1.0, rows, grid=grid)
    assert exp[2].tolist() == [4, 3, 3, 2] * 2
    kids = sr.unpack(exp[0], n)
    assert kids[1, :3].all() and kids[2, 7:10].all()                     # equal sizes: the smaller anchor first
    finite = np.isfinite(pts).all(1)
    for k in range(2):                                                   # min_points = 1: the OR of the children
        assert np.array_equal(kids[exp[1] == k].any(0), finite) and (kids[exp[1] == k].sum(0) <= 1).all()
    assert check_split(sp, pts, 1.0, rows, 3, grid=grid)[2].tolist() == [4, 3, 3] * 2       # exactly min_points: kept
    assert check_split(sp, pts, 1.0, rows, 4, grid=grid)[2].tolist() == [4] * 2             # min_points - 1: dropped
    assert check_split(sp, pts, 1.0, rows, 5, grid=grid)[0].shape[0] == 0
    assert check_split(sp, pts, 1.0, rows, 1, "largest", grid=grid)[2].tolist() == [4, 4]
    tie = np.concatenate([th.cells((5, 0, 0), per=3), th.cells((0, 0, 0), per=3)])
    exp = check_split(sp, tie, 1.0, sr.pack(np.ones((1, 6), bool)), 1, "largest")
    assert sr.unpack(exp[0], 6)[0].tolist() == [False] * 3 + [True] * 3
    with pytest.raises(ValueError, match="mode"):
        sp.split_rows(grid, dev_rows(rows), n, 1, "dbscan")
    with pytest.raises(ValueError, match="min_points"):
        sp.split_rows(grid, dev_rows(rows), n, 0)


@pytest.mark.parametrize("mode", ["split", "largest"])
def test_more_kept_parts_than_the_first_read_fetches(sp, monkeypatch, mode):
    """Six kept parts, five of them in row 0, against a first read of two: the rest comes with the overflow fetch, and the
    result is the statement's and the one of a first read that holds them all."""
    from beyond_fixed_forms_amd import instances3d
    pts, rows = dc.five_groups()
    grid = sp.voxel_grid(pts, dc.EPS, DEV)
    whole = [t.cpu() for t in sp.split_rows(grid, dev_rows(rows), 70, 1, mode)]
    monkeypatch.setattr(instances3d, "KEPT_FIRST_READ", 2)
    exp = check_split(sp, pts, dc.EPS, rows, 1, mode, grid=grid)
    assert exp[2].tolist() == ([14, 12, 12, 12, 10, 10] if mode == "split" else [14, 10]) and exp[1].tolist()[-1] == 1
    again = [t.cpu() for t in sp.split_rows(grid, dev_rows(rows), 70, 1, mode)]
    assert all(torch.equal(a, b) for a, b in zip(whole, again))


# ------------------------------------------------------------------ the random case
@functools.lru_cache(maxsize=None)
def blobs():
    pts, dense = th.blobs_cloud()
    return pts, sr.pack(dense)


@pytest.mark.parametrize("cell", [0.05, 0.1, 0.3])
def test_random_blobs(sp, cell):
    pts, rows = blobs()
    exp = check_split(sp, pts, cell, rows, min_points=10)
    assert len(exp[1]) >= 3 and 5 not in exp[1]
    check_split(sp, pts, cell, rows, min_points=10, mode="largest")


def test_two_calls_give_equal_outputs(sp):
    pts, rows = blobs()
    grid = sp.voxel_grid(pts, 0.1, DEV)
    again = sp.voxel_grid(pts, 0.1, DEV)
    assert torch.equal(grid.vox, again.vox) and torch.equal(grid.keys, again.keys) and torch.equal(grid.nbr, again.nbr)
    a = sp.split_rows(grid, dev_rows(rows), len(pts), 2)
    b = sp.split_rows(grid, dev_rows(rows), len(pts), 2)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape[0] > 6


# ------------------------------------------------------------------ the wrapper and the tool
@functools.lru_cache(maxsize=None)
def tiny_result():
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import project_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=11)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height, split_voxel=0.1, split_min_points=2)
    return scene, cfg, project_scene(scene, cfg, device=DEV, return_result=True)


def test_split_instances(sp):
    scene, cfg, res = tiny_result()
    n = scene.points.shape[0]
    grid = sp.voxel_grid_for(scene, cfg, DEV)
    assert grid.n_points == n and grid.cell == 0.1
    from beyond_fixed_forms_amd.scene import prepare_scene
    resident = sp.voxel_grid_for(prepare_scene(scene, cfg, device=DEV), cfg)        # the sorted cloud, put back in order
    assert torch.equal(resident.vox, grid.vox) and torch.equal(resident.keys, grid.keys) and torch.equal(resident.nbr, grid.nbr)
    rows = res.rows.cpu().numpy()
    exp = sr.split_ref(scene.points, 0.1, rows, n, 2)
    got = sp.split_instances(grid, res, cfg)
    assert type(got) is type(res) and got is not res and res.rows.shape[0] == rows.shape[0]
    assert np.array_equal(got.rows.cpu().numpy(), exp[0]) and np.array_equal(got.parent.numpy(), exp[1])
    assert got.conf.dtype == res.conf.dtype and got.conf.device == res.conf.device
    assert torch.equal(got.conf.cpu(), res.conf.cpu()[torch.from_numpy(exp[1])])
    assert got.final_class == [res.final_class[i] for i in exp[1].tolist()] and len(exp[1]) >= 1
    d = got.to_dict()
    assert tuple(d["ins"].shape) == (len(exp[1]), n) and np.array_equal(d["ins"].cpu().numpy(), sr.unpack(exp[0], n))
    from types import SimpleNamespace
    listed = SimpleNamespace(rows=res.rows, conf=[float(c) for c in res.conf.cpu()], final_class=list(res.final_class))
    got = sp.split_instances(grid, listed, dict(cfg, split_mode="largest"))
    largest = sr.split_ref(scene.points, 0.1, rows, n, 2, "largest")
    assert isinstance(got.conf, list) and got.conf == [listed.conf[i] for i in largest[1].tolist()]
    assert np.array_equal(got.rows.cpu().numpy(), largest[0])


@pytest.mark.parametrize("stage", ["final", "mask_3d"])
def test_tool(sp, tmp_path, stage, monkeypatch):
    import yaml
    from beyond_fixed_forms_amd import cli
    from beyond_fixed_forms_amd.config import Config
    from oracle import rle_ref
    scene, _, res = tiny_result()
    n, cls = scene.points.shape[0], "table"
    rows = res.rows.cpu().numpy()
    dense = sr.unpack(rows, n)
    dirs = {"final": tmp_path / "final", "mask_3d": tmp_path / "m3d"}
    (dirs[stage] / cls).mkdir(parents=True)
    (tmp_path / "npy").mkdir()
    conf = torch.linspace(0.3, 0.8, len(dense)).to(torch.float16)
    saved = {"ins": torch.from_numpy(dense), "conf": conf, "final_class": [f"thing {i}" for i in range(len(dense))]}
    for name in ("scene_a", "scene_empty"):
        np.save(tmp_path / "npy" / f"{name}.npy", scene.points)
    torch.save(saved, dirs[stage] / cls / "scene_a.pth")
    torch.save({"ins": [], "conf": [], "final_class": []}, dirs[stage] / cls / "scene_empty.pth")      # the list-valued empty form
    cfg = Config.with_defaults(scene_npy_dir=str(tmp_path / "npy"), final_output_dir=str(dirs["final"]),
                               mask_3d_dir=str(dirs["mask_3d"]), split_output_dir=str(tmp_path / "split"), split_voxel=0.1,
                               split_min_points=2)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    argv = ["--config", str(tmp_path / "config.yaml"), "--cls", cls, "--stage", stage]
    monkeypatch.delenv("BFF_SAVE_RLE", raising=False)
    assert cli.split_main(argv) == 0
    exp = sr.split_ref(scene.points, 0.1, rows, n, 2)
    out = torch.load(tmp_path / "split" / cls / "scene_a.pth", weights_only=False)
    assert out["ins"].dtype == torch.bool and not out["ins"].is_cuda and np.array_equal(out["ins"].numpy(), sr.unpack(exp[0], n))
    assert np.array_equal(out["parent"].numpy(), exp[1]) and out["conf"].dtype == torch.float16
    assert torch.equal(out["conf"], conf[torch.from_numpy(exp[1])])
    assert out["final_class"] == [f"thing {i}" for i in exp[1].tolist()]
    empty = torch.load(tmp_path / "split" / cls / "scene_empty.pth", weights_only=False)
    assert empty == {"ins": [], "conf": [], "final_class": []}
    monkeypatch.setenv("BFF_SAVE_RLE", "1")
    assert cli.split_main(argv) == 0
    out = torch.load(tmp_path / "split" / cls / "scene_a.pth", weights_only=False)
    assert isinstance(out["ins"], list) and np.array_equal(rle_ref.rle_decode_batch_ref(out["ins"]).bool().numpy(),
                                                           sr.unpack(exp[0], n))
    other = "mask_3d" if stage == "final" else "final"
    assert cli.split_main(argv[:-1] + [other]) == 1                      # that stage has no directory for the class
