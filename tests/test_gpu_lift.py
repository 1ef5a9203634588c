"""3-D instances lifted from a subsampled cloud to the full cloud on the GPU: lift.subsample, the search (bff_nn_search),
the many-row bit gather (bff_rows_to_columns, bff_lift_bits), lift_instances and the two command-line tools against their
NumPy statement (tests/lift_ref.py).  Everything is compared for equality, the squared distances bit for bit."""
import dataclasses
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lift_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 0.125
STEP = 2.0 ** -6                  # the lattice: every difference, square and sum of a distance is exact
SEARCH_BLOCK = 256                # queries per block of the search kernel


@pytest.fixture(scope="module")
def lift():
    from beyond_fixed_forms_amd import _lib, lift
    _lib.load()
    assert torch.cuda.is_available()
    return lift


def dev_rows(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(DEV)


def check_search(lift, src, radius, qs, index=None):
    """The device's nn and d2 against the 27-cell statement's; -> the statement's."""
    exp_nn, exp_d2 = lr.nearest_ref(src, radius, qs)
    index = lift.nearest_index(src, radius, DEV) if index is None else index
    nn, d2 = lift.nearest(index, qs, return_d2=True)
    assert nn.dtype == torch.int32 and d2.dtype == torch.float64 and nn.is_cuda and d2.is_cuda
    assert tuple(nn.shape) == tuple(d2.shape) == (len(qs),)
    assert np.array_equal(nn.cpu().numpy(), exp_nn)
    assert np.array_equal(d2.cpu().numpy().view(np.int64), exp_d2.view(np.int64))      # bit for bit, +inf included
    assert torch.equal(lift.nearest(index, qs), nn)                          # without d2: the same nn
    return exp_nn, exp_d2


# ------------------------------------------------------------------ the search
@functools.lru_cache(maxsize=None)
def search_case(m):
    """M sources on the three planes (random floats), 5000 queries: random floats on the planes, then lattice points."""
    src = lr.three_planes(1300, seed=11)[:m]
    qs = np.concatenate([lr.three_planes(4000, seed=12), lr.three_planes(1000, lattice=True, seed=13)])
    rng = np.random.default_rng(14)
    qs = qs[rng.permutation(len(qs))]
    return src, qs, lr.nearest_ref(src, V, qs)


@pytest.mark.parametrize("m", [0, 1, 1300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_search_sizes(lift, n, m):
    src, qs, (exp_nn, exp_d2) = search_case(m)
    index = lift.nearest_index(src, V, DEV)
    assert index.n_source == m and tuple(index.cloud.shape) == (m, 3) and index.offs.shape[0] == index.grid.n_voxels + 1
    nn, d2 = lift.nearest(index, qs[:n], return_d2=True)
    assert np.array_equal(nn.cpu().numpy(), exp_nn[:n])
    assert np.array_equal(d2.cpu().numpy().view(np.int64), exp_d2[:n].view(np.int64))
    if m == 1300 and n == 5000:
        assert n > SEARCH_BLOCK and (exp_nn >= 0).sum() > 1000 and (exp_nn < 0).sum() > 10
    if m == 0:
        assert (exp_nn == -1).all()


def test_search_random_floats_and_query_kinds(lift):
    """Non-lattice floats against the 27-cell statement at two radii; the queries as an array of 6 columns, as a device
    tensor with a stride of 6, and an empty query set."""
    src = lr.three_planes(1300, seed=21)
    qs = lr.three_planes(700, seed=22)
    for radius in (V, 0.3):
        check_search(lift, src, radius, qs)
    index = lift.nearest_index(src, V, DEV)
    six = np.concatenate([qs, np.full((len(qs), 3), 7.0)], axis=1)
    want = lift.nearest(index, qs)
    assert torch.equal(lift.nearest(index, six), want)
    assert torch.equal(lift.nearest(index, torch.from_numpy(six).to(DEV)), want)
    nn, d2 = lift.nearest(index, np.zeros((0, 3)), return_d2=True)
    assert tuple(nn.shape) == tuple(d2.shape) == (0,)
    again = lift.nearest_index(torch.from_numpy(src).to(DEV), V)             # a device cloud: the same index
    assert all(torch.equal(getattr(again, f), getattr(index, f)) for f in ("order", "offs", "cloud"))
    with pytest.raises(ValueError, match="no CPU"):
        lift.nearest(index, torch.from_numpy(qs))


def test_search_self_and_subsample(lift):
    """Queries that equal a source point; nn[sample[j]] == j; nobody without a source at r = 2 v, some at r = v."""
    for lattice in (False, True):
        pts = lr.three_planes(3000, lattice)
        sample = lift.subsample(pts, V, DEV)
        assert sample.dtype == torch.int32 and sample.is_cuda
        s = sample.cpu().numpy()
        assert np.array_equal(s, lr.subsample_ref(pts, V))
        near, _ = check_search(lift, pts[s], V, pts)
        far, d_far = check_search(lift, pts[s], 2 * V, pts)
        assert np.array_equal(far[s], np.arange(len(s))) and np.array_equal(near[s], np.arange(len(s)))
        assert (d_far[s] == 0).all() and (far >= 0).all() and 0 < (near < 0).sum() < 100


def test_search_ties_duplicates_and_the_radius(lift):
    r = 8 * STEP                                                             # cells of 0.125 from lo = (0, 0, 0)
    c = lambda *v: [x * STEP for x in v]
    src = np.array([c(0, 0, 0),
                    c(10, 2, 2), c(14, 2, 2),                               # 1, 2: equidistant from (12, 2, 2) in one cell
                    c(20, 20, 20), c(28, 20, 20),                           # 3, 4: equidistant from (24, 20, 20), cells 2 and 3
                    c(40, 40, 40), c(40, 40, 40), c(40, 40, 40),            # 5, 6, 7: duplicates
                    c(60, 60, 68), c(60, 60, 52),                           # 9 before 8 in key order: the tie still goes to 8
                    c(100, 100, 100)])
    qs = np.array([c(12, 2, 2), c(24, 20, 20), c(40, 40, 40), c(41, 40, 40), c(60, 60, 60),
                   c(100, 100, 108), c(100, 100, 109), c(100, 108, 100), c(108, 100, 100), c(109, 100, 100),
                   c(100 + 5, 100 + 5, 100 + 4), c(100 + 5, 100 + 5, 100 + 3), c(100 + 5, 100 + 5, 100 + 5)])
    nn, d2 = check_search(lift, src, r, qs)
    assert nn.tolist() == [1, 3, 5, 5, 8, 10, -1, 10, 10, -1, -1, 10, -1]
    assert d2[5] == r * r and d2[4] == r * r and d2[11] == 59 * STEP * STEP and d2[10] == np.inf      # 66 > 64 >= 59
    flipped = src[::-1].copy()                                               # the same cloud in the opposite index order
    back, _ = check_search(lift, flipped, r, qs)
    assert back.tolist() == [8, 6, 3, 3, 1, 0, -1, 0, 0, -1, -1, 0, -1]


def test_search_outside_the_box_and_non_finite(lift):
    r = 1.0
    src = np.array([[0.0, 0.0, 0.0], [1.5, 0.5, 0.5], [0.5, 0.5, 0.5], [3.0, 3.0, 3.0], [3.0, 3.0, 3.0],
                    [np.nan, 0.0, 0.0], [2.0, 0.0, np.inf], [-np.inf, 1.0, 1.0]])
    qs = np.array([[1.0, 0.5, 0.5], [3.0, 3.0, 3.0], [3.0, 3.0, 4.0], [3.0, 3.0, 4.0 + 2.0 ** -40], [-0.5, 0.0, 0.0],
                   [-1.0, 0.0, 0.0], [-1.0 - 2.0 ** -40, 0.0, 0.0], [-1.5, 0.0, 0.0], [0.0, -0.5, -0.5], [3.5, 3.5, 3.5],
                   [4.0, 3.0, 3.0], [4.5, 3.0, 3.0], [5.5, 3.0, 3.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf],
                   [1e300, 0.0, 0.0], [-1e300, 0.0, 0.0], [0.0, 1e300, 0.0], [0.0, 0.0, -1e300], [2.0, 0.0, 0.5],
                   [2.0, 2.0, 2.0], [1.5, 2.5, 0.5], [2.0 ** 22, 0.0, 0.0], [-2.0 ** 22, 0.0, 0.0]])
    nn, d2 = check_search(lift, src, r, qs)
    assert nn.tolist() == [1, 3, 3, -1, 0, 0, -1, -1, 0, 3, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, 1, -1, -1, -1, -1]
    assert not np.isin(nn, [5, 6, 7]).any()                                 # a non-finite source is never returned
    assert d2[2] == 1.0 and d2[5] == 1.0 and d2[9] == 0.75 and np.isinf(d2[21])      # query 21: its own cell is empty
    bn, bd = lr.brute_ref(src, r, qs)
    assert np.array_equal(nn, bn) and np.array_equal(d2, bd)
    only_bad = src[5:]                                                       # no finite source: no grid, everybody -1
    nn, _ = check_search(lift, only_bad, r, qs)
    assert (nn == -1).all()


def test_search_a_crowded_cell(lift):
    """One cell of 300 sources (more than a wave), duplicates among them, beside sparse ones; lattice queries around it."""
    rng = np.random.default_rng(31)
    crowd = (rng.integers(0, 8, (300, 3)) + 16) * STEP                       # 512 lattice sites for 300 points: duplicates
    sparse = rng.integers(0, 64, (60, 3)) * STEP
    src = np.concatenate([sparse[:30], crowd, sparse[30:]])
    src[0] = 0.0                                                             # lo = (0, 0, 0): the crowd is cell (2, 2, 2)
    qs = np.concatenate([rng.integers(6, 34, (400, 3)), rng.integers(-8, 72, (200, 3))]) * STEP      # around it, and all over
    nn, d2 = check_search(lift, src, 8 * STEP, qs)
    _, cells = lr.grid_ref(src, 8 * STEP)
    assert len(cells[(2, 2, 2)]) >= 300 and len(np.unique(crowd, axis=0)) < 300
    assert ((nn >= 30) & (nn < 330)).sum() > 50 and (nn < 0).sum() > 0
    bn, bd = lr.brute_ref(src, 8 * STEP, qs)                                 # exact arithmetic: the grid changes nothing
    assert np.array_equal(nn, bn) and np.array_equal(d2, bd)


# ------------------------------------------------------------------ the bit gather
def lift_case(k, m, n, seed=0, holes=True):
    """K rows over M sources with garbage in the padding, one spare word included; an nn with -1, repeats and values out
    of range."""
    rng = np.random.default_rng(100 + seed)
    dense = rng.random((k, m)) < rng.random((k, 1))
    rows = lr.pack(dense, (m + 63) // 64 + 1)
    if m % 64:
        rows[:, m // 64] |= np.int64(-1) << np.int64(m % 64)
    rows[:, (m + 63) // 64:] = -1
    nn = rng.integers(0, max(m, 1), n).astype(np.int32) if m else np.full(n, -1, np.int32)
    nn[rng.random(n) < 0.3] = nn[0]                                          # many targets on one source
    if holes:
        bad = np.array([-1, -1, -1, m, m + 5, -2, 2 ** 31 - 1, -2 ** 31, 64 * rows.shape[1]], dtype=np.int64)
        where = rng.random(n) < 0.25
        nn[where] = bad[rng.integers(0, len(bad), int(where.sum()))].astype(np.int32)
    return rows, nn


@pytest.mark.parametrize("m,n", [(128, 192), (100, 257), (1300, 5000), (70, 64), (1, 1), (0, 130)])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 130])
def test_lift_rows_equals_statement(lift, k, m, n):
    from beyond_fixed_forms_amd import _lib
    rows, nn = lift_case(k, m, n, seed=k)
    exp = lr.lift_ref(nn, rows, m, n)
    got = lift.lift_rows(torch.from_numpy(nn).to(DEV), dev_rows(rows), m, n)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (k, (n + 63) // 64) == exp.shape
    assert np.array_equal(got.cpu().numpy(), exp)                            # output padding zero, input padding ignored
    if k and n % 64:
        assert (lr.unpack(got.cpu().numpy(), 64 * got.shape[1])[:, n:] == 0).all()
    if k and m:                                                              # the independent cross-check: no holes
        rows, nn = lift_case(k, m, n, seed=k, holes=False)
        got = lift.lift_rows(torch.from_numpy(nn).to(DEV), dev_rows(rows), m, n)
        assert torch.equal(got, _lib.permute_bits(dev_rows(rows), torch.from_numpy(nn).to(DEV), n))
        assert np.array_equal(got.cpu().numpy(), lr.lift_ref(nn, rows, m, n))


def test_lift_rows_arguments(lift):
    rows, nn = lift_case(3, 100, 257)
    d_rows, d_nn = dev_rows(rows), torch.from_numpy(nn).to(DEV)
    with pytest.raises(ValueError, match="no CPU"):
        lift.lift_rows(d_nn, torch.from_numpy(rows), 100, 257)
    with pytest.raises(ValueError, match="no CPU"):
        lift.lift_rows(torch.from_numpy(nn), d_rows, 100, 257)
    with pytest.raises(TypeError):
        lift.lift_rows(d_nn.long(), d_rows, 100, 257)
    with pytest.raises(TypeError):
        lift.lift_rows(d_nn, d_rows.to(torch.int32), 100, 257)
    with pytest.raises(ValueError, match="words"):
        lift.lift_rows(d_nn, d_rows, 200, 257)                               # 200 points need 4 words, the rows have 3
    with pytest.raises(ValueError, match="target"):
        lift.lift_rows(d_nn, d_rows, 100, 256)
    a, b = lift.lift_rows(d_nn, d_rows, 100, 257), lift.lift_rows(d_nn, d_rows, 100, 257)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ the subsample
def test_subsample_equals_numpy(lift):
    pts = np.concatenate([lr.three_planes(3000, seed=41), np.full((3000, 3), 9.0)], axis=1)
    pts[[0, 7, 1500, 2999], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
    fin = np.isfinite(pts[:, :3]).all(1)
    key = np.floor((pts[fin, :3] - pts[fin, :3].min(0)) / V).astype(np.int64) @ np.array([1, 1 << 21, 1 << 42])
    want = np.sort(np.flatnonzero(fin)[np.unique(key, return_index=True)[1]]).astype(np.int32)
    for cloud in (pts, torch.from_numpy(pts).to(DEV)):
        got = lift.subsample(cloud, V, DEV)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want, lr.subsample_ref(pts, V)) and not np.isin([0, 7, 1500, 2999], want).any()
    assert (np.diff(want) > 0).all() and 500 < len(want) < 3000
    assert tuple(lift.subsample(np.zeros((0, 3)), V, DEV).shape) == (0,)
    assert tuple(lift.subsample(np.full((5, 3), np.nan), V, DEV).shape) == (0,)
    assert lift.subsample(np.zeros((4, 3)), V, DEV).tolist() == [0]          # one cell: its smallest index


# ------------------------------------------------------------------ the wrapper, the tools, a generator scene
@functools.lru_cache(maxsize=None)
def scene_case():
    from beyond_fixed_forms_amd import lift
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import project_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("c1", n_views=24, distinct_masks=True, cut_masks=False)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height, subsample_voxel=0.15)
    sample = lift.subsample(scene.points, lift.subsample_voxel(cfg), DEV).cpu().numpy()
    small = dataclasses.replace(scene, points=scene.points[sample], point_object=scene.point_object[sample], stage1=None)
    res = project_scene(small, cfg, device=DEV, return_result=True)
    return scene, small, sample, cfg, res


def test_lift_instances_of_a_generator_scene(lift):
    scene, small, sample, cfg, res = scene_case()
    n, m = scene.points.shape[0], len(sample)
    assert 1000 < m < n and res.rows.shape[0] >= 1 and res.n_points == m
    radius = lift.lift_max_dist(cfg)
    assert radius == 2 * 0.15
    nn = lift.nearest(lift.nearest_index(small.points, radius, DEV), scene.points)
    exp_nn = scene_nn()
    assert np.array_equal(nn.cpu().numpy(), exp_nn)
    assert (exp_nn >= 0).all() and np.array_equal(exp_nn[sample], np.arange(m))      # nobody is left without a source
    got = lift.lift_instances(nn, res, m, n)
    assert type(got) is type(res) and got is not res and res.n_points == m and got.n_points == n
    rows = res.rows.cpu().numpy()
    assert np.array_equal(got.rows.cpu().numpy(), lr.lift_ref(exp_nn, rows, m, n))
    dense = lr.unpack(got.rows.cpu().numpy(), n)
    assert np.array_equal(dense[:, sample], lr.unpack(rows, m))              # restricted to the sample: the small run's rows
    assert dense.shape[0] == rows.shape[0] and got.final_class == res.final_class and got.conf is res.conf
    assert getattr(got, "prefetch", None) is None
    d = got.to_dict()
    assert tuple(d["ins"].shape) == (rows.shape[0], n) and np.array_equal(d["ins"].cpu().numpy(), dense)
    listed = SimpleNamespace(rows=torch.cat([res.rows, torch.zeros_like(res.rows[:1])]), conf=[0.5] * (rows.shape[0] + 1),
                             final_class=[f"thing {i}" for i in range(rows.shape[0] + 1)])
    got = lift.lift_instances(nn, listed, m, n)                              # an empty row stays, in its place
    assert got.rows.shape[0] == rows.shape[0] + 1 and not got.rows[-1].any() and got.conf is listed.conf
    assert got.final_class == listed.final_class and torch.equal(got.rows[:-1], lift.lift_rows(nn, res.rows, m, n))


@functools.lru_cache(maxsize=None)
def scene_nn():
    scene, small = scene_case()[:2]
    return lr.nearest_ref(small.points, 0.3, scene.points)[0]


def run_main(name, tmp_path, *argv):
    """cli.<name> in this process, torch's thread count put back."""
    from beyond_fixed_forms_amd import cli
    threads = torch.get_num_threads()
    try:
        return getattr(cli, name)(["--config", str(tmp_path / "config.yaml"), *argv])
    finally:
        torch.set_num_threads(threads)


def tool_tree(tmp_path):
    """The full clouds (one of them float32) and the first tool's config."""
    import yaml
    from beyond_fixed_forms_amd.config import Config
    scene = scene_case()[0]
    (tmp_path / "full").mkdir()
    for name in ("scene_a", "scene_empty"):
        np.save(tmp_path / "full" / f"{name}.npy", scene.points.astype(np.float32) if name == "scene_empty" else scene.points)
    cfg = Config.with_defaults(scene_npy_dir=str(tmp_path / "full"), subsample_npy_dir=str(tmp_path / "small"), subsample_voxel=0.15)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    return cfg


def small_run_tree(tmp_path, cfg, stage, cls):
    """The small run's config (scene_npy_dir names the subsample's folder) and its saved instances of one class."""
    import yaml
    _, _, sample, _, res = scene_case()
    dirs = {"final": tmp_path / "final", "mask_3d": tmp_path / "m3d"}
    dense = lr.unpack(res.rows.cpu().numpy(), len(sample))
    (dirs[stage] / cls).mkdir(parents=True)
    conf = torch.linspace(0.3, 0.8, len(dense)).to(torch.float16)
    names = [f"thing {i}" for i in range(len(dense))]
    torch.save({"ins": torch.from_numpy(dense), "conf": conf, "final_class": names}, dirs[stage] / cls / "scene_a.pth")
    torch.save({"ins": [], "conf": [], "final_class": []}, dirs[stage] / cls / "scene_empty.pth")
    cfg = dict(cfg, scene_npy_dir=str(tmp_path / "small"), lift_target_npy_dir=str(tmp_path / "full"),
               lift_output_dir=str(tmp_path / "lift"), final_output_dir=str(dirs["final"]), mask_3d_dir=str(dirs["mask_3d"]))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    return dirs, dense, conf, names


@pytest.mark.parametrize("stage,rle", [("final", False), ("mask_3d", True)])
def test_tools(lift, tmp_path, monkeypatch, stage, rle):
    from oracle import rle_ref
    scene, small, sample, _, res = scene_case()
    n, m, cls = scene.points.shape[0], len(sample), "table"
    cfg = tool_tree(tmp_path)
    assert run_main("subsample_main", tmp_path, "--scene", "scene_a") == 0
    assert not (tmp_path / "small" / "scene_empty.npy").exists()            # only the named scene
    assert run_main("subsample_main", tmp_path) == 0
    got = np.load(tmp_path / "small" / "scene_a.npy")
    idx = np.load(tmp_path / "small" / "sample" / "scene_a.npy")
    assert idx.dtype == np.int32 and np.array_equal(idx, sample)
    assert got.dtype == scene.points.dtype and np.array_equal(got, scene.points[sample])      # all columns, the dtype kept
    assert np.load(tmp_path / "small" / "scene_empty.npy").dtype == np.float32
    dirs, dense, conf, names = small_run_tree(tmp_path, cfg, stage, cls)
    monkeypatch.setenv("BFF_SAVE_RLE", "1" if rle else "0")
    assert run_main("lift_main", tmp_path, "--cls", cls, "--stage", stage) == 0
    out = torch.load(tmp_path / "lift" / cls / "scene_a.pth", weights_only=False)
    if rle:
        assert isinstance(out["ins"], list) and all(int(x["length"]) == n for x in out["ins"])
        ins = rle_ref.rle_decode_batch_ref(out["ins"]).bool().numpy()
    else:
        assert out["ins"].dtype == torch.bool and not out["ins"].is_cuda
        ins = out["ins"].numpy()
    assert np.array_equal(ins, lr.unpack(lr.lift_ref(scene_nn(), res.rows.cpu().numpy(), m, n), n))
    assert out["conf"].dtype == torch.float16 and torch.equal(out["conf"], conf) and out["final_class"] == names
    assert torch.load(tmp_path / "lift" / cls / "scene_empty.pth", weights_only=False) == {"ins": [], "conf": [], "final_class": []}
    # masks of another length than the source cloud: an error naming the scene
    torch.save({"ins": torch.from_numpy(dense[:, :-1]), "conf": conf, "final_class": names}, dirs[stage] / cls / "scene_a.pth")
    with pytest.raises(ValueError, match="scene_a"):
        run_main("lift_main", tmp_path, "--cls", cls, "--stage", stage)
    other = "mask_3d" if stage == "final" else "final"
    assert run_main("lift_main", tmp_path, "--cls", cls, "--stage", other) == 1          # that stage has no directory


def test_tool_scripts_run_end_to_end(lift, tmp_path):
    """The two scripts as processes of their own, one after the other, on a generator scene written to disk."""
    scene, _, sample, _, res = scene_case()
    n, m, cls = scene.points.shape[0], len(sample), "table"
    run = lambda tool, *argv: subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--config",
                                              str(tmp_path / "config.yaml"), *argv], cwd=tmp_path, capture_output=True,
                                             text=True, timeout=300)
    cfg = tool_tree(tmp_path)
    r = run("subsample_cloud.py", "--scene", "scene_a")
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(tmp_path / "small" / "sample" / "scene_a.npy"), sample)
    small_run_tree(tmp_path, cfg, "final", cls)
    (tmp_path / "final" / cls / "scene_empty.pth").unlink()                 # its small cloud was not made
    r = run("lift_instances_3d.py", "--cls", cls)
    assert r.returncode == 0, r.stderr[-2000:]
    out = torch.load(tmp_path / "lift" / cls / "scene_a.pth", weights_only=False)
    assert np.array_equal(out["ins"].numpy(), lr.unpack(lr.lift_ref(scene_nn(), res.rows.cpu().numpy(), m, n), n))
