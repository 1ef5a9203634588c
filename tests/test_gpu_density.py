"""3-D instances clustered by density on the GPU: density.cluster_rows (bff_dbscan_elements, bff_dbscan_core,
bff_dbscan_link and the split's tail), cluster_instances and the command-line tool against their NumPy statement
(tests/density_ref.py: brute force over every pair).  Rows, parents and point counts are compared for equality."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import density_cases as dc
import density_ref as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def density():
    from beyond_fixed_forms_amd import _lib, density
    _lib.load()
    assert torch.cuda.is_available()
    return density


def dev_rows(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(DEV)


def check(density, pts, eps, min_samples, rows, min_points=1, mode="split", index=None, expected=None):
    """The device's rows, parents and point counts against the statement's; -> the statement's."""
    n = len(pts)
    exp = dr.cluster_ref(pts, eps, min_samples, rows, n, min_points, mode) if expected is None else expected
    index = density.density_index(pts, eps, DEV) if index is None else index
    out, parent, count = density.cluster_rows(index, dev_rows(rows), n, min_samples, min_points, mode)
    assert out.dtype == torch.int64 and out.is_cuda and parent.dtype == count.dtype == torch.int64
    assert not parent.is_cuda and not count.is_cuda
    assert tuple(out.shape) == exp[0].shape and out.shape[1] == rows.shape[1]
    assert np.array_equal(parent.numpy(), exp[1]) and np.array_equal(count.numpy(), exp[2])
    assert np.array_equal(out.cpu().numpy(), exp[0])                        # bit for bit: the padding bits zero
    return exp


# ------------------------------------------------------------------ hand cases
def test_a_size_that_is_no_multiple_of_64_and_garbage_padding(density):
    n = 1000 + 37
    pts = dr.blobs(n, seed=3)
    rows = dc.garbage(dc.random_rows(n, [300, 700, n], seed=4), n)
    out, parent, count = check(density, pts, 0.1, 4, rows)
    assert out.shape[1] == (n + 63) // 64 + 1 and len(set(parent.tolist())) == 3 and len(parent) > 6
    assert (dr.unpack(out, 64 * out.shape[1])[:, n:] == 0).all() and count.max() > 50


def test_a_pair_at_exactly_eps(density):
    pts = dc.exact_boundary()
    out, _, count = check(density, pts, dc.EPS, 2, dc.all_set(3))
    assert count.tolist() == [2] and dr.unpack(out, 3).tolist() == [[True, True, False]]
    out, parent, count = check(density, pts, dc.EPS, 1, dc.all_set(3))
    assert count.tolist() == [2, 1] and dr.unpack(out, 3).tolist() == [[True, True, False], [False, False, True]]


def test_neighbours_in_all_26_directions_at_the_grids_ends(density):
    pts, centre = dc.all_directions()
    index = density.density_index(pts, dc.EPS, DEV)
    cell = index.nearest.grid.cell
    q = np.floor((pts - pts.min(0)) / cell).astype(int)
    assert len({tuple(c) for c in q[:27].tolist()}) == 27 and q[:27].min() == 0 and q[:27].max() == 2 == q.max()
    out, _, count = check(density, pts, dc.EPS, 27, dc.all_set(28), index=index)   # the centre is core only with all 26 found
    assert count.tolist() == [27] and dr.unpack(out, 28)[0].tolist() == [True] * 27 + [False]
    for min_samples in (1, 4, 8):                                            # the corners ask from the first and the last cell
        check(density, pts, dc.EPS, min_samples, dc.all_set(28), index=index)


def test_min_samples_one_and_min_samples_above_every_count(density):
    pts = dr.blobs(800, seed=6)
    rows = dc.random_rows(800, [800, 300], seed=7)
    index = density.density_index(pts, 0.1, DEV)
    out, parent, count = check(density, pts, 0.1, 1, rows, index=index)      # everybody is core: plain eps-connectivity
    assert count.sum() == 1100 and (count == 1).sum() > 10 and count.max() > 100
    out, parent, count = check(density, pts, 0.1, 10 ** 6, rows, index=index)
    assert tuple(out.shape) == (0, 13) and len(parent) == len(count) == 0


@pytest.mark.parametrize("mode", ["split", "largest"])
def test_more_kept_clusters_than_the_first_read_fetches(density, monkeypatch, mode):
    """Six kept clusters, five of them in row 0, against a first read of two: the rest comes with the overflow fetch, and
    the result is the statement's and the one of a first read that holds them all."""
    from beyond_fixed_forms_amd import instances3d
    pts, rows = dc.five_groups()
    index = density.density_index(pts, dc.EPS, DEV)
    whole = [t.cpu() for t in density.cluster_rows(index, dev_rows(rows), 70, 3, 1, mode)]
    monkeypatch.setattr(instances3d, "KEPT_FIRST_READ", 2)
    _, parent, count = check(density, pts, dc.EPS, 3, rows, 1, mode, index=index)
    assert count.tolist() == ([14, 12, 12, 12, 10, 10] if mode == "split" else [14, 10]) and parent.tolist()[-1] == 1
    again = [t.cpu() for t in density.cluster_rows(index, dev_rows(rows), 70, 3, 1, mode)]
    assert all(torch.equal(a, b) for a, b in zip(whole, again))


@pytest.mark.parametrize("tie", [True, False])
def test_border_points_follow_their_nearest_core_neighbour(density, tie):
    pts, x, anchor = dc.two_clusters(tie)
    out, parent, count = check(density, pts, dc.EPS, 5, dc.all_set(11))
    assert count.tolist() == [6, 5]
    dense = dr.unpack(out, 11)
    assert dense[0, x] and dense[0, anchor] and dense[1, 0] and not dense[1, x]


def test_a_chain_of_2000_points_is_one_cluster(density):
    pts = dc.chain(2000)                                                     # shuffled: unions in every direction
    index = density.density_index(pts, dc.EPS, DEV)
    assert index.nearest.grid.n_voxels > 1900                                # about one point per cell
    for min_samples in (1, 2, 3):                                            # at 3 the two ends are border points
        out, _, count = check(density, pts, dc.EPS, min_samples, dc.all_set(2000), index=index)
        assert count.tolist() == [2000] and np.array_equal(out, dc.all_set(2000))
    _, _, count = check(density, pts, dc.EPS, 4, dc.all_set(2000), index=index)
    assert len(count) == 0


def test_200_duplicates_in_one_cell(density):
    pts = dc.duplicates(200)
    for min_samples, counts in ((1, [201, 1]), (200, [201]), (201, [201]), (202, [])):
        _, _, count = check(density, pts, dc.EPS, min_samples, dc.all_set(202))
        assert count.tolist() == counts
    rows = dr.pack(np.array([[1] * 100 + [0] * 100 + [1, 1], [0] * 100 + [1] * 100 + [0, 1]], bool))
    _, parent, count = check(density, pts, dc.EPS, 100, rows)                # two rows that share the cell: independent
    assert parent.tolist() == [0, 1] and count.tolist() == [101, 100]


def test_rows_that_share_points_an_empty_row_and_non_finite_points(density):
    pts, x, _ = dc.two_clusters(True)
    pts = np.concatenate([pts, [[np.nan, 0.0, 0.0]], [[0.5, np.inf, 0.0]], [[0.5, 0.0, -np.inf]]])
    n = len(pts)
    rows = dc.garbage(dr.pack(np.array([[1] * 14, [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1], [0] * 14,
                                        [0] * 11 + [1, 1, 1]], bool)), n)
    index = density.density_index(pts, dc.EPS, DEV)
    out, parent, count = check(density, pts, dc.EPS, 5, rows, index=index)
    assert parent.tolist() == [0, 0, 1] and count.tolist() == [6, 5, 6]
    dense = dr.unpack(out, n)
    assert dense[0, x] and dense[2, x] and not dense[:, 11:].any()           # X goes to B in row 0, to A in row 1
    check(density, pts, dc.EPS, 5, rows, mode="largest", index=index)
    check(density, pts, dc.EPS, 1, rows, index=index)                        # a non-finite point is not even its own cluster
    out, parent, count = density.cluster_rows(index, dev_rows(rows[:0]), n, 5)      # K = 0
    assert tuple(out.shape) == (0, 2) and len(parent) == len(count) == 0
    only_bad = density.density_index(pts[11:], dc.EPS, DEV)                  # no finite point: no grid, no row
    out, parent, _ = density.cluster_rows(only_bad, dev_rows(dc.all_set(3)), 3, 1)
    assert tuple(out.shape) == (0, 1) and len(parent) == 0
    none = density.density_index(np.zeros((0, 3)), dc.EPS, DEV)
    assert tuple(density.cluster_rows(none, dev_rows(np.zeros((2, 0), np.int64)), 0, 1)[0].shape) == (0, 0)


# ------------------------------------------------------------------ the random case
N_RANDOM = 6000


@functools.lru_cache(maxsize=None)
def random_case():
    pts = dr.blobs(N_RANDOM, n_blobs=6, seed=21)
    rows = dc.random_rows(N_RANDOM, [500, 1200, 1900, 2500, 3000], seed=22)
    return pts, rows


@functools.lru_cache(maxsize=None)
def random_labels(min_samples):
    """Per row the statement's labels: the brute force runs once per min_samples, mode and min_points only choose."""
    pts, rows = random_case()
    return [dr.labels_ref(pts, 0.1, min_samples, d)[0] for d in dr.unpack(rows, N_RANDOM)]


def chosen(labels, nw, min_points, mode):
    out, parent, count = [], [], []
    for k, label in enumerate(labels):
        comps = [(int((label == a).sum()), int(a)) for a in np.unique(label[label >= 0])]
        comps = sorted((c for c in comps if c[0] >= min_points), key=lambda c: (-c[0], c[1]))
        for size, a in (comps[:1] if mode == "largest" else comps):
            out.append(label == a), parent.append(k), count.append(size)
    packed = dr.pack(np.stack(out), nw) if out else np.zeros((0, nw), np.int64)
    return packed, np.asarray(parent, np.int64), np.asarray(count, np.int64)


@pytest.fixture(scope="module")
def random_index(density):
    return density.density_index(random_case()[0], 0.1, DEV)


@pytest.mark.parametrize("min_points", [1, 20])
@pytest.mark.parametrize("mode", ["split", "largest"])
@pytest.mark.parametrize("min_samples", [4, 8])
def test_random_blobs_and_noise(density, random_index, min_samples, mode, min_points):
    pts, rows = random_case()
    exp = chosen(random_labels(min_samples), rows.shape[1], min_points, mode)
    out, parent, count = check(density, pts, 0.1, min_samples, rows, min_points, mode, index=random_index, expected=exp)
    assert len(set(parent.tolist())) == 5 and count.max() > 100
    if mode == "split" and min_points == 1:
        assert len(parent) > 20 and count.sum() < 9100 - 1000                # of the rows' 9100 points the noise is dropped
    if mode == "split" and min_points == 1 and min_samples == 4:
        assert count.min() < 20                                              # small clusters in the noise
    if min_samples == 4 and mode == "split" and min_points == 1:             # the shared helper is cluster_ref's choice
        small = dr.cluster_ref(pts, 0.1, 4, rows[:1], N_RANDOM)
        assert np.array_equal(small[0], out[:len(small[0])]) and np.array_equal(small[2], count[:len(small[0])])


def test_two_calls_are_equal_and_inputs_are_checked(density, random_index):
    pts, rows = random_case()
    d_rows = dev_rows(rows)
    a = density.cluster_rows(random_index, d_rows, N_RANDOM, 4)
    b = density.cluster_rows(random_index, d_rows, N_RANDOM, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    again = density.density_index(torch.from_numpy(pts).to(DEV), 0.1)        # a device cloud: the same index
    c = density.cluster_rows(again, d_rows, N_RANDOM, 4)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    six = np.concatenate([pts, np.full((N_RANDOM, 3), 7.0)], axis=1)          # an array of 6 columns, a stride of 6
    for cloud in (six, torch.from_numpy(six).to(DEV)):
        c = density.cluster_rows(density.density_index(cloud, 0.1, DEV), d_rows, N_RANDOM, 4)
        assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])
    with pytest.raises(ValueError, match="no CPU"):
        density.cluster_rows(random_index, torch.from_numpy(rows), N_RANDOM, 4)
    with pytest.raises(TypeError):
        density.cluster_rows(random_index, d_rows.to(torch.int32), N_RANDOM, 4)
    with pytest.raises(ValueError, match="words"):
        density.cluster_rows(random_index, d_rows[:, :-1].contiguous(), N_RANDOM, 4)
    with pytest.raises(ValueError, match="index holds"):
        density.cluster_rows(random_index, d_rows, N_RANDOM - 1, 4)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_samples"):
            density.cluster_rows(random_index, d_rows, N_RANDOM, bad)
        with pytest.raises(ValueError, match="min_points"):
            density.cluster_rows(random_index, d_rows, N_RANDOM, 4, bad)
    with pytest.raises(ValueError, match="mode"):
        density.cluster_rows(random_index, d_rows, N_RANDOM, 4, 1, "dbscan")


# ------------------------------------------------------------------ the wrapper and the tool
@pytest.mark.parametrize("kind", ["list", "tensor", "ndarray"])
def test_cluster_instances_keeps_container_kind_and_dtype(density, random_index, kind):
    from beyond_fixed_forms_amd.config import Config
    pts, rows = random_case()
    conf = [0.9, 0.8, 0.7, 0.6, 0.5]
    conf = {"list": conf, "tensor": torch.tensor(conf, dtype=torch.float16), "ndarray": np.asarray(conf, np.float32)}[kind]
    names = [f"thing {i}" for i in range(5)]
    res = SimpleNamespace(rows=dev_rows(rows), conf=conf, final_class=names, prefetch=object())
    cfg = Config.with_defaults(cluster_eps=0.1, cluster_min_samples=8, cluster_min_points=20)
    got = density.cluster_instances(random_index, res, cfg)
    exp = chosen(random_labels(8), rows.shape[1], 20, "split")
    assert got is not res and res.rows.shape[0] == 5 and got.prefetch is None
    assert np.array_equal(got.rows.cpu().numpy(), exp[0]) and np.array_equal(got.parent.numpy(), exp[1])
    assert got.final_class == [names[i] for i in exp[1].tolist()] and type(got.conf) is type(conf)
    if kind == "list":
        assert got.conf == [conf[i] for i in exp[1].tolist()]
    else:
        assert got.conf.dtype == conf.dtype and np.array_equal(np.asarray(got.conf), np.asarray(conf)[exp[1]])
    largest = density.cluster_instances(random_index, res, dict(cfg, cluster_mode="largest"))
    assert largest.parent.tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="cluster_min_samples"):
        density.cluster_instances(random_index, res, Config.with_defaults(cluster_eps=0.1))


def tool_tree(tmp_path, stage, cls):
    """A tiny saved scene: the random case's cloud (6 columns) and its rows as the stage's file, and an empty form."""
    import yaml
    from beyond_fixed_forms_amd.config import Config
    pts, rows = random_case()
    dirs = {"final": tmp_path / "final", "mask_3d": tmp_path / "m3d"}
    (tmp_path / "npy").mkdir()
    np.save(tmp_path / "npy" / "scene_a.npy", np.concatenate([pts, np.full((N_RANDOM, 3), 7.0)], axis=1))
    np.save(tmp_path / "npy" / "scene_empty.npy", pts[:100].astype(np.float32))
    (dirs[stage] / cls).mkdir(parents=True)
    conf = torch.linspace(0.3, 0.8, 5).to(torch.float16)
    names = [f"thing {i}" for i in range(5)]
    torch.save({"ins": torch.from_numpy(dr.unpack(rows, N_RANDOM)), "conf": conf, "final_class": names},
               dirs[stage] / cls / "scene_a.pth")
    torch.save({"ins": [], "conf": [], "final_class": []}, dirs[stage] / cls / "scene_empty.pth")
    cfg = Config.with_defaults(scene_npy_dir=str(tmp_path / "npy"), final_output_dir=str(dirs["final"]), mask_3d_dir=str(dirs["mask_3d"]),
                               cluster_output_dir=str(tmp_path / "cluster"), cluster_eps=0.1, cluster_min_samples=8,
                               cluster_min_points=20)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    return conf, names


@pytest.mark.parametrize("stage,rle", [("final", False), ("mask_3d", True)])
def test_tool(density, tmp_path, monkeypatch, stage, rle):
    from beyond_fixed_forms_amd import cli
    from oracle import rle_ref
    cls = "table"
    conf, names = tool_tree(tmp_path, stage, cls)
    monkeypatch.setenv("BFF_SAVE_RLE", "1" if rle else "0")
    threads = torch.get_num_threads()
    try:
        assert cli.cluster_main(["--config", str(tmp_path / "config.yaml"), "--cls", cls, "--stage", stage]) == 0
        other = "mask_3d" if stage == "final" else "final"                   # that stage has no directory
        assert cli.cluster_main(["--config", str(tmp_path / "config.yaml"), "--cls", cls, "--stage", other]) == 1
    finally:
        torch.set_num_threads(threads)
    out = torch.load(tmp_path / "cluster" / cls / "scene_a.pth", weights_only=False)
    exp = chosen(random_labels(8), (N_RANDOM + 63) // 64, 20, "split")
    if rle:
        assert isinstance(out["ins"], list) and all(int(x["length"]) == N_RANDOM for x in out["ins"])
        ins = rle_ref.rle_decode_batch_ref(out["ins"]).bool().numpy()
    else:
        assert out["ins"].dtype == torch.bool and not out["ins"].is_cuda
        ins = out["ins"].numpy()
    assert np.array_equal(ins, dr.unpack(exp[0], N_RANDOM)) and len(ins) > 5
    assert torch.equal(out["parent"], torch.from_numpy(exp[1])) and out["conf"].dtype == torch.float16
    assert torch.equal(out["conf"], conf[out["parent"]]) and out["final_class"] == [names[i] for i in exp[1].tolist()]
    assert torch.load(tmp_path / "cluster" / cls / "scene_empty.pth", weights_only=False) == {"ins": [], "conf": [], "final_class": []}


def test_tool_script_runs_end_to_end(density, tmp_path):
    """The script as a process of its own."""
    tool_tree(tmp_path, "final", "table")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cluster_instances_3d.py"), "--config",
                        str(tmp_path / "config.yaml"), "--cls", "table"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = torch.load(tmp_path / "cluster" / "table" / "scene_a.pth", weights_only=False)
    exp = chosen(random_labels(8), (N_RANDOM + 63) // 64, 20, "split")
    assert np.array_equal(out["ins"].numpy(), dr.unpack(exp[0], N_RANDOM))
