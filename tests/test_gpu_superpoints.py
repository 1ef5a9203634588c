"""3-D instances snapped to superpoints on the GPU: the index, the three entry points (bff_spp_*), superpoints.snap_rows,
snap_instances and the command-line tool against their NumPy statement (tests/superpoints_ref.py).  Everything is
compared for equality."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import superpoints_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what one step of the implementation covers
FILL_PASS = 64                # points of a superpoint one pass of a wave's fill loop covers
BLOCK_SUPERPOINTS = 256       # superpoints per block of the owner kernel (256 threads) and of the fill kernel (4 waves x 64)
COUNT_BLOCK_WORDS = 256       # words of a row per block of the count kernel (4 waves x 64 words = 16 384 points)
MODES = ("snap", "exclusive")


@pytest.fixture(scope="module")
def sp():
    from beyond_fixed_forms_amd import _lib, superpoints
    _lib.load()
    assert torch.cuda.is_available()
    return superpoints


def dev_rows(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(DEV)


def with_garbage(rows, n):
    """The same rows with every bit at a position >= n set."""
    rows = np.array(rows, dtype=np.int64)
    if n % 64:
        rows[:, n // 64] |= np.int64(-1) << np.int64(n % 64)
    rows[:, (n + 63) // 64:] = -1
    return rows


def check_index(sp, spp):
    exp = pr.index_ref(spp)
    ix = sp.superpoint_index(spp, DEV)
    n, s = len(exp["seg"]), len(exp["ids"])
    assert (ix.n_points, ix.n_segments) == (n, s)
    assert ix.seg.dtype == ix.order.dtype == ix.offs.dtype == ix.size.dtype == torch.int32
    assert ix.ids.dtype == ix.free.dtype == torch.int64 and tuple(ix.free.shape) == (1, (n + 63) // 64)
    assert np.array_equal(ix.ids.cpu().numpy(), exp["ids"]) and np.array_equal(ix.seg.cpu().numpy(), exp["seg"])
    assert np.array_equal(ix.size.cpu().numpy(), exp["size"]) and np.array_equal(ix.offs.cpu().numpy(), exp["offs"])
    assert np.array_equal(ix.order.cpu().numpy(), exp["order"])            # stable: ascending point index
    assert np.array_equal(ix.free.cpu().numpy(), pr.pack(exp["free"][None, :]))
    return ix, exp


def check_snap(sp, index, spp, rows, n, ratio=0.5, mode="snap", min_points=1):
    """rows: int64 [K][nw] (NumPy).  The device's rows, parent and points against the statement's; -> the statement's."""
    exp = pr.snap_ref(spp, rows, n, ratio, mode, min_points)
    out, parent, points = sp.snap_rows(index, dev_rows(rows), n, ratio, mode, min_points)
    assert out.dtype == torch.int64 and out.is_cuda and parent.dtype == points.dtype == torch.int64
    assert not parent.is_cuda and not points.is_cuda and tuple(out.shape) == exp[0].shape
    assert np.array_equal(parent.numpy(), exp[1]) and np.array_equal(points.numpy(), exp[2])
    assert np.array_equal(out.cpu().numpy(), exp[0])
    return exp


# ------------------------------------------------------------------ the index
def index_ids():
    """N = 1000 (15.6 words), 40 distinct ids >= 0 interleaved across the cloud: small ones, values above 2^40 up to 2^62,
    the ids -1 and -7 among them, a superpoint of exactly one point."""
    rng = np.random.default_rng(31)
    values = np.concatenate([rng.integers(0, 500, 20), (1 << 40) + rng.integers(0, 1 << 20, 17), [1 << 62, (1 << 62) - 1, 0]])
    values = np.unique(values)[:39]
    spp = values[rng.integers(0, len(values), 1000)]
    spp[rng.choice(1000, 30, replace=False)] = np.repeat([-1, -7], 15)
    spp[spp == 123456789] = 0
    spp[517] = 123456789                                                    # the superpoint of one point
    return spp.astype(np.int64)


def test_index_equals_numpy(sp):
    spp = index_ids()
    ix, exp = check_index(sp, spp)
    assert len(exp["ids"]) == 40 and exp["ids"][-1] >= (1 << 61) and (exp["ids"] > (1 << 40)).sum() >= 10
    assert exp["free"].sum() == 30 and 1 in exp["size"].tolist() and exp["seg"][517] >= 0
    assert ix.need(0.5).dtype == torch.int32 and np.array_equal(ix.need(0.5).cpu().numpy(), pr.need_ref(exp["size"], 0.5))
    small = np.where(spp > 1000, spp % 1000 + 1000, spp)
    for kind in (small.astype(np.int32), torch.from_numpy(spp), torch.from_numpy(spp).to(DEV), small.astype(np.int16)):
        got = sp.superpoint_index(kind, DEV)                                 # any integer dtype, array or tensor
        want = pr.index_ref(kind.cpu().numpy() if torch.is_tensor(kind) else kind)
        assert np.array_equal(got.seg.cpu().numpy(), want["seg"]) and np.array_equal(got.ids.cpu().numpy(), want["ids"])
    again = sp.superpoint_index(spp, DEV)
    assert all(torch.equal(getattr(ix, f), getattr(again, f)) for f in ("ids", "seg", "order", "offs", "size", "free"))


def test_index_edge_cases(sp):
    ix, _ = check_index(sp, np.full(200, -3, np.int64))                     # all ids negative: S = 0
    assert ix.n_segments == 0 and tuple(ix.offs.shape) == (1,)
    ix, exp = check_index(sp, np.full(200, 1 << 45, np.int64))              # one superpoint holds every point
    assert exp["size"].tolist() == [200] and exp["order"].tolist() == list(range(200))
    ix, _ = check_index(sp, np.zeros(0, np.int64))                          # N = 0
    assert (ix.n_points, ix.n_segments) == (0, 0) and tuple(ix.free.shape) == (1, 0)
    rng = np.random.default_rng(32)
    check_index(sp, rng.integers(-1, 5, 130))                               # N = 130: two words and two bits
    check_index(sp, np.arange(130)[::-1].copy())                            # every point a superpoint of its own


# ------------------------------------------------------------------ count, owner, fill, snap_rows
SIZES = (1, 63, 64, 65, 300, 100)             # superpoints 0 .. 5 of the case below, by id


@functools.lru_cache(maxsize=None)
def main_case(k):
    """N = 1000.  Superpoints of 1, 63, 64, 65, 300 and 100 points (ids 0 .. 5) scattered over the cloud, 7 free points,
    the other 400 points in 12 more superpoints.  k rows: densities 0, 0.02, 0.5 (rows 0 .. 2) and 1 (the last row); row 3
    identical to the 300-point superpoint; the 100-point superpoint hit by 55 (row 4) and by 56 points (row 5); random
    densities for the rest."""
    rng = np.random.default_rng(33)
    n = 1000
    perm = rng.permutation(n)
    spp = np.empty(n, np.int64)
    at = 0
    for j, size in enumerate(SIZES):
        spp[perm[at:at + size]] = j
        at += size
    spp[perm[at:at + 7]] = -1 - np.arange(7)
    spp[perm[at + 7:]] = 10 + rng.integers(0, 12, n - at - 7)
    spp = np.where(spp >= 0, spp * 1_000_003 + 17, spp)                      # neither dense nor small
    ident = lambda j: spp == j * 1_000_003 + 17
    dense = rng.random((k, n)) < rng.random((k, 1))
    if k == 1:
        dense[0] = rng.random(n) < 0.5
    else:
        for row, d in ((0, 0.0), (1, 0.02), (2, 0.5), (k - 1, 1.0)):         # the full row last: it wins no tie in "exclusive"
            dense[row] = rng.random(n) < d
        dense[3] = ident(4)
        hundred = np.flatnonzero(ident(5))
        for row, hits in ((4, 55), (5, 56)):
            dense[row] = rng.random(n) < 0.1
            dense[row, hundred] = False
            dense[row, hundred[:hits]] = True
    return spp, with_garbage(pr.pack(dense), n), n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ratio", [1e-9, 0.5, 0.55, 1.0])
@pytest.mark.parametrize("k", [1, 70])
def test_snap_rows_equals_statement(sp, k, ratio, mode):
    spp, rows, n = main_case(k)
    index = sp.superpoint_index(spp, DEV)
    assert sorted(index.size.cpu().tolist())[0] == 1 and {63, 64, 65, 100, 300} <= set(index.size.cpu().tolist())
    assert 300 > 4 * FILL_PASS and rows[0, -1] >> 40 == -1                  # several passes; garbage in the bits >= N
    out, parent, points = check_snap(sp, index, spp, rows, n, ratio, mode)
    if k == 70 and mode == "snap":
        got = {int(p): r for r, p in enumerate(parent)}
        hundred = spp == 5 * 1_000_003 + 17
        took = lambda row: row in got and bool(pr.unpack(out[got[row]:got[row] + 1], n)[0, hundred].all())
        if ratio == 0.55:                                                   # need = 56: 55 points do not take it, 56 do
            assert not took(4) and took(5)
        if ratio == 0.5:
            assert took(4) and took(5)
        if ratio == 1.0:                                                    # the row identical to a superpoint keeps it
            assert np.array_equal(pr.unpack(out[got[3]:got[3] + 1], n)[0], spp == 4 * 1_000_003 + 17)
        assert 0 not in got and points[got[k - 1]] == n                     # the empty row is dropped, the full one stays full


@pytest.mark.parametrize("ratio", [0.5, 0.55])
def test_entry_points_equal_statement(sp, ratio):
    """bff_spp_count, bff_spp_owner and bff_spp_fill one by one."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd._lib import _ptr, call
    spp, rows, n = main_case(70)
    ix = pr.index_ref(spp)
    index = sp.superpoint_index(spp, DEV)
    k, nw, s = rows.shape[0], rows.shape[1], index.n_segments
    dense = pr.unpack(rows, n)
    count_exp, need_exp = pr.count_ref(ix["seg"], s, dense), pr.need_ref(ix["size"], ratio)
    owner_exp = pr.owner_ref(count_exp, need_exp)
    r = dev_rows(rows)
    count = torch.full((k, s), 12345, dtype=torch.int32, device=DEV)        # cleared by the call
    call("bff_spp_count", _ptr(r), k, nw, n, _ptr(index.seg), s, _ptr(count))
    assert np.array_equal(count.cpu().numpy(), count_exp)
    need = index.need(ratio)
    assert np.array_equal(need.cpu().numpy(), need_exp)
    owner = torch.full((s,), 12345, dtype=torch.int32, device=DEV)
    call("bff_spp_owner", _ptr(count), k, s, _ptr(need), _ptr(owner))
    assert np.array_equal(owner.cpu().numpy(), owner_exp) and len(set(owner_exp.tolist())) >= 3
    for own in (None, owner):
        out = torch.zeros((k, nw), dtype=torch.int64, device=DEV)           # no free part: the superpoints alone
        call("bff_spp_fill", _ptr(count), k, s, _ptr(need), _ptr(own), _ptr(index.order), _ptr(index.offs), _ptr(out), nw)
        want = np.zeros((k, n), bool)
        for row in range(k):
            for j in range(s):
                if (owner_exp[j] == row) if own is not None else (count_exp[row, j] >= need_exp[j]):
                    want[row, ix["seg"] == j] = True
        assert np.array_equal(out.cpu().numpy(), pr.pack(want, nw))
    assert _lib.load().bff_abi_version() == 16


@functools.lru_cache(maxsize=None)
def big_case():
    """N = 70 000: rows of more words than one block of the count kernel covers, more superpoints than one block of the
    owner and fill kernels, one superpoint (a floor) of 6000 points."""
    rng = np.random.default_rng(34)
    n = 70_000
    spp = rng.integers(0, 3 * BLOCK_SUPERPOINTS, n) * 7919 + 5
    spp[rng.choice(n, 6000, replace=False)] = 1 << 50                       # the floor: the last superpoint
    spp[rng.choice(n, 50, replace=False)] = -1
    dense = np.stack([rng.random(n) < 0.02, rng.random(n) < 0.5, np.arange(n) % 9000 < 2500, spp == 1 << 50])
    dense[2] |= spp == 1 << 50                                              # the floor whole in two rows: exclusive -> the first
    return spp.astype(np.int64), with_garbage(pr.pack(dense, (n + 63) // 64 + 3), n), n      # three words past the cloud


@pytest.mark.parametrize("mode", MODES)
def test_more_than_one_block_covers(sp, mode):
    spp, rows, n = big_case()
    index = sp.superpoint_index(spp, DEV)
    assert (n + 63) // 64 > 4 * COUNT_BLOCK_WORDS and index.n_segments > 2 * BLOCK_SUPERPOINTS
    assert int(index.size.max()) > 64 * FILL_PASS
    for ratio in (0.02, 0.4):                 # superpoints of ~90 points: the 2 % row takes some at 0.02 and none at 0.4
        out, parent, points = check_snap(sp, index, spp, rows, n, ratio, mode)
        floor = pr.unpack(out, n)[:, spp == 1 << 50]
        # rows 2 and 3 hold the floor whole: both keep it, or the first does and row 3, left empty, is dropped
        assert parent.tolist()[-1] == (3 if mode == "snap" else 2) and floor[-1].all()
        assert (out[:, (n + 63) // 64:] == 0).all()                         # whole words past the cloud come back zero


# ------------------------------------------------------------------ exclusive
def test_exclusive(sp):
    from beyond_fixed_forms_amd import _lib
    n = 300
    spp = np.repeat([40, -1, 10, 20], [100, 50, 100, 50]).astype(np.int64)
    dense = np.zeros((4, n), bool)
    dense[0, 150:155] = dense[1, 155:164] = dense[2, 164:173] = True        # superpoint 10 claimed with 5, 9 and 9 points
    dense[:, 100:120] = True                                                # free points in every row
    dense[3, :60] = dense[1, 30:100] = True                                 # superpoint 40: 60 against 70 points
    dense[3, 250:] = True
    index = sp.superpoint_index(spp, DEV)
    out, parent, points = check_snap(sp, index, spp, pr.pack(dense), n, 0.04, "exclusive")
    got = pr.unpack(out, n)
    assert parent.tolist() == [0, 1, 2, 3]
    assert got[1, 150:250].all() and not got[[0, 2, 3], 150:250].any()     # 5, 9, 9: the second, the first of the tie
    assert got[1, :100].all() and not got[3, :100].any() and got[3, 250:].all()
    assert got[:, 100:120].all() and not got[:, 120:150].any()              # free points are still shared
    spp, rows, n = main_case(70)
    index = sp.superpoint_index(spp, DEV)
    for ratio in (1e-9, 0.5):
        rows_out, _, _ = sp.snap_rows(index, dev_rows(rows), n, ratio, "exclusive")
        taken = rows_out.clone()
        _lib.and_rows(taken, ~index.free.reshape(-1))                       # over ~free (its bits >= N are zero in the rows)
        cross = _lib.cross_popcount(taken, taken).cpu()
        assert (cross - torch.diag(torch.diag(cross))).abs().sum() == 0 and torch.diag(cross).sum() > 0
        shared = rows_out.clone()
        _lib.and_rows(shared, index.free.reshape(-1))
        assert (_lib.cross_popcount(shared, shared).cpu() - torch.diag(_lib.popcount_rows(shared).cpu())).sum() > 0


# ------------------------------------------------------------------ idempotence, reproducibility
@pytest.mark.parametrize("mode", MODES)
def test_idempotent_and_reproducible(sp, mode):
    spp, rows, n = main_case(70)
    index = sp.superpoint_index(spp, DEV)
    for ratio in (0.3, 0.5, 1.0):
        a = sp.snap_rows(index, dev_rows(rows), n, ratio, mode)
        b = sp.snap_rows(index, dev_rows(rows), n, ratio, mode)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].shape[0] > 10
        again = sp.snap_rows(index, a[0], n, ratio, mode)
        assert torch.equal(again[0], a[0]) and torch.equal(again[2], a[2])
        assert again[1].tolist() == list(range(a[0].shape[0]))


# ------------------------------------------------------------------ min_points, arguments
def test_min_points_and_arguments(sp):
    spp, rows, n = main_case(70)
    index = sp.superpoint_index(spp, DEV)
    all_rows = check_snap(sp, index, spp, rows, n, 0.5, "snap", 1)
    some = check_snap(sp, index, spp, rows, n, 0.5, "snap", 400)
    assert 0 < len(some[1]) < len(all_rows[1]) and (some[2] >= 400).all()
    assert some[1].tolist() == sorted(some[1].tolist())                     # the order is kept, parent names the input row
    keep = np.isin(all_rows[1], some[1])
    assert np.array_equal(all_rows[0][keep], some[0]) and (all_rows[2][~keep] < 400).all()
    exact = int(all_rows[2][5])
    assert all_rows[1][5] in check_snap(sp, index, spp, rows, n, 0.5, "snap", exact)[1]             # exactly min_points: kept
    assert all_rows[1][5] not in check_snap(sp, index, spp, rows, n, 0.5, "snap", exact + 1)[1]
    out, parent, points = sp.snap_rows(index, dev_rows(rows), n, 0.5, "exclusive", n + 1)           # every row dropped
    assert tuple(out.shape) == (0, rows.shape[1]) and out.is_cuda and len(parent) == 0 and len(points) == 0
    out, parent, _ = sp.snap_rows(index, torch.zeros((0, 16), dtype=torch.int64, device=DEV), n)    # K = 0
    assert tuple(out.shape) == (0, 16) and len(parent) == 0
    i0 = sp.superpoint_index(np.zeros(0, np.int64), DEV)                                            # N = 0
    assert tuple(sp.snap_rows(i0, torch.zeros((3, 0), dtype=torch.int64, device=DEV), 0)[0].shape) == (0, 0)
    free = sp.superpoint_index(np.full(n, -1), DEV)                                                 # S = 0: rows pass through
    out, _, _ = sp.snap_rows(free, dev_rows(rows), n)
    assert np.array_equal(pr.unpack(out.cpu().numpy(), n), pr.unpack(rows, n)[1:]) and (out[:, -1] >> 40 == 0).all()
    r = dev_rows(rows)
    with pytest.raises(ValueError, match="mode"):
        sp.snap_rows(index, r, n, 0.5, "largest")
    for bad in (0.0, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match="ratio"):
            sp.snap_rows(index, r, n, bad)
    with pytest.raises(ValueError, match="min_points"):
        sp.snap_rows(index, r, n, 0.5, "snap", 0)
    with pytest.raises(ValueError, match="points"):
        sp.snap_rows(index, r, n - 1)                                       # another length than the index
    with pytest.raises(ValueError, match="words"):
        sp.snap_rows(index, r[:, :15].contiguous(), n)
    with pytest.raises(ValueError, match="no CPU"):
        sp.snap_rows(index, r.cpu(), n)
    with pytest.raises(TypeError):
        sp.snap_rows(index, r.to(torch.int32), n)


def test_superpoints_from_grid(sp):
    from beyond_fixed_forms_amd import spatial
    rng = np.random.default_rng(35)
    pts = rng.uniform(0.0, 2.0, (1500, 3))
    pts[[3, 700]] = np.nan                                                  # no cell: free
    grid = spatial.voxel_grid(pts, 0.25, DEV)
    a, b = sp.superpoints_from_grid(grid), sp.superpoint_index(grid.vox)
    assert a.n_segments == grid.n_voxels and a.n_points == 1500 and torch.equal(a.seg, grid.vox)
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("ids", "seg", "order", "offs", "size", "free"))
    assert pr.unpack(a.free.cpu().numpy(), 1500)[0].nonzero()[0].tolist() == [3, 700]
    check_index(sp, grid.vox.cpu().numpy())


# ------------------------------------------------------------------ the wrapper, the tool, a generator scene
@functools.lru_cache(maxsize=None)
def scene_case():
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import project_scene
    from beyond_fixed_forms_amd.synthetic import make_scene, make_superpoints
    scene = make_scene("c1", n_views=24, distinct_masks=True, cut_masks=False)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height, snap_ratio=0.4, snap_min_points=20)
    res = project_scene(scene, cfg, device=DEV, return_result=True)
    return scene, cfg, res, make_superpoints(scene)


def test_generator_scene(sp):
    from beyond_fixed_forms_amd.synthetic import make_superpoints
    scene, cfg, res, spp = scene_case()
    n = scene.points.shape[0]
    assert spp.dtype == np.int64 and spp.shape == (n,) and spp.min() == 0 and len(np.unique(spp)) == spp.max() + 1
    assert (np.diff(spp) < 0).any() and np.array_equal(spp, make_superpoints(scene))
    obj_of = {}
    for s, o in zip(spp.tolist(), scene.point_object.tolist()):             # leak = 0: no superpoint straddles two objects
        assert obj_of.setdefault(s, o) == o
    leaky = make_superpoints(scene, leak=0.5, seed=1)
    assert len({(s, o) for s, o in zip(leaky.tolist(), scene.point_object.tolist())}) > len(np.unique(leaky))
    index = sp.superpoint_index(spp, DEV)
    rows = res.rows.cpu().numpy()
    assert rows.shape[0] >= 3 and index.n_segments > BLOCK_SUPERPOINTS
    for mode in MODES:
        check_snap(sp, index, spp, rows, n, 0.4, mode, 20)


def test_snap_instances(sp):
    scene, cfg, res, spp = scene_case()
    n = scene.points.shape[0]
    index = sp.superpoint_index(spp, DEV)
    rows = res.rows.cpu().numpy()
    exp = pr.snap_ref(spp, rows, n, 0.4, "snap", 20)
    got = sp.snap_instances(index, res, cfg)
    assert type(got) is type(res) and got is not res and res.rows.shape[0] == rows.shape[0]
    assert np.array_equal(got.rows.cpu().numpy(), exp[0]) and np.array_equal(got.parent.numpy(), exp[1]) and len(exp[1]) >= 1
    assert got.conf.dtype == res.conf.dtype and got.conf.device == res.conf.device
    assert torch.equal(got.conf.cpu(), res.conf.cpu()[torch.from_numpy(exp[1])])
    assert got.final_class == [res.final_class[i] for i in exp[1].tolist()]
    assert getattr(got, "prefetch", None) is None
    d = got.to_dict()
    assert tuple(d["ins"].shape) == (len(exp[1]), n) and np.array_equal(d["ins"].cpu().numpy(), pr.unpack(exp[0], n))
    keys = dict(cfg, snap_mode="exclusive", snap_min_points=1000)
    excl = pr.snap_ref(spp, rows, n, 0.4, "exclusive", 1000)
    listed = SimpleNamespace(rows=res.rows, conf=[float(c) for c in res.conf.cpu()], final_class=list(res.final_class))
    got = sp.snap_instances(index, listed, keys)
    assert isinstance(got.conf, list) and got.conf == [listed.conf[i] for i in excl[1].tolist()]
    assert np.array_equal(got.rows.cpu().numpy(), excl[0]) and got.parent.tolist() == excl[1].tolist()
    tensor = SimpleNamespace(rows=res.rows, conf=torch.linspace(0.1, 0.9, rows.shape[0]).to(torch.float16),
                             final_class=[f"thing {i}" for i in range(rows.shape[0])])
    got = sp.snap_instances(index, tensor, keys)
    assert got.conf.dtype == torch.float16 and torch.equal(got.conf, tensor.conf[torch.from_numpy(excl[1])])
    assert got.final_class == [f"thing {i}" for i in excl[1].tolist()]
    with pytest.raises(ValueError, match="snap_ratio"):
        sp.snap_instances(index, tensor, dict(cfg, snap_ratio=0))


def run_tool(tmp_path, *argv, **env):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "snap_instances_3d.py"), "--config",
                           str(tmp_path / "config.yaml"), *argv], cwd=tmp_path, env=dict(os.environ, **env),
                          capture_output=True, text=True, timeout=300)


def tool_tree(tmp_path, stage, spp_file):
    """A class directory of the stage with one scene and one list-valued empty form, the clouds, the superpoint files."""
    import yaml
    from beyond_fixed_forms_amd.config import Config
    scene, _, res, spp = scene_case()
    n, cls = scene.points.shape[0], "table"
    dense = pr.unpack(res.rows.cpu().numpy(), n)
    dirs = {"final": tmp_path / "final", "mask_3d": tmp_path / "m3d"}
    (dirs[stage] / cls).mkdir(parents=True)
    (tmp_path / "npy").mkdir()
    (tmp_path / "spp").mkdir()
    conf = torch.linspace(0.3, 0.8, len(dense)).to(torch.float16)
    saved = {"ins": torch.from_numpy(dense), "conf": conf, "final_class": [f"thing {i}" for i in range(len(dense))]}
    for name in ("scene_a", "scene_empty"):
        np.save(tmp_path / "npy" / f"{name}.npy", scene.points)
        torch.save(spp_file, tmp_path / "spp" / f"{name}.pth")
    torch.save(saved, dirs[stage] / cls / "scene_a.pth")
    torch.save({"ins": [], "conf": [], "final_class": []}, dirs[stage] / cls / "scene_empty.pth")
    cfg = Config.with_defaults(scene_npy_dir=str(tmp_path / "npy"), final_output_dir=str(dirs["final"]),
                               mask_3d_dir=str(dirs["mask_3d"]), snap_output_dir=str(tmp_path / "snap"),
                               superpoint_dir=str(tmp_path / "spp"), snap_ratio=0.4, snap_mode="exclusive", snap_min_points=20)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    return conf, pr.snap_ref(spp, res.rows.cpu().numpy(), n, 0.4, "exclusive", 20), n, cls


@pytest.mark.parametrize("stage,as_tensor,rle", [("final", False, False), ("mask_3d", True, True)])
def test_tool(sp, tmp_path, stage, as_tensor, rle):
    from oracle import rle_ref
    spp = scene_case()[3]
    conf, exp, n, cls = tool_tree(tmp_path, stage, torch.from_numpy(spp) if as_tensor else spp.astype(np.int32))
    r = run_tool(tmp_path, "--cls", cls, "--stage", stage, BFF_SAVE_RLE="1" if rle else "0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = torch.load(tmp_path / "snap" / cls / "scene_a.pth", weights_only=False)
    if rle:
        assert isinstance(out["ins"], list)
        ins = rle_ref.rle_decode_batch_ref(out["ins"]).bool().numpy()
    else:
        assert out["ins"].dtype == torch.bool and not out["ins"].is_cuda
        ins = out["ins"].numpy()
    assert np.array_equal(ins, pr.unpack(exp[0], n)) and len(exp[1]) >= 1
    assert np.array_equal(out["parent"].numpy(), exp[1]) and out["conf"].dtype == torch.float16
    assert torch.equal(out["conf"], conf[torch.from_numpy(exp[1])])
    assert out["final_class"] == [f"thing {i}" for i in exp[1].tolist()]
    empty = torch.load(tmp_path / "snap" / cls / "scene_empty.pth", weights_only=False)
    assert empty == {"ins": [], "conf": [], "final_class": []}


def test_tool_rejects(sp, tmp_path):
    spp = scene_case()[3]
    _, _, _, cls = tool_tree(tmp_path, "final", spp[:-1])                   # a superpoint file of another length
    r = run_tool(tmp_path, "--cls", cls)
    assert r.returncode != 0 and "ValueError" in r.stderr and "superpoint file" in r.stderr
    assert not (tmp_path / "snap" / cls / "scene_a.pth").exists()
    r = run_tool(tmp_path, "--cls", cls, "--stage", "mask_3d")              # that stage has no directory for the class
    assert r.returncode == 1 and "not a directory" in r.stderr
