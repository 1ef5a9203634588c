"""The run-major cached sweep (bff_project_views_runs) and the pixel-sorted companion of the visibility table it walks.

1. bff_visibility_sorted against its NumPy statement (tests/visibility_sorted_ref.py) on the small case.
2. bff_project_views_runs against bff_project_views_cached and the multi-frame-tile case's own reference
   (tests/sweep_case.py), bit for bit, word_bits 32 and 64, every prefix: frames in another order than the slots, viewed-only
   frames, mask frames without flag bit 0, views of more than 32 masks, rows with several runs.
3. Hand-made masks over the 24 x 32 case against a brute-force membership: a run across a row end, one run over the whole
   image, one-pixel runs at both ends, a mask without runs between two with runs, a mask that hits nothing, two identical
   masks; N = 1500, 1100 (nw = 18: no multiple of 4 or of a chunk's 8 words) and 1.
4. The LDS bound, lowered through the environment: the scene call reports the point-major form, results equal.
5. The scene call with BFF_SWEEP_RUNS=0 in a fresh child: the same snapshots as the default run."""
import faulthandler
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_case as sc
import test_gpu_visibility_table as vt
import visibility_ref as vr
import visibility_sorted_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEM_LIMIT_S = 120
FILL, SENTINEL, TAIL = 7, -12345, 64
to_dev, soa = vt.to_dev, vt.soa


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(ITEM_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def counters(n):
    out = []
    for _ in range(2):
        buf = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
        buf[:n] = FILL
        out.append(buf)
    return out


# ------------------------------------------------------------------ 1. the companion against its statement
@pytest.fixture(scope="module")
def small(lib):
    case = vr.build_case()
    return dict(case=case, forms=vt.depth_forms(lib, case["raw"], case["depth"]))


def small_table(lib, small, xyz_np):
    """(host table, device table, device companion, pairs) of the small case's slots for the cloud xyz_np."""
    case, n = small["case"], xyz_np.shape[0]
    exp = vr.table(xyz_np, case["poses"], vr.K, case["depth"], vr.THRESH)
    depth, size = small["forms"]["f32tiles"]
    tab = lib.visibility_table(soa(xyz_np), n, to_dev(case["poses"]), vr.K, depth, vr.H, vr.W, vr.THRESH, depth_size=size)
    pairs = int(exp[2].size)
    assert np.array_equal(u32(tab[2])[:pairs], exp[2])
    return exp, tab, lib.visibility_sorted(tab, pairs, n, vr.H, vr.W), pairs


def test_companion_equals_numpy_statement(lib, small):
    exp, _tab, comp, pairs = small_table(lib, small, small["case"]["xyz"])
    espix, espt, erow = sr.companion(*exp, vr.H, vr.W)
    spix, spt, rowstart = (u32(t) for t in comp)
    assert pairs > 1000 and rowstart.shape == erow.shape
    assert np.array_equal(spix[:pairs], espix), "pixels"
    assert np.array_equal(spt[:pairs], espt), "points"
    assert np.array_equal(rowstart, erow), "row starts"
    assert lib.visibility_sorted_bytes(vr.N_SLOTS, vr.H, pairs) == (espix.nbytes, espt.nbytes, erow.nbytes)
    assert lib.sorted_temp_bytes >= 12 * pairs


# ------------------------------------------------------------------ 2. run-major = point-major = the case's reference
N = sc.N_POINTS


class RunTiles(vt.Tiles):
    """The multi-frame-tile case with the companion of its table and the masks' run offsets."""

    def __init__(self, lib):
        super().__init__(lib)
        self.sorted = lib.visibility_sorted(self.vis, int(self.vis[2].shape[0]), N, sc.H, sc.W)
        self.offs = {wb: to_dev(self.case.sets[wb].run_tables()[2], np.int32) for wb in (32, 64)}
        torch.cuda.synchronize()

    def sweep_runs(self, wb, p):
        d = self.sets[wb]
        n_rows = int(d["s"].rows_upto[p])
        rows = torch.zeros((n_rows + 1, sc.NW), dtype=torch.int64, device=DEV)               # + one guard row
        cmask = torch.zeros((n_rows + 1, d["mw"]), dtype=torch.int64, device=DEV)
        mc, vc = counters(N)
        rs, re, voffs = d["runs"]
        self.lib.project_views_runs(N, self.depth_index[:p], sc.H, sc.W, self.vis, self.sorted, rs, re, self.offs[wb], voffs,
                                    wb, d["frame_mask"][:p], d["rowbase"][:p], d["nmask"][:p], self.flags[:p], rows[:n_rows],
                                    mc[:N], vc[:N], cmask[:n_rows])
        return rows, cmask, mc, vc


@pytest.fixture(scope="module")
def tiles(lib):
    return RunTiles(lib)


@pytest.mark.parametrize("p", sc.PREFIXES)
@pytest.mark.parametrize("wb", [32, 64])
def test_runs_sweep_equals_points_sweep(lib, tiles, wb, p):
    assert lib.sweep_runs_ok(N)
    d = tiles.sets[wb]
    s = d["s"]
    fm, flags = s.frame_mask[:p], tiles.case.frame_flags[:p]
    assert (fm < 0).any() and ((fm >= 0) & (flags & 1 == 0)).any()            # viewed-only frames, mask frames that do not count
    assert wb == 32 or s.frame_nmask[:p].max() > 32
    assert not np.array_equal(tiles.case.depth_index, np.arange(sc.N_FRAMES))
    offs = s.run_tables()[2]
    assert np.diff(offs).max() > sc.H                                         # rows with several runs
    points, runs = tiles.sweep(wb, p, True), tiles.sweep_runs(wb, p)
    for a, b, what in zip(points, runs, ("rows", "chunk_mask", "masked", "viewed")):
        assert torch.equal(a, b), f"{what}: the run-major sweep differs from the point-major one"
    n_rows = int(s.rows_upto[p])
    rows, cmask, mc, vc = runs
    assert torch.equal(rows[:n_rows], d["exp_rows"][:n_rows]) and not rows[n_rows:].any()
    assert torch.equal(cmask[:n_rows], d["exp_cmask"][:n_rows]) and not cmask[n_rows:].any()
    assert torch.equal(mc[:N], d["masked_at"][p] + FILL) and (mc[N:] == SENTINEL).all()
    assert torch.equal(vc[:N], to_dev(tiles.case.viewed_at[p]) + FILL) and (vc[N:] == SENTINEL).all()


# ------------------------------------------------------------------ 3. hand-made masks against brute force
HW, DEPTH_INDEX, FRAME_MASK, FRAME_FLAGS, hand_masks = sr.HW, sr.DEPTH_INDEX, sr.FRAME_MASK, sr.FRAME_FLAGS, sr.hand_masks


@pytest.mark.parametrize("n", [1500, 1100, 1])
def test_hand_made_masks_equal_brute_force(lib, small, n):
    case = small["case"]
    full = case["xyz"]
    if n == 1:      # one point that slot 0 sees
        vis0 = vr.frame_visibility(full, case["poses"][0], vr.K, case["depth"][0], vr.THRESH)[0]
        xyz = full[np.flatnonzero(vis0)[:1]]
    else:
        xyz = full[:n]
    nw = (n + 63) // 64
    assert n != 1100 or (nw == 18 and nw % 4 and nw % 8)
    seen = np.zeros(HW, bool)
    for s in range(vr.N_SLOTS):
        vis, u, v, _why = vr.frame_visibility(xyz, case["poses"][s], vr.K, case["depth"][s], vr.THRESH)
        seen[(v * vr.W + u)[vis]] = True
    assert seen.any() and not seen.all()
    runs = hand_masks(int(np.flatnonzero(~seen)[0]))
    m = len(runs)
    cover = sr.dense_masks(runs, HW)
    e_rows, e_cmask, e_masked, e_viewed = sr.membership_sweep(xyz, case["poses"], vr.K, case["depth"], vr.THRESH, DEPTH_INDEX,
                                                              FRAME_MASK, FRAME_FLAGS, cover)
    n_rows = e_rows.shape[0]
    assert n_rows == 6 * m and not e_rows[6::m].any() and not e_rows[4::m].any()      # the miss and the mask without runs
    assert n == 1 or (e_rows[0::m].any() and e_rows[2::m].any() and np.array_equal(e_rows[7::m], e_rows[8::m]))
    assert e_rows[1::m].any() and e_viewed.any() and e_masked.any()

    _exp, tab, comp, _pairs = small_table(lib, small, xyz)
    rs, re, offs = (to_dev(a) for a in sr.run_tables(runs))
    voffs = to_dev(np.array([0, m], np.int32))
    rowbase = to_dev((np.cumsum(np.where(FRAME_MASK >= 0, m, 0)) - np.where(FRAME_MASK >= 0, m, 0)).astype(np.int32))
    nmask = to_dev(np.where(FRAME_MASK >= 0, m, 0).astype(np.int32))
    rows = torch.zeros((n_rows + 1, nw), dtype=torch.int64, device=DEV)
    cmask = torch.zeros((n_rows + 1, e_cmask.shape[1]), dtype=torch.int64, device=DEV)
    mc, vc = counters(n)
    lib.project_views_runs(n, to_dev(DEPTH_INDEX), vr.H, vr.W, tab, comp, rs, re, offs, voffs, 32, to_dev(FRAME_MASK), rowbase,
                           nmask, to_dev(FRAME_FLAGS), rows[:n_rows], mc[:n], vc[:n], cmask[:n_rows])
    assert torch.equal(rows[:n_rows], to_dev(e_rows)) and not rows[n_rows:].any()
    assert torch.equal(cmask[:n_rows], to_dev(e_cmask)) and not cmask[n_rows:].any()
    assert torch.equal(mc[:n], to_dev(e_masked) + FILL) and (mc[n:] == SENTINEL).all()
    assert torch.equal(vc[:n], to_dev(e_viewed) + FILL) and (vc[n:] == SENTINEL).all()


# ------------------------------------------------------------------ 4. / 5. the scene call
def snapshot(res):
    """Everything a caller of the fast path receives, as host arrays (as test_gpu_visibility_table.snapshot)."""
    out = dict(rows=res.rows.cpu().numpy(), conf=res.conf.cpu().numpy(), labels=list(res.final_class),
               before=res.debug["before"].numpy(), after=res.debug["after"].numpy(), keep=res.debug["keep"].numpy(),
               thr=res.debug.get("thr"), path=res.debug["path"])
    if res.prefetch is not None:
        out.update({k: np.asarray(res.prefetch[k]) for k in ("area1", "area2", "inter", "inter11")},
                   s1=res.prefetch["s1"].cpu().numpy())
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def project_thrice():
    """Three projections of one resident tiny scene (with its stage 1) -> ([(sweep, form)], [snapshots])."""
    from beyond_fixed_forms_amd.projection import projection_back, projection_front
    from beyond_fixed_forms_amd.refinement import prepare_stage1
    from beyond_fixed_forms_amd.scene import prepare_scene
    scene = vt.tiny()
    cfg = vt.cfg_for(scene)
    ds = prepare_scene(scene, cfg, device=DEV)
    st1 = prepare_stage1(scene.stage1, DEV)
    kinds, snaps = [], []
    for _ in range(3):
        res = projection_back(projection_front(ds, cfg, stage1=st1))
        kinds.append((res.debug["sweep"], res.debug.get("sweep_form")))
        snaps.append(snapshot(res))
    torch.cuda.synchronize()
    return kinds, snaps


@pytest.fixture(scope="module")
def default_run(lib):
    assert "BFF_SWEEP_RUNS" not in os.environ and "BFF_SWEEP_RUNS_LDS_BYTES" not in os.environ
    kinds, snaps = project_thrice()
    assert kinds == [("plain", None), ("cached", "runs"), ("cached", "runs")]
    assert snaps[0]["path"] == "fast" and snaps[0]["rows"].shape[0] > 0 and "inter" in snaps[0]
    assert_same(snaps[0], snaps[1])
    assert_same(snaps[0], snaps[2])
    return snaps


def test_scene_over_the_lds_bound_keeps_the_points_form(lib, default_run, monkeypatch):
    monkeypatch.setenv("BFF_SWEEP_RUNS_LDS_BYTES", "8")           # read per call: no row fits
    kinds, snaps = project_thrice()
    assert kinds == [("plain", None), ("cached", "points"), ("cached", "points")]
    for s in snaps:
        assert_same(default_run[1], s)


CHILD = """
import pickle, sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_sweep_runs as t
kinds, snaps = t.project_thrice()
assert kinds == [("plain", None), ("cached", "points"), ("cached", "points")], kinds
with open(sys.argv[1], "wb") as f:
    pickle.dump(snaps, f)
print("child ok")
"""


def test_switched_off_in_a_fresh_process(lib, default_run, tmp_path):
    env = dict(os.environ, BFF_SWEEP_RUNS="0")
    out = tmp_path / "snaps.pkl"
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")), str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-3000:]
    with open(out, "rb") as f:
        snaps = pickle.load(f)
    for s in snaps:
        assert_same(default_run[1], s)
