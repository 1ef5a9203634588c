"""The per-scene visibility table and the sweep that reads it.

1. bff_visibility_table against its NumPy statement (tests/visibility_ref.py): bits, offsets and pixels equal, in every depth
   layout the look-up sweep accepts, with and without the culling table.
2. bff_project_views_cached against bff_project_views_lookup on the multi-frame-tile case of tests/sweep_case.py, bit for
   bit: every tile size 1 ... 8, frames in another order than the depth slots, viewed-only frames, mask frames without flag
   bit 0, views of more than 32 masks, noise masks with several runs per row.  Both also equal the case's own reference.
3. The scene call: a DeviceScene projected three times sweeps plain, cached, cached with identical results; BFF_VIS_TABLE=0
   in a fresh child stays plain; one scene on two streams builds one table.
4. Three classes of one geometry: each equals its single-class run, one table is built."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_case as sc
import visibility_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEM_LIMIT_S = 120                # a test item that is still running by then has hung: the process ends with a traceback


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


def to_dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def soa(xyz, pad=3):
    out = np.full((3, xyz.shape[0] + pad), np.nan)                   # n_pad need not be a multiple of anything
    out[:, :xyz.shape[0]] = xyz.T
    return to_dev(out)


def depth_forms(lib, raw_np, f32_np):
    """layout name -> (device frames, depth_size) for sensor frames raw uint16 [S][hs][ws] and their resized images."""
    raw = to_dev(raw_np)
    size = tuple(raw_np.shape[1:])
    return {"f32": (to_dev(f32_np.reshape(f32_np.shape[0], -1)), None), "u16rows": (raw, None),
            "u16tiles": (lib.tile_depth(raw, metres=False), size), "f32tiles": (lib.tile_depth(raw, metres=True), size)}


def table_np(tab):
    mask, off, pix = (t.cpu().numpy() for t in tab)
    return mask.view(np.uint64), off.view(np.uint32), pix.view(np.uint32)


# ------------------------------------------------------------------ 1. the table against its statement
@pytest.fixture(scope="module")
def small(lib):
    case = vr.build_case()
    exp = vr.table(case["xyz"], case["poses"], vr.K, case["depth"], vr.THRESH)
    xyz = soa(case["xyz"])
    return dict(case=case, exp=exp, xyz=xyz, poses=to_dev(case["poses"]), forms=depth_forms(lib, case["raw"], case["depth"]),
                bounds=lib.point_tile_bounds(xyz, vr.N_POINTS))


@pytest.mark.parametrize("culling", [False, True], ids=["notable", "table"])
@pytest.mark.parametrize("layout", ["f32", "u16rows", "f32tiles", "u16tiles"])
def test_table_equals_numpy_statement(lib, small, layout, culling):
    depth, size = small["forms"][layout]
    before = lib.visibility_builds()
    tab = lib.visibility_table(small["xyz"], vr.N_POINTS, small["poses"], vr.K, depth, vr.H, vr.W, vr.THRESH,
                               tile_bounds=small["bounds"] if culling else None, depth_size=size)
    assert lib.visibility_builds() == before + 1
    mask, off, pix = table_np(tab)
    emask, eoff, epix = small["exp"]
    assert mask.shape == emask.shape == (vr.N_SLOTS, lib.visibility_words(vr.N_POINTS)) == (vr.N_SLOTS, 32)
    assert epix.size > 1000 and not emask[vr.SLOT_NO_DEPTH].any() and not emask[vr.SLOT_AWAY].any()
    assert np.array_equal(mask, emask), f"bits: {int((mask != emask).sum())} words differ"
    assert np.array_equal(off, eoff), "offsets"
    assert pix.shape == epix.shape and np.array_equal(pix, epix), "pixels"
    assert lib.visibility_table_bytes(vr.N_POINTS, vr.N_SLOTS, epix.size) == (mask.nbytes, off.nbytes, epix.nbytes)


def test_table_size_limit_keeps_the_plain_sweep(lib, small):
    depth, size = small["forms"]["f32tiles"]
    args = (small["xyz"], vr.N_POINTS, small["poses"], vr.K, depth, vr.H, vr.W, vr.THRESH)
    need = sum(lib.visibility_table_bytes(vr.N_POINTS, vr.N_SLOTS, small["exp"][2].size))
    assert lib.visibility_table(*args, depth_size=size, max_bytes=need - 1) is None
    assert lib.visibility_table(*args, depth_size=size, max_bytes=need) is not None


# ------------------------------------------------------------------ 2. cached sweep = plain sweep
N = sc.N_POINTS
FILL, SENTINEL, TAIL = 7, -12345, 64


class Tiles:
    """The multi-frame-tile case on the device with its visibility table, uploaded once per module."""

    def __init__(self, lib):
        self.lib = lib
        c = self.case = sc.get()
        self.xyz = soa(c.xyz)
        self.inv_pose = to_dev(c.inv_pose.reshape(sc.N_FRAMES, 16))
        self.depth_index = to_dev(c.depth_index)
        self.flags = to_dev(c.frame_flags)
        self.depth, self.depth_size = depth_forms(lib, c.depth_raw, c.depth_f32)["f32tiles"]
        self.bounds = lib.point_tile_bounds(self.xyz, N)
        slot_pose = np.empty((sc.N_FRAMES, 16))
        slot_pose[c.depth_index] = c.inv_pose.reshape(sc.N_FRAMES, 16)         # depth_index is a permutation
        assert not np.array_equal(c.depth_index, np.arange(sc.N_FRAMES))         # frames in another order than the slots
        self.vis = lib.visibility_table(self.xyz, N, to_dev(slot_pose), sc.K, self.depth, sc.H, sc.W, sc.THRESH,
                                        tile_bounds=self.bounds, depth_size=self.depth_size)
        self.sets = {wb: self.mask_set(c.sets[wb]) for wb in (32, 64)}
        torch.cuda.synchronize()

    def mask_set(self, s):
        rs, re, offs, voffs = (to_dev(a, np.int32) for a in s.run_tables())
        tab, directory = self.lib.mask_row_directory(rs, re, offs, int(voffs[-1]), sc.H, sc.W)
        mw = s.chunk_mask.shape[1]
        return dict(s=s, runs=(rs, re, voffs), tab=tab, directory=directory, frame_mask=to_dev(s.frame_mask),
                    rowbase=to_dev(s.frame_rowbase), nmask=to_dev(s.frame_nmask), exp_rows=to_dev(s.rows),
                    exp_cmask=to_dev(s.chunk_mask), masked_at={p: to_dev(v) for p, v in s.masked_at.items()}, mw=mw)

    def sweep(self, wb, p, cached):
        d, lib = self.sets[wb], self.lib
        n_rows = int(d["s"].rows_upto[p])
        rows = torch.zeros((n_rows + 1, sc.NW), dtype=torch.int64, device=DEV)               # + one guard row
        cmask = torch.zeros((n_rows + 1, d["mw"]), dtype=torch.int64, device=DEV)
        counters = []
        for _ in range(2):
            buf = torch.full((N + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
            buf[:N] = FILL
            counters.append(buf)
        mc, vc = counters
        rs, re, voffs = d["runs"]
        frames = (d["frame_mask"][:p], d["rowbase"][:p], d["nmask"][:p], self.flags[:p])
        if cached:
            lib.project_views_cached(N, self.depth_index[:p], sc.H, sc.W, self.vis, d["tab"], d["directory"], rs, re, voffs,
                                     wb, *frames, rows[:n_rows], mc[:N], vc[:N], chunk_mask=cmask[:n_rows])
        else:
            lib.project_views_lookup(self.xyz, N, self.inv_pose[:p], sc.K, self.depth, self.depth_index[:p], sc.H, sc.W,
                                     sc.THRESH, d["tab"], d["directory"], rs, re, voffs, wb, *frames, rows[:n_rows], mc[:N],
                                     vc[:N], chunk_mask=cmask[:n_rows], tile_bounds=self.bounds, depth_size=self.depth_size)
        return rows, cmask, mc, vc


@pytest.fixture(scope="module")
def tiles(lib):
    return Tiles(lib)


def test_table_of_the_tile_case_equals_its_reference(tiles):
    """The table of 1001 slots against the case's per-frame reference (oracle.geom_fma): bits and pixels per frame."""
    c = tiles.case
    mask, off, pix = table_np(tiles.vis)
    assert pix.size == int(c.n_visible.sum()) and int(c.n_behind.sum()) > 0
    bits = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")
    for f in range(sc.N_FRAMES):
        s = c.depth_index[f]
        idx = np.flatnonzero(bits[s])
        assert np.array_equal(idx, c.vis_idx[f]), f"frame {f}: visible points"
        got = pix[off[s, 0]:off[s, 0] + idx.size].astype(np.int64)
        assert np.array_equal((got >> 16) * sc.W + (got & 0xffff), c.vis_pix[f]), f"frame {f}: pixels"


@pytest.mark.parametrize("p", sc.PREFIXES)
@pytest.mark.parametrize("wb", [32, 64])
def test_cached_sweep_equals_plain_sweep(lib, tiles, wb, p):
    assert lib.load().bff_sweep_frames_per_block(N, p) == sc.EXPECTED_FPB[sc.PREFIXES.index(p)]
    d = tiles.sets[wb]
    s = d["s"]
    fm, flags = s.frame_mask[:p], tiles.case.frame_flags[:p]
    assert (fm < 0).any() and ((fm >= 0) & (flags & 1 == 0)).any()            # viewed-only frames, mask frames that do not count
    assert wb == 32 or s.frame_nmask[:p].max() > 32
    directory = d["directory"].cpu().numpy().view(np.uint32)
    assert (directory >> 31).any()                                           # rows with several runs: the flagged entries
    plain, cached = tiles.sweep(wb, p, False), tiles.sweep(wb, p, True)
    for a, b, what in zip(plain, cached, ("rows", "chunk_mask", "masked", "viewed")):
        assert torch.equal(a, b), f"{what}: the cached sweep differs from the plain one"
    n_rows = int(s.rows_upto[p])
    rows, cmask, mc, vc = cached
    assert torch.equal(rows[:n_rows], d["exp_rows"][:n_rows]) and not rows[n_rows:].any()
    assert torch.equal(cmask[:n_rows], d["exp_cmask"][:n_rows]) and not cmask[n_rows:].any()
    assert torch.equal(mc[:N], d["masked_at"][p] + FILL) and (mc[N:] == SENTINEL).all()
    assert torch.equal(vc[:N], to_dev(tiles.case.viewed_at[p]) + FILL) and (vc[N:] == SENTINEL).all()


# ------------------------------------------------------------------ 3. the scene call
def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


def tiny(seed=11):
    from beyond_fixed_forms_amd.synthetic import make_scene
    return make_scene("tiny", seed=seed)


def snapshot(res):
    """Everything a caller of the fast path receives, as host arrays."""
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


def project_thrice(streams=None):
    """Three projections of one resident tiny scene (with its stage 1) -> ([sweep kinds], [snapshots], tables built)."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.projection import projection_back, projection_front
    from beyond_fixed_forms_amd.refinement import prepare_stage1
    from beyond_fixed_forms_amd.scene import prepare_scene
    scene = tiny()
    cfg = cfg_for(scene)
    ds = prepare_scene(scene, cfg, device=DEV)
    st1 = prepare_stage1(scene.stage1, DEV)
    torch.cuda.synchronize()
    before = _lib.visibility_builds()
    kinds, snaps = [], []
    for i in range(3):
        st = streams[i % len(streams)] if streams else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            res = projection_back(projection_front(ds, cfg, stage1=st1))
            kinds.append(res.debug["sweep"])
            snaps.append(snapshot(res))
    torch.cuda.synchronize()
    return kinds, snaps, _lib.visibility_builds() - before


def test_scene_call_plain_then_cached(lib):
    kinds, snaps, built = project_thrice()
    assert kinds == ["plain", "cached", "cached"] and built == 1
    assert snaps[0]["path"] == "fast" and snaps[0]["rows"].shape[0] > 0 and "inter" in snaps[0]
    assert_same(snaps[0], snaps[1])
    assert_same(snaps[0], snaps[2])


def test_scene_on_two_streams_builds_one_table(lib):
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    kinds, snaps, built = project_thrice(streams)
    assert kinds == ["plain", "cached", "cached"] and built == 1
    assert_same(snaps[0], snaps[1])
    assert_same(snaps[0], snaps[2])


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_visibility_table as t
kinds, snaps, built = t.project_thrice()
assert kinds == ["plain"] * 3 and built == 0, (kinds, built)
t.assert_same(snaps[0], snaps[1]); t.assert_same(snaps[0], snaps[2])
np.save(sys.argv[1], snaps[0]["rows"])
print("child ok", snaps[0]["conf"].tolist(), snaps[0]["labels"], snaps[0]["after"].tolist())
"""


def test_switched_off_in_a_fresh_process(lib, tmp_path):
    env = dict(os.environ, BFF_VIS_TABLE="0")
    out = tmp_path / "rows.npy"
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")), str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _kinds, snaps, _built = project_thrice()
    want = f"child ok {snaps[1]['conf'].tolist()} {snaps[1]['labels']} {snaps[1]['after'].tolist()}"
    assert want in r.stdout
    assert np.array_equal(np.load(out), snaps[1]["rows"])


# ------------------------------------------------------------------ 4. several classes of one geometry
def same(got: dict, exp: dict):
    assert got["ins"].dtype == exp["ins"].dtype and tuple(got["ins"].shape) == tuple(exp["ins"].shape)
    assert torch.equal(got["ins"].cpu(), exp["ins"].cpu())
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"].cpu())
    assert list(got["final_class"]) == list(exp["final_class"])


def test_three_classes_share_one_table(lib):
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes
    from beyond_fixed_forms_amd.synthetic import class_scene, derive_classes
    scene = tiny(seed=5)
    cfg = cfg_for(scene)
    masks = derive_classes(scene, k=3, fraction=0.6, seed=3)
    assert len(masks) == 3
    exp = {c: project_scene(class_scene(scene, m), cfg, DEV) for c, m in masks.items()}       # one visit each: plain
    torch.cuda.synchronize()
    before = lib.visibility_builds()
    got = project_scene_classes(scene, masks, cfg, DEV, return_result=True)
    assert lib.visibility_builds() == before + 1
    assert [got[c].debug["sweep"] for c in masks] == ["plain", "cached", "cached"]
    for c in masks:
        same(got[c].to_dict(), exp[c])
