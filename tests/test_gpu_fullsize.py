"""GPU parity at BASELINE config 2's full size (200k points, 300 views @968x1296, 30 masks/view,
Ins = 9000) through size-independent properties, plus the oracle on a frame subset at full N / HxW / M.
The complete oracle run at this size (~40 s of CPU on 16 threads) is part of the suite, and so are two more on the
scenes and the depth format the benchmark times (test_timed_configuration_against_the_complete_oracle: 41 s for the
"default" and 41 s for the "many" variant on 16 threads, measured next to an MI355X); set BFF_SKIP_FULL_SCALE=1 to
leave all three out.  The timed scenes are projected three times each, so that the cached sweeps the benchmark runs are
held against the oracle-checked plain one (test_timed_configuration_sweeps_cached_with_the_same_result)."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import projection_ref as pref, refinement_ref as rref
from test_gpu_sweep_runs import assert_same, snapshot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def c2():
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import make_scene
    _lib.load()
    scene = make_scene("c2", seed=0, device=DEV)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
    return scene, cfg, prepare_scene(scene, cfg, device=DEV)


def bits(rows, n):
    return np.unpackbits(rows.cpu().numpy().view(np.uint8), axis=-1, bitorder="little")[:, :n].astype(bool)


def test_checksums_and_layout_invariance(c2):
    """(a) every set instance bit is one vote: sum of row popcounts == sum of masked_count;
    (b) the Morton-sorted layout and the caller's point order give identical results;
    (c) one fused sweep == a mask sweep followed by a separate viewed sweep (what the reference does)."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene
    scene, cfg, ds = c2
    res = run_projection(ds, cfg, debug_out=True)
    raw, masked, viewed = res.debug["raw_rows"], res.debug["masked_counts_raw"], res.debug["viewed_counts"]
    assert int(_lib.popcount_rows(raw).sum().item()) == int(masked.sum().item()) > 10 ** 6
    assert int(viewed.max().item()) <= ds.n_viewed and int(masked.max().item()) <= ds.n_rows
    ds_plain = prepare_scene(scene, cfg, device=DEV, sort_points=False)
    res2 = run_projection(ds_plain, cfg, debug_out=True)
    assert torch.equal(res2.debug["raw_rows"], raw) and torch.equal(res2.debug["masked_counts_raw"], masked)
    assert torch.equal(res2.debug["viewed_counts"], viewed)
    assert res2.groups == res.groups and torch.equal(res2.rows, res.rows) and torch.equal(res2.conf, res.conf)
    # separate sweeps on the unsorted layout
    n = ds_plain.n_points
    mb = torch.empty((ds_plain.n_mask_frames, ds_plain.height * ds_plain.width), dtype=torch.int32, device=DEV)
    _lib.rle_to_maskbits(ds_plain.run_start, ds_plain.run_end, ds_plain.mask_run_offs, ds_plain.view_mask_offs,
                         ds_plain.n_mask_frames, ds_plain.height * ds_plain.width, 32, mb)
    rows_a = torch.zeros_like(raw)
    m_a = torch.zeros(n, dtype=torch.int32, device=DEV)
    v_a = torch.zeros(n, dtype=torch.int32, device=DEV)
    zero_flags = torch.zeros_like(ds_plain.frame_flags)
    _lib.project_views(ds_plain.xyz, n, ds_plain.inv_pose, ds_plain.cam_intr, ds_plain.depth, ds_plain.depth_index,
                       ds_plain.height, ds_plain.width, 0.08, mb, 32, ds_plain.frame_mask, ds_plain.frame_rowbase,
                       ds_plain.frame_nmask, zero_flags, rows_a, m_a, None)          # full images, no segment bitmap
    _lib.project_views(ds_plain.xyz, n, ds_plain.inv_pose, ds_plain.cam_intr, ds_plain.depth, ds_plain.depth_index,
                       ds_plain.height, ds_plain.width, 0.08, None, 32, ds_plain.frame_mask, ds_plain.frame_rowbase,
                       ds_plain.frame_nmask, torch.ones_like(zero_flags), None, None, v_a)
    assert torch.equal(rows_a, raw) and torch.equal(m_a, masked) and torch.equal(v_a, viewed)


def test_raw_depth_in_the_sweep_equals_the_resize_pass(c2):
    """Config 2 with the depth frames resident as 16-bit half-resolution images (the stored format, P:431-436): the
    sweep's per-point /1000 + bilinear resize gives rows and counters bit-identical to the separate resize pass
    into float32 (H, W) images followed by the float32 sweep."""
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene
    from beyond_fixed_forms_amd.synthetic import with_sensor_depth
    scene, cfg, _ = c2
    raw = with_sensor_depth(scene)
    a = run_projection(prepare_scene(raw, cfg, device=DEV, raw_depth_resident=True), cfg, debug_out=True)
    b = run_projection(prepare_scene(raw, cfg, device=DEV, raw_depth_resident=False), cfg, debug_out=True)
    for k in ("raw_rows", "masked_counts_raw", "viewed_counts"):
        assert torch.equal(a.debug[k], b.debug[k]), k
    assert int(a.debug["masked_counts_raw"].sum().item()) > 10 ** 6
    assert a.groups == b.groups and torch.equal(a.rows, b.rows) and torch.equal(a.conf, b.conf)


def test_components_two_formulations_agree(c2):
    """Union-find tile pass (production) == adjacency matrix + label propagation (cross-check), Ins = 9000."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.projection import groups_from_labels, run_projection
    scene, cfg, ds = c2
    res = run_projection(ds, cfg, debug_out=True)
    rows = res.debug["raw_rows"]
    area, _mw, cmask, hist, sig = _lib.row_stats(rows)
    order = torch.argsort(sig, stable=True).to(torch.int32)
    comp = _lib.merge_components(rows, area, ds.label_id, cfg.iou_thres, order, cmask, hist).cpu().numpy()
    adj = _lib.merge_adjacency(rows, area, ds.label_id, cfg.iou_thres)                      # dense, identity order
    lab = _lib.components(adj).cpu().numpy()
    self_loop = area.cpu().numpy() > 0
    assert groups_from_labels(comp, self_loop, 2) == groups_from_labels(lab, self_loop, 2) == list(res.groups)


def test_decode_checksum(c2):
    """Mask-word images: per mask, the number of pixels with its bit set == the total run length of its RLE."""
    from beyond_fixed_forms_amd import _lib
    scene, cfg, ds = c2
    hw = ds.height * ds.width
    nv = 8
    mb = torch.empty((nv, hw), dtype=torch.int32, device=DEV)
    _lib.rle_to_maskbits(ds.run_start, ds.run_end, ds.mask_run_offs, ds.view_mask_offs, nv, hw, 32, mb)
    run_len = (ds.run_end - ds.run_start).cpu().numpy().astype(np.int64)
    offs = ds.mask_run_offs.cpu().numpy()
    voffs = ds.view_mask_offs.cpu().numpy()
    for v in range(nv):
        img = mb[v].cpu().numpy().view(np.uint32)
        for b in range(voffs[v + 1] - voffs[v]):
            g = voffs[v] + b
            assert int(((img >> np.uint32(b)) & 1).sum()) == int(run_len[offs[g]:offs[g + 1]].sum()), (v, b)
        assert not (img >> np.uint32(voffs[v + 1] - voffs[v])).any()


def test_oracle_on_a_frame_subset_at_full_size(c2):
    """Oracle (CPU) on 3 of the 300 frames at full N / HxW / M: raw instance rows and both vote counters of
    the HIP sweep are bit-identical."""
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene
    scene, cfg, _ = c2
    sub = copy.copy(scene)
    sub.mask_2d = [dict(f) for f in scene.mask_2d[100:103]]
    keep = {int(f["frame_id"][:-4]) for f in sub.mask_2d}
    sub.color_files = [f"{i}.jpg" for i in sorted(keep)]
    cfg1 = type(cfg)(cfg); cfg1["downsample_ratio"] = 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp, dbg = pref.project_scene_ref(sub, cfg1, return_debug=True)
    res = run_projection(prepare_scene(sub, cfg1, device=DEV), cfg1, debug_out=True)
    n = scene.points.shape[0]
    assert np.array_equal(bits(res.debug["raw_rows"], n), dbg["raw_ins"].numpy())
    assert np.array_equal(res.debug["masked_counts_raw"].cpu().numpy(), dbg["masked_counts_raw"].numpy().astype(np.int32))
    assert np.array_equal(res.debug["viewed_counts"].cpu().numpy(), dbg["viewed_counts"].numpy().astype(np.int32))
    assert list(res.groups) == dbg["groups"]
    got = res.to_dict()
    assert tuple(got["ins"].shape) == tuple(exp["ins"].shape) and torch.equal(got["ins"].cpu(), exp["ins"])
    assert torch.equal(got["conf"].cpu(), exp["conf"])


@pytest.mark.skipif(os.environ.get("BFF_SKIP_FULL_SCALE") == "1", reason="~40 s of CPU; skipped on request")
def test_complete_oracle_at_config2(c2):
    """The whole path at config 2 against the oracle: stage-2 and final masks bit-identical."""
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.refinement import TextSimilarity, refine_class
    from beyond_fixed_forms_amd.synthetic import make_text_bank
    from oracle.make_golden_shared import bank_encoder
    scene, cfg, ds = c2
    torch.set_num_threads(16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp, dbg = pref.project_scene_ref(scene, cfg, return_debug=True)
    res = run_projection(ds, cfg)
    assert list(res.groups) == dbg["groups"]
    got = res.to_dict()
    assert tuple(got["ins"].shape) == tuple(exp["ins"].shape) and torch.equal(got["ins"].cpu(), exp["ins"])
    assert torch.equal(got["conf"].cpu(), exp["conf"]) and got["final_class"] == exp["final_class"]
    bank, index = make_text_bank(768, seed=0)
    enc = bank_encoder(bank.float(), index)
    fin = refine_class([(scene.scene_id, scene.stage1, res)], cfg, "table", TextSimilarity(enc, DEV), DEV)
    fexp = rref.refine_class_ref([(scene.scene_id, scene.stage1, exp)], cfg, "table", enc)
    fd = fin[scene.scene_id].to_dict()
    assert torch.equal(fd["ins"].cpu(), fexp[scene.scene_id]["ins"]) and torch.equal(fd["conf"], fexp[scene.scene_id]["conf"])


# The scenes bench.py rotates through its timed loop ("default" / "many" of its SCENE_VARIANTS; seeds as its first
# rank's first two scenes): the generator's default, and 40 smaller objects with one exact full-silhouette mask per
# visible object and view, where many stage-2 instances survive the filters (K >> 1 through the back half).
TIMED_VARIANTS = {
    "default": dict(seed=0),
    "many": dict(seed=1, cut_masks=False, n_objects=40, distinct_masks=True, dilate=False),
}
_timed = {}


def timed_device(variant):
    """The device half of one variant in the timed configuration -- 16-bit depth at the sensor's resolution
    (with_sensor_depth), ingested by prepare_scene_fast -- projected THREE times by the one-call path from one resident
    DeviceScene, as the benchmark's loop does: the first projection sweeps plain, the later ones from the scene's
    visibility table.  -> (scene, cfg, raw, first result, [(sweep, form)], [snapshots]).  Computed once per module run."""
    key = ("device", variant)
    if key not in _timed:
        from beyond_fixed_forms_amd import _lib
        from beyond_fixed_forms_amd.config import Config
        from beyond_fixed_forms_amd.ingest import prepare_scene_fast
        from beyond_fixed_forms_amd.projection import projection_back, projection_front
        from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth
        _lib.load()
        scene = make_scene("c2", device=DEV, **TIMED_VARIANTS[variant])
        scene.scene_id = f"scene_{variant}"
        cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
        raw = with_sensor_depth(scene)
        ds = prepare_scene_fast(raw, cfg, DEV)
        first, kinds, snaps = None, [], []
        for _ in range(3):
            res = projection_back(projection_front(ds, cfg))
            first = res if first is None else first
            kinds.append((res.debug["sweep"], res.debug.get("sweep_form")))
            snaps.append(snapshot(res))
        torch.cuda.synchronize()
        _timed[key] = (scene, cfg, raw, first, kinds, snaps)
    return _timed[key]


def timed_run(variant):
    """One variant in the timed configuration (timed_device: its first, plain-sweep projection) next to the oracle on the
    host restatement of the resize.  Computed once per module run: the joint refinement needs both variants."""
    if variant not in _timed:
        import time
        from beyond_fixed_forms_amd.io import resize_bilinear_f32
        scene, cfg, raw, res, _kinds, _snaps = timed_device(variant)
        host = copy.copy(scene)               # what the reference holds after cv2.imread / 1000 + cv2.resize (restated)
        host.depths = {f: resize_bilinear_f32(m.astype(np.float32) / np.float32(1000), scene.width, scene.height)
                       for f, m in raw.depths_raw.items()}
        torch.set_num_threads(16)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp, dbg = pref.project_scene_ref(host, cfg, return_debug=True)
        print(f"oracle on the {variant} variant: {time.perf_counter() - t0:.1f} s, {len(dbg['groups'])} groups, "
              f"{len(exp['conf'])} stage-2 instances")
        _timed[variant] = (scene, cfg, exp, dbg, res)
    return _timed[variant]


def timed_refinement():
    """Both variants' results refined TOGETHER, as one class (a batch of two scenes, as the bench batches eight): the
    similarity percentile of R:324 is taken over the class, so neither scene's final masks can be checked alone."""
    if "final" not in _timed:
        from beyond_fixed_forms_amd.refinement import TextSimilarity, refine_class
        from beyond_fixed_forms_amd.synthetic import make_text_bank
        from oracle.make_golden_shared import bank_encoder
        runs = [timed_run(v) for v in TIMED_VARIANTS]
        cfg = runs[0][1]
        bank, index = make_text_bank(768, seed=0)
        enc = bank_encoder(bank.float(), index)
        fin = refine_class([(sc.scene_id, sc.stage1, res) for sc, _c, _e, _d, res in runs], cfg, "table", TextSimilarity(enc, DEV), DEV)
        fexp = rref.refine_class_ref([(sc.scene_id, sc.stage1, exp) for sc, _c, exp, _d, _r in runs], cfg, "table", enc)
        _timed["final"] = (fin, fexp)
    return _timed["final"]


@pytest.mark.skipif(os.environ.get("BFF_SKIP_FULL_SCALE") == "1", reason="two complete oracle runs at config 2; skipped on request")
@pytest.mark.parametrize("variant", list(TIMED_VARIANTS))
def test_timed_configuration_against_the_complete_oracle(variant):
    """The configuration the headline number is printed on -- config 2, depth as 16-bit half-resolution frames resized
    per point inside the sweep, prepare_scene_fast, the one-call path -- on both scene variants of the benchmark against
    the complete oracle: groups, stage-2 masks, confidences and labels bit-identical, and the final masks of both scenes
    refined as one class equal refine_class_ref's.
    "many" is there for K >> 1: the oracle returns 3 stage-2 instances on "default" and 25 on "many" (of 40 objects)."""
    scene, cfg, exp, dbg, res = timed_run(variant)
    assert res.debug["path"] == "fast"                    # otherwise this checks another path than the timed one
    assert list(res.groups) == dbg["groups"]
    got = res.to_dict()
    assert tuple(got["ins"].shape) == tuple(exp["ins"].shape) and torch.equal(got["ins"].cpu(), exp["ins"])
    assert torch.equal(got["conf"].cpu(), exp["conf"]) and got["final_class"] == exp["final_class"]
    k_default, k_many = (len(timed_run(v)[2]["conf"]) for v in ("default", "many"))
    # a condition on the input, not a measurement: "many" must put many instances through the back half -- at least half
    # of its 40 objects, and several times what the default scene leaves
    assert k_default >= 1 and k_many >= 20 and k_many >= 5 * k_default, (k_default, k_many)
    fin, fexp = timed_refinement()
    fd, fe = fin[scene.scene_id].to_dict(), fexp[scene.scene_id]
    assert not isinstance(fe["ins"], list) and fe["ins"].shape[0] >= 1
    assert tuple(fd["ins"].shape) == tuple(fe["ins"].shape) and torch.equal(fd["ins"].cpu(), fe["ins"])
    assert torch.equal(fd["conf"].cpu(), fe["conf"].cpu()) and list(fd["final_class"]) == list(fe["final_class"])


@pytest.mark.parametrize("variant", list(TIMED_VARIANTS))
def test_timed_configuration_sweeps_cached_with_the_same_result(variant):
    """What the benchmark times is the SECOND and later projection of a resident scene: the run-major cached sweep
    (200 000 points: an instance row fits the LDS bound).  At 968 x 1296, 300 frames and 200 000 points the three
    projections of one DeviceScene report plain, cached / runs, cached / runs, and everything a caller receives from the
    cached ones -- rows, confidences, labels, the filters' counts -- equals the plain one, which
    test_timed_configuration_against_the_complete_oracle holds against the oracle.  Needs no oracle itself."""
    _scene, _cfg, _raw, first, kinds, snaps = timed_device(variant)
    assert kinds == [("plain", None), ("cached", "runs"), ("cached", "runs")]
    assert first.debug["path"] == "fast" and snaps[0]["path"] == "fast" and snaps[0]["rows"].shape[0] >= 1
    assert_same(snaps[0], snaps[1])
    assert_same(snaps[0], snaps[2])
