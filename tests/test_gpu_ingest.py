"""The ingestion path in front of the kernels, on the GPU: host files -> a resident DeviceScene.

A. Depth frames that io.load_scene(staging=...) decoded into the loader's pinned buffer in ITS order, uploaded in the
   order prepare_scene_fast's slots want (the two differ as soon as a mask_2d entry has no masks): every table and the
   depth itself against scene.prepare_scene of the same files loaded without staging, results against the oracle.
B. bff_cloud_layout, bff_point_tile_bounds, bff_depth_tile_u16 and bff_depth_from_u16 against NumPy, at the sizes and
   values where such kernels go wrong (n around the 1024 granule, strides, non-finite coordinates, degenerate boxes,
   frames whose last tile is partial, stored depth of 32768 mm and more), and depth beyond 32.767 m through the sweep
   in all four depth forms against the oracle.

Every comparison is bit for bit.  References: NumPy in float64 / exact integers, the oracle, and io.resize_bilinear_f32
as the stand-in for cv2.resize (parity with cv2 itself is unpinned, here as everywhere in the suite)."""
import copy
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLS = "table"


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib, ingest
    ingest.host_lib()
    _lib.load()
    return _lib


def same(got: dict, exp: dict):
    """Bit-identical masks, identical conf values+dtype, identical labels, identical empty forms."""
    if isinstance(exp["ins"], list):
        assert isinstance(got["ins"], list) and got["ins"] == [] and got["conf"] == [] and got["final_class"] == []
        return
    assert got["ins"].dtype == exp["ins"].dtype and tuple(got["ins"].shape) == tuple(exp["ins"].shape)
    assert torch.equal(got["ins"].cpu(), exp["ins"])
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"])
    assert list(got["final_class"]) == list(exp["final_class"])


def oracle(scene, cfg, debug=False):
    """The oracle on a scene.  mask_2d entries without masks are left out of ITS list: the reference's decoder cannot
    stack zero masks (rle_encode_decode.py:35-61 raises), and its own 2-D stage never writes such an entry; for the
    device path such a frame carries no rows and no votes, which is what leaving it out means."""
    if any(len(fr["segmented_frame_masks"]) == 0 for fr in scene.mask_2d):
        scene = copy.copy(scene)
        scene.mask_2d = [fr for fr in scene.mask_2d if len(fr["segmented_frame_masks"])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return pref.project_scene_ref(scene, cfg, return_debug=debug)


# ------------------------------------------------------------------ A. staged depth in another order than the upload's
def sensor_frames(scene, factor=2):
    """The scene's depth as a sensor of 1/factor of the working resolution stores it: uint16 millimetres per frame id."""
    return {f: np.ascontiguousarray(np.round(d[::factor, ::factor].astype(np.float64) * 1000.0).astype(np.uint16))
            for f, d in scene.depths.items()}


def write_scene(root, scene, masks, frames_mm):
    """The reference's directory layout for one scene: masks = {class: mask_2d list}, frames_mm = {frame id: uint16}."""
    from PIL import Image
    sd = root / "2d" / scene.scene_id
    for sub in ("intrinsic", "pose", "depth", "color"):
        (sd / sub).mkdir(parents=True, exist_ok=True)
    (root / "npy").mkdir(parents=True, exist_ok=True)
    np.savetxt(sd / "intrinsic" / "intrinsic_color.txt", scene.cam_intr)
    np.save(root / "npy" / f"{scene.scene_id}.npy", scene.points)
    for f in scene.color_files:
        (sd / "color" / f).write_bytes(b"")
    for fid, pose in scene.poses.items():
        np.savetxt(sd / "pose" / f"{fid}.txt", pose)
        Image.fromarray(frames_mm[fid]).save(sd / "depth" / f"{fid}.png")
    for cls, m in masks.items():
        (root / "m2d" / cls).mkdir(parents=True, exist_ok=True)
        torch.save(m, root / "m2d" / cls / f"{scene.scene_id}.pth")


def disk_cfg(root, scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, scene_2d_dir=str(root / "2d"),
                                scene_npy_dir=str(root / "npy"), mask_2d_dir=str(root / "m2d"), **over)


def no_masks(fr):
    """A mask_2d entry of a frame the detector found nothing in."""
    return dict(fr, segmented_frame_masks=[], confidences=fr["confidences"][:0], labels=[])


def edit_masks(mask_2d, empty=(), repeat=None):
    out = [no_masks(fr) if k in empty else fr for k, fr in enumerate(mask_2d)]
    if repeat is not None:                               # (entry, position): the same frame id a second time
        out.insert(repeat[1], dict(mask_2d[repeat[0]]))
    return out


STAGED_CASES = {
    # name: (mask_2d edits, config overrides).  Frame ids are "0", "10", ..., "230"; with downsample_ratio 10 all of
    # them are frames of the detection-ratio sweep, with 20 every other one is.
    # entry 1 is empty and a viewed frame: its slot moves behind the mask frames'.  Fails deterministically on a
    # tree that packs the staged block into itself (slot 1 is overwritten before frame "10" is read from it)
    "moved_back": (dict(empty=(1,)), {}),
    # entry 1 is empty and NOT viewed: it gets no slot at all, every later frame moves up by one
    "no_slot": (dict(empty=(1,)), dict(downsample_ratio=20)),
    # the occurrence filter needs no viewed counts: pipeline.project_stream / the CLI pass with_viewed=False, and
    # io.load_scene stages the mask frames alone -- the empty one among them
    "occurrence": (dict(empty=(1,)), dict(if_occurance_threshold=True)),
    "first_middle_last": (dict(empty=(0, 7, 23)), {}),
    "first_middle_last_no_slot": (dict(empty=(0, 7, 23)), dict(downsample_ratio=20)),
    # a frame id twice in mask_2d: one slot, two kernel frames; the orders agree (no repacking)
    "frame_twice": (dict(repeat=(3, 10)), {}),
    "frame_twice_and_empty": (dict(empty=(2,), repeat=(3, 10)), {}),
    "nothing_empty": ({}, {}),
}
DS_TENSORS = ("xyz", "unsort", "perm", "tile_bounds", "inv_pose", "depth_index", "frame_mask", "frame_rowbase", "frame_nmask",
              "frame_flags", "view_mask_offs", "conf", "label_id", "mask_run_offs", "run_start", "run_end")
DS_VALUES = ("n_points", "n_frames", "n_mask_frames", "n_viewed", "word_bits", "n_rows", "labels", "depth_size", "height", "width")


def same_device_scene(got, exp):
    """Every table of two DeviceScenes and the depth in whichever form it is resident."""
    for k in DS_VALUES:
        assert getattr(got, k) == getattr(exp, k), k
    for k in DS_TENSORS + ("depth", "depth_raw"):
        a, b = getattr(got, k), getattr(exp, k)
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), k
    assert (got.depth is None) != (got.depth_raw is None)


def staged_case(tmp_path, case, n_scenes=2):
    """Scenes of 24 views on disk (half-resolution 16-bit depth), their configuration, and per scene the host-side
    restatement the oracle reads (float32 metres resized with io.resize_bilinear_f32, P:431-436)."""
    from beyond_fixed_forms_amd.io import resize_bilinear_f32
    from beyond_fixed_forms_amd.synthetic import make_scene
    edits, over = STAGED_CASES[case]
    scenes = []
    for k in range(n_scenes):
        sc = make_scene("tiny", seed=90 + k, n_views=24)
        sc.scene_id = f"scene{90 + k:04d}_00"
        assert len(sc.mask_2d) == 24
        sc.mask_2d = edit_masks(sc.mask_2d, **edits)
        mm = sensor_frames(sc)
        write_scene(tmp_path, sc, {CLS: sc.mask_2d}, mm)
        host = copy.copy(sc)
        host.depths = {f: resize_bilinear_f32(m.astype(np.float32) / np.float32(1000), sc.width, sc.height) for f, m in mm.items()}
        scenes.append(host)
    return scenes, disk_cfg(tmp_path, scenes[0], **over)


def staged_loader(cfg, cls, scene_id, seen):
    """The CLI's loader, functools.partial(io.load_scene, ..., depth_on_device=True), behind a wrapper that records
    whether the frames really were decoded into the loader thread's staging."""
    from beyond_fixed_forms_amd import io as bio
    inner = functools.partial(bio.load_scene, cfg, cls, scene_id, depth_on_device=True)

    def loader(staging=None):
        sc = inner(staging=staging)
        assert sc.depth_staged is not None and sc.depth_staged[0] is staging, "the depth frames were not staged"
        held = staging.buf["depth"]
        lo = held.data_ptr()
        assert all(lo <= f.ctypes.data < lo + held.numel() for f in sc.depths_raw.values())
        seen.append((scene_id, list(sc.depth_staged[1])))
        return sc
    return loader


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case", list(STAGED_CASES))
def test_staged_depth_in_another_order_than_the_upload(lib, tmp_path, case, threads):
    """io.load_scene decodes the PNGs into the loader's pinned "depth" buffer in its own order; the upload wants the
    order of prepare_scene_fast's slots.  Where they differ the frames are packed into a SECOND pinned buffer (never
    into the one they live in), where they agree the block is uploaded in place.  Scene 1, scene 2 and scene 1 again
    go through ONE loader thread, whose buffers are reused: no scene may see another's frames.  Each resulting
    DeviceScene equals scene.prepare_scene of the same files loaded without staging, table by table and texel by texel,
    and its projection equals the oracle's."""
    from beyond_fixed_forms_amd import ingest, io as bio
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene, viewed_frame_ids, with_viewed_counts
    scenes, cfg = staged_case(tmp_path, case)
    with_viewed = with_viewed_counts(cfg)                          # what pipeline.project_stream passes in this mode
    assert with_viewed == (case != "occurrence")
    seen = []
    ing = ingest.Ingestor(cfg, DEV, n_loaders=1, native_threads=threads, with_viewed=with_viewed, with_stage1=False)
    try:
        futs = [ing.submit(staged_loader(cfg, CLS, sc.scene_id, seen)) for sc in (scenes[0], scenes[1], scenes[0])]
        got = [f.result() for f in futs]
    finally:
        ing.close()
    assert [s for s, _ in seen] == [scenes[0].scene_id, scenes[1].scene_id, scenes[0].scene_id]
    st = torch.cuda.Stream(device=DEV)
    for (ds, st1, ev), host, (_, staged_order) in zip(got, (scenes[0], scenes[1], scenes[0]), seen):
        plain = bio.load_scene(cfg, CLS, host.scene_id, depth_on_device=True)
        assert plain.depth_staged is None
        exp_ds = prepare_scene(plain, cfg, device=DEV, with_viewed=with_viewed)
        st.wait_event(ev)
        with torch.cuda.stream(st):
            same_device_scene(ds, exp_ds)
            res = run_projection(ds, cfg)
        st.synchronize()
        # the condition of the case: the staged order and the slots' order differ exactly where the case says so
        slots = [fr["frame_id"][:-4] for fr in host.mask_2d if len(fr["segmented_frame_masks"])]
        slots = list(dict.fromkeys(slots + (viewed_frame_ids(host.color_files, cfg.downsample_ratio) if with_viewed else [])))
        assert ds.depth_raw.shape[0] == len(slots)
        assert (staged_order != slots) == (case not in ("frame_twice", "nothing_empty")), (staged_order, slots)
        if case == "moved_back":
            assert len(slots) == len(staged_order) and slots.index("10") > 1
        if case in ("no_slot", "occurrence"):
            assert "10" not in slots and len(slots) == len(staged_order) - 1
        same(res.to_dict(), oracle(host, cfg))


def test_staged_depth_through_the_resize_pass(lib, tmp_path, monkeypatch):
    """The moved-back case with the depth taken through the separate scale + resize pass (float32 (H, W) images,
    BFF_DEPTH_RESIZE_PASS=1) instead of kept at the sensor's resolution: `depth` equals prepare_scene's and the host
    restatement of the resize, frame for frame in slot order."""
    from beyond_fixed_forms_amd import ingest, io as bio
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene, viewed_frame_ids
    monkeypatch.setenv("BFF_DEPTH_RESIZE_PASS", "1")
    scenes, cfg = staged_case(tmp_path, "moved_back", n_scenes=1)
    host, seen = scenes[0], []
    ing = ingest.Ingestor(cfg, DEV, n_loaders=1, native_threads=1, with_stage1=False)
    try:
        ds, _st1, ev = ing.submit(staged_loader(cfg, CLS, host.scene_id, seen)).result()
    finally:
        ing.close()
    ev.synchronize()
    exp_ds = prepare_scene(bio.load_scene(cfg, CLS, host.scene_id, depth_on_device=True), cfg, device=DEV)
    same_device_scene(ds, exp_ds)
    assert ds.depth_raw is None and ds.depth.dtype == torch.float32
    slots = [fr["frame_id"][:-4] for fr in host.mask_2d if len(fr["segmented_frame_masks"])]
    slots = list(dict.fromkeys(slots + viewed_frame_ids(host.color_files, cfg.downsample_ratio)))
    assert slots != seen[0][1]
    assert np.array_equal(ds.depth.cpu().numpy(), np.stack([host.depths[f].reshape(-1) for f in slots]))
    same(run_projection(ds, cfg).to_dict(), oracle(host, cfg))


def test_staged_depth_of_several_classes(lib, tmp_path):
    """The multi-class twin: io.load_scene_classes through Ingestor.submit_classes, one class whose list has a frame
    without masks and one whose list is a strict subset of the frames.  scene.frame_union gives the staged order AND
    the geometry's slots, so the block is uploaded in place; pinned here.  Geometry and every class equal
    prepare_geometry / prepare_class of the files loaded without staging, every class's result equals the oracle's."""
    from beyond_fixed_forms_amd import ingest, io as bio
    from beyond_fixed_forms_amd.io import resize_bilinear_f32
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import frame_union, prepare_class, prepare_geometry, viewed_frame_ids
    from beyond_fixed_forms_amd.synthetic import class_scene, make_scene
    sc = make_scene("tiny", seed=93, n_views=24)
    classes = ["with an empty frame", "a subset"]
    masks = {classes[0]: edit_masks(sc.mask_2d, empty=(1, 23)),
             classes[1]: [dict(fr, labels=[classes[1]] * len(fr["labels"])) for fr in sc.mask_2d[15:4:-2]]}
    mm = sensor_frames(sc)
    write_scene(tmp_path, sc, masks, mm)
    host = copy.copy(sc)
    host.depths = {f: resize_bilinear_f32(m.astype(np.float32) / np.float32(1000), sc.width, sc.height) for f, m in mm.items()}
    cfg = disk_cfg(tmp_path, sc)
    inner = functools.partial(bio.load_scene_classes, cfg, classes, sc.scene_id, depth_on_device=True)
    seen = []

    def loader(staging=None):
        item = inner(staging=staging)
        assert item.scene.depth_staged is not None and item.scene.depth_staged[0] is staging
        seen.append(list(item.scene.depth_staged[1]))
        return item

    real_lib, packs = ingest.host_lib(), []

    class Counting:                                  # the native library with a counter on the packing entry point
        def __getattr__(self, name):
            if name == "bff_host_pack_frames":
                packs.append(1)
            return getattr(real_lib, name)

    ing = ingest.Ingestor(cfg, DEV, n_loaders=1, native_threads=4, with_stage1=False)
    ingest._host = Counting()
    try:
        outs = [ing.submit_classes(loader, classes).result() for _ in range(2)]      # the pinned buffers are used twice
    finally:
        ingest._host = real_lib
        ing.close()
    order = frame_union([masks[c] for c in classes], viewed_frame_ids(sc.color_files, cfg.downsample_ratio))
    assert seen == [order, order] and order[:3] == ["0", "10", "20"] and packs == []        # in place, both times
    plain = bio.load_scene_classes(cfg, classes, sc.scene_id, depth_on_device=True)
    exp_geom = prepare_geometry(plain.scene, cfg, [plain.masks[c] for c in classes], device=DEV)
    for geom, dss, ev in outs:
        ev.synchronize()
        assert geom.frame_ids == exp_geom.frame_ids == order
        assert np.array_equal(geom.inv_pose_host, exp_geom.inv_pose_host)
        assert geom.depth is None and exp_geom.depth is None and geom.depth_size == exp_geom.depth_size
        for k in ("xyz", "depth_raw", "unsort", "perm", "tile_bounds", "viewed"):
            assert torch.equal(getattr(geom, k), getattr(exp_geom, k)), k
        for c, ds in zip(classes, dss):
            exp_ds = prepare_class(exp_geom, plain.masks[c], cfg)
            for k in DS_TENSORS + ("depth_raw", "viewed_in"):
                assert torch.equal(getattr(ds, k), getattr(exp_ds, k)), (c, k)
            for k in DS_VALUES:
                assert getattr(ds, k) == getattr(exp_ds, k), (c, k)
            same(run_projection(ds, cfg).to_dict(), oracle(class_scene(host, masks[c]), cfg))


def test_a_type_error_inside_a_loader_surfaces(lib):
    """Whether a loader is handed `staging` is read from its signature.  A TypeError raised INSIDE a loader that takes
    the keyword reaches future.result() after exactly one call (it is not mistaken for "takes no such keyword" and the
    scene silently loaded a second time); loaders without the keyword still work, also as functools.partial."""
    from beyond_fixed_forms_amd import ingest
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import run_projection
    from beyond_fixed_forms_amd.scene import SceneClasses
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=94)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
    calls = []

    def broken(staging=None):
        calls.append(staging)
        return len(None)                                 # TypeError: object of type 'NoneType' has no len()

    def without_keyword():
        calls.append("plain")
        return scene

    def with_argument(sc):
        calls.append("partial")
        return sc

    def classes_without_keyword():
        calls.append("classes")
        return SceneClasses(scene, {CLS: scene.mask_2d})

    ing = ingest.Ingestor(cfg, DEV, n_loaders=1, with_stage1=False)
    try:
        with pytest.raises(TypeError, match="has no len"):
            ing.submit(broken).result()
        assert len(calls) == 1 and isinstance(calls[0], ingest.Staging)
        del calls[:]
        with pytest.raises(TypeError, match="has no len"):
            ing.submit_classes(broken, [CLS]).result()
        assert len(calls) == 1 and isinstance(calls[0], ingest.Staging)
        del calls[:]
        exp = oracle(scene, cfg)
        for loader in (without_keyword, functools.partial(with_argument, scene)):
            ds, _st1, ev = ing.submit(loader).result()
            ev.synchronize()
            same(run_projection(ds, cfg).to_dict(), exp)
        _geom, dss, ev = ing.submit_classes(classes_without_keyword, [CLS]).result()
        ev.synchronize()
        same(run_projection(dss[0], cfg).to_dict(), exp)
        assert calls == ["plain", "partial", "classes"]
    finally:
        ing.close()


def test_hand_written_scene_through_the_native_path(lib):
    """The twin of test_multiclass_host.test_hand_written_scene_against_hand_written_tables: the same five-point scene
    and the same hand-written tables (tests/hand_scene_case.py) through prepare_scene_fast and through
    prepare_geometry_fast + prepare_class_fast; the viewed counts of the shared geometry are int32, one per point."""
    import hand_scene_case as case
    from beyond_fixed_forms_amd import ingest
    cfg = case.config()
    m32, m64 = case.masks()
    staging = ingest.Staging()
    for mask_2d, with_viewed, row in ((m32, True, "scene m32"), (m32, False, "scene m32 without viewed"), (m64, True, "scene m64")):
        ds = ingest.prepare_scene_fast(case.scene(mask_2d), cfg, DEV, with_viewed=with_viewed, staging=staging)
        torch.cuda.synchronize()
        assert ds.xyz.is_cuda
        case.check_tables(ds, row, None)
    geom = ingest.prepare_geometry_fast(case.scene([]), cfg, [m32, m64], DEV, staging=staging)
    assert geom.viewed.dtype == torch.int32 and tuple(geom.viewed.shape) == (5,)
    class_staging = ingest.Staging()
    for mask_2d, row in ((m32, "class m32"), (m64, "class m64")):
        ds = ingest.prepare_class_fast(geom, mask_2d, cfg, staging=class_staging)
        torch.cuda.synchronize()
        case.check_tables(ds, row, geom)


# ------------------------------------------------------------------ B. the ingestion kernels against NumPy
def morton_codes_np(xyz):
    """30-bit Morton codes, 10 bits per axis over the bounding box, non-finite coordinates counted as 0: the arithmetic
    scene.morton_order documents, restated here so that the codes themselves can be compared."""
    p = np.where(np.isfinite(xyz), xyz, 0.0).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    q = np.minimum(((p - lo) / np.maximum(hi - lo, 1e-300) * 1023.0).astype(np.uint64), 1023)
    code = np.zeros(len(p), dtype=np.uint64)
    for bit in range(10):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
    return code.astype(np.uint32), q


def cloud_layout(lib, pts, n_pad, sort, exact_temp=True):
    """bff_cloud_layout as ingest._cloud_to_device calls it, with every output pre-filled: -> host arrays."""
    n, stride = pts.shape
    pts_dev = torch.from_numpy(pts).to(DEV)
    xyz = torch.full((3, n_pad), 7.25, dtype=torch.float64, device=DEV)
    unsort = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    perm = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    codes = torch.full((2 * n,), -1, dtype=torch.int32, device=DEV)
    box = torch.zeros(6, dtype=torch.float64, device=DEV)
    need = ctypes.c_size_t(0)
    lib.call("bff_cloud_layout", None, n, stride, n_pad, 1, None, None, None, None, None, None, ctypes.byref(need))
    assert need.value > 0
    temp = torch.empty(int(need.value) + (0 if exact_temp else 4096), dtype=torch.uint8, device=DEV)     # exactly what the query said
    nbytes = ctypes.c_size_t(temp.numel())
    lib.call("bff_cloud_layout", lib._ptr(pts_dev), n, stride, n_pad, sort, lib._ptr(xyz), lib._ptr(unsort), lib._ptr(perm),
             lib._ptr(codes), lib._ptr(box), lib._ptr(temp), ctypes.byref(nbytes))
    torch.cuda.synchronize()
    return xyz, unsort.cpu().numpy(), perm.cpu().numpy(), codes.cpu().numpy().view(np.uint32), box.cpu().numpy()


def tile_bounds_np(xyz, n, tile):
    """min / max per tile of `tile` consecutive points; NaN coordinates are ignored (fmin / fmax), as the kernel documents."""
    out = np.empty(((n + tile - 1) // tile, 6))
    for t in range(out.shape[0]):
        part = xyz[:, t * tile:min(n, (t + 1) * tile)]
        out[t, :3] = np.fmin.reduce(part, axis=1, initial=np.inf)
        out[t, 3:] = np.fmax.reduce(part, axis=1, initial=-np.inf)
    return out


def nan_with_payload(k):
    return np.array([0x7FF8000000000000 | (int(k) + 1)], dtype=np.uint64).view(np.float64)[0]


def make_cloud(kind, n, stride, seed):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, stride)) * np.array([6.0, 4.0, 3.0] + [255.0] * (stride - 3))
    if kind == "flat_axis":                                      # one axis of zero extent
        pts[:, 1] = 2.5
    elif kind == "identical":
        pts[:, :] = pts[0]
    elif kind == "nonfinite":                                    # NaN (with payloads), +inf, -inf, -0.0 in some coordinates
        for k in range(0, n, 5):
            pts[k, k % 3] = (nan_with_payload(k), np.inf, -np.inf, -0.0)[(k // 5) % 4]
        if n > 7:
            pts[7, :3] = np.nan
    elif kind == "on_the_box":                                   # coordinates exactly on lo and hi of the box
        pts[0, :3] = 0.0
        pts[n - 1, :3] = (6.0, 4.0, 3.0)
        if n > 4:
            pts[1, :3] = (6.0, 0.0, 3.0)
            pts[n // 2, :3] = (0.0, 4.0, 0.0)
    elif kind == "far_and_thin":                                 # values of about 1e6 over an extent of about 1e-3
        pts[:, :3] = 1.0e6 + rng.random((n, 3)) * 1.0e-3
    elif kind == "coarse":                                       # few distinct cells: many equal codes, ties everywhere
        pts[:, :3] = rng.integers(0, 3, (n, 3)).astype(np.float64)
    else:
        assert kind == "room"
    return np.ascontiguousarray(pts)


CLOUD_SIZES = [1, 2, 63, 1023, 1024, 1025, 200_003]
CLOUD_CASES = [("room", n, 3) for n in CLOUD_SIZES] + [("room", n, 6) for n in CLOUD_SIZES] + \
    [("room", n, 7) for n in (1, 63, 1025)] + \
    [(kind, n, stride) for kind in ("flat_axis", "identical", "nonfinite", "on_the_box", "far_and_thin", "coarse")
     for n, stride in ((2, 3), (1025, 6), (200_003, 6) if kind in ("nonfinite", "coarse") else (63, 7))]


@pytest.mark.parametrize("kind,n,stride", CLOUD_CASES, ids=[f"{k}-n{n}-stride{s}" for k, n, s in CLOUD_CASES])
def test_cloud_layout_against_numpy(lib, kind, n, stride):
    """bff_cloud_layout (bounding box, Morton codes, stable radix sort, gather into [3][n_pad]) and
    bff_point_tile_bounds on its result against scene.morton_order + a plain gather + NumPy min / max per tile."""
    from beyond_fixed_forms_amd.scene import morton_order
    pts = make_cloud(kind, n, stride, seed=1000 * stride + n % 997)
    n_pad = max(1024, (n + 1023) // 1024 * 1024)                 # the granule ingest.prepare_scene_fast pads to
    codes_np, q = morton_codes_np(pts[:, :3])
    perm_np = morton_order(pts[:, :3])
    assert np.array_equal(perm_np, np.argsort(codes_np, kind="stable"))            # the restatement is the product's order
    if kind == "on_the_box":
        assert codes_np[0] == 0 and codes_np[n - 1] == 0x3FFFFFFF and q.max() == 1023
    if kind == "coarse" and n > 100:
        assert len(np.unique(codes_np)) <= 27
    xyz, unsort, perm, codes, _box = cloud_layout(lib, pts, n_pad, 1)
    # perm is THE stable order: a permutation, ties in the caller's order, codes along it non-decreasing
    assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(perm, perm_np)
    assert np.array_equal(unsort[perm], np.arange(n))
    assert np.array_equal(codes[:n], codes_np)
    assert np.array_equal(codes[n:], codes_np[perm]) and np.all(np.diff(codes[n:].astype(np.int64)) >= 0)
    tie = codes[n:][1:] == codes[n:][:-1]
    assert np.all(perm[1:][tie] > perm[:-1][tie])
    # the cloud: copied through bit for bit (NaN payloads, infinities and -0.0 included), zero behind the last point
    got = xyz.cpu().numpy()
    assert np.array_equal(got[:, :n].view(np.uint64), np.ascontiguousarray(pts[perm, :3].T).view(np.uint64))
    assert np.array_equal(got[:, n:].view(np.uint64), np.zeros((3, n_pad - n), np.uint64))
    tile = lib.load().bff_point_tile_size()
    assert tile == 256
    bounds = lib.point_tile_bounds(xyz, n).cpu().numpy()
    assert np.array_equal(bounds.view(np.uint64), tile_bounds_np(got, n, tile).view(np.uint64))
    # sort = 0: the caller's order, `unsort` and `perm` untouched; a pad that is not the granule
    n_pad0 = n + 5
    xyz0, unsort0, perm0, _codes0, _ = cloud_layout(lib, pts, n_pad0, 0, exact_temp=False)
    got0 = xyz0.cpu().numpy()
    assert np.all(unsort0 == -7) and np.all(perm0 == -7)
    assert np.array_equal(got0[:, :n].view(np.uint64), np.ascontiguousarray(pts[:, :3].T).view(np.uint64))
    assert np.array_equal(got0[:, n:].view(np.uint64), np.zeros((3, 5), np.uint64))
    assert np.array_equal(lib.point_tile_bounds(xyz0, n).cpu().numpy().view(np.uint64), tile_bounds_np(got0, n, tile).view(np.uint64))


def test_cloud_layout_rejects_too_little_scratch_on_the_host(lib):
    """One byte less than the size query asked for is refused by the argument check (nothing is launched)."""
    n = 1000
    pts = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    xyz = torch.zeros((3, 1024), dtype=torch.float64, device=DEV)
    ints = [torch.zeros(2 * n, dtype=torch.int32, device=DEV) for _ in range(3)]
    box = torch.zeros(6, dtype=torch.float64, device=DEV)
    need = ctypes.c_size_t(0)
    lib.call("bff_cloud_layout", None, n, 3, 1024, 1, None, None, None, None, None, None, ctypes.byref(need))
    temp = torch.empty(int(need.value), dtype=torch.uint8, device=DEV)
    short = ctypes.c_size_t(int(need.value) - 1)
    with pytest.raises(RuntimeError, match="scratch missing"):
        lib.call("bff_cloud_layout", lib._ptr(pts), n, 3, 1024, 1, lib._ptr(xyz), lib._ptr(ints[0]), lib._ptr(ints[1]),
                 lib._ptr(ints[2]), lib._ptr(box), lib._ptr(temp), ctypes.byref(short))
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("bff_cloud_layout", lib._ptr(pts), n, 2, 1024, 1, lib._ptr(xyz), lib._ptr(ints[0]), lib._ptr(ints[1]),
                 lib._ptr(ints[2]), lib._ptr(box), lib._ptr(temp), ctypes.byref(need))
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("bff_cloud_layout", lib._ptr(pts), n, 3, n - 1, 1, lib._ptr(xyz), lib._ptr(ints[0]), lib._ptr(ints[1]),
                 lib._ptr(ints[2]), lib._ptr(box), lib._ptr(temp), ctypes.byref(need))


DEPTH_VALUES = np.array([0, 1, 32767, 32768, 40000, 65535], dtype=np.uint16)


def depth_frames(n_frames, hs, ws, seed):
    """uint16 frames over the whole range of the format; the values that break a signed or a narrowed read sit in the
    last row, the last column and the corner texel (the partial tiles) as well as in the middle."""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 65536, (n_frames, hs, ws)).astype(np.uint16)
    pick = rng.random(fr.shape) < 0.3
    fr[pick] = DEPTH_VALUES[rng.integers(0, len(DEPTH_VALUES), int(pick.sum()))]
    for f in range(n_frames):
        fr[f, hs - 1, :] = DEPTH_VALUES[(np.arange(ws) + f) % 6]
        fr[f, :, ws - 1] = DEPTH_VALUES[(np.arange(hs) + 2 * f + 1) % 6]
        fr[f, 0, 0] = (32768, 65535, 0, 40000, 1)[f % 5]
        fr[f, hs - 1, ws - 1] = (65535, 32768, 40000, 32767, 1)[f % 5]
    return fr


def tiles_np(frames):
    """[F][hs][ws] -> [F][ceil(hs/8)][ceil(ws/8)][8][8] flattened, zero-padded."""
    f, hs, ws = frames.shape
    th, tw = (hs + 7) // 8, (ws + 7) // 8
    pad = np.zeros((f, th * 8, tw * 8), dtype=frames.dtype)
    pad[:, :hs, :ws] = frames
    return np.ascontiguousarray(pad.reshape(f, th, 8, tw, 8).transpose(0, 1, 3, 2, 4)).reshape(f, th * tw * 64)


DEPTH_SIZES = [(1, 1), (1, 2), (7, 9), (8, 8), (9, 17), (240, 320), (480, 640), (41, 67)]


@pytest.mark.parametrize("n_frames", [0, 1, 5])
@pytest.mark.parametrize("hs,ws", DEPTH_SIZES)
def test_depth_tiles_against_numpy(lib, hs, ws, n_frames):
    """bff_depth_tile_u16, both outputs: the uint16 values as stored and float32 `np.float32(v) / np.float32(1000)`, in
    8 x 8 tiles with zero padding, against a NumPy re-tiling; written into pre-filled outputs, so padding texels that
    are left unwritten show."""
    fr = depth_frames(n_frames, hs, ws, seed=hs * 1000 + ws)
    if n_frames:
        assert fr.max() == 65535 and (fr >= 32768).sum() > 0 and fr[:, hs - 1, ws - 1].max() >= 32768
    texels = int(lib.load().bff_depth_tiled_texels(hs, ws))
    assert texels == ((hs + 7) // 8) * ((ws + 7) // 8) * 64
    exp = tiles_np(fr)
    raw = torch.from_numpy(fr.view(np.int16)).to(DEV)
    out16 = torch.full((n_frames, texels), 0x5A5A, dtype=torch.int16, device=DEV)
    out32 = torch.full((n_frames, texels), 7.25, dtype=torch.float32, device=DEV)
    lib.call("bff_depth_tile_u16", lib._ptr(raw, torch.int16), n_frames, hs, ws, lib._ptr(out16), 0)
    lib.call("bff_depth_tile_u16", lib._ptr(raw, torch.int16), n_frames, hs, ws, lib._ptr(out32), 1)
    assert np.array_equal(out16.cpu().numpy().view(np.uint16), exp)
    assert np.array_equal(out32.cpu().numpy().view(np.uint32), (exp.astype(np.float32) / np.float32(1000)).view(np.uint32))
    # the wrapper the scene path calls
    assert np.array_equal(lib.tile_depth(raw, metres=False).cpu().numpy().view(np.uint16), exp)
    assert np.array_equal(lib.tile_depth(raw, metres=True).cpu().numpy().view(np.uint32),
                          (exp.astype(np.float32) / np.float32(1000)).view(np.uint32))


@pytest.mark.parametrize("hs,ws,h,w", [(480, 640, 968, 1296), (48, 64, 97, 131), (120, 160, 120, 160), (100, 90, 37, 41)])
def test_depth_resize_pass_over_the_whole_uint16_range(lib, hs, ws, h, w):
    """bff_depth_from_u16 on frames that use all 16 bits == io.resize_bilinear_f32(frame.astype(float32) / 1000)."""
    from beyond_fixed_forms_amd import io as bio
    fr = depth_frames(3, hs, ws, seed=hs * w)
    assert (fr >= 32768).mean() > 0.3
    exp = np.stack([bio.resize_bilinear_f32(r.astype(np.float32) / np.float32(1000), w, h) for r in fr])
    assert exp.max() > 65.0
    taps = None if (hs, ws) == (h, w) else tuple(torch.from_numpy(a).to(DEV) for a in bio.bilinear_taps(hs, ws, h, w))
    got = lib.depth_from_u16(torch.from_numpy(fr.view(np.int16)).to(DEV), h, w, taps).cpu().numpy().reshape(3, h, w)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def scaled_scene(seed, scale):
    """A tiny scene blown up by `scale`: points, pose translations and depth times `scale`, intrinsics unchanged -- the
    same pixels, stored depth beyond 32767 mm.  -> (scene with depths_raw at half resolution, the oracle's host scene,
    the host scene with every stored value >= 32768 zeroed)."""
    from beyond_fixed_forms_amd.io import resize_bilinear_f32
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=seed)
    h, w = scene.height, scene.width
    raw = copy.copy(scene)
    raw.points = scene.points.copy()
    raw.points[:, :3] *= scale
    raw.poses = {}
    for f, p in scene.poses.items():
        q = np.array(p, dtype=np.float64)
        q[:3, 3] *= scale
        raw.poses[f] = q
    raw.depths_raw = {}
    for f, d in scene.depths.items():
        mm = np.round(d[::2, ::2].astype(np.float64) * 1000).astype(np.int64) * scale
        assert mm.max() < 65535
        raw.depths_raw[f] = np.ascontiguousarray(mm.astype(np.uint16))
    raw.depths = {}
    host, low = copy.copy(raw), copy.copy(raw)
    host.depths = {f: resize_bilinear_f32(m.astype(np.float32) / np.float32(1000), w, h) for f, m in raw.depths_raw.items()}
    low.depths = {f: resize_bilinear_f32(np.where(m >= 32768, 0, m).astype(np.float32) / np.float32(1000), w, h)
                  for f, m in raw.depths_raw.items()}
    return raw, host, low


@pytest.mark.parametrize("seed,scale", [(84, 13), (80, 10), (81, 10)])
def test_depth_beyond_32767_mm_through_the_sweep(lib, seed, scale):
    """Stored depth of 32768 mm and more (the frames travel as int16 tensors) through the sweep in all four depth forms
    -- float32 tiles, uint16 tiles, uint16 rows, and the separate resize pass -- step by step and through the one-call
    path: raw rows, both counters and the final masks equal the oracle's, which reads the host restatement of the
    resize.  Condition on the input, taken from the oracle alone: visible (point, frame) pairs behind such values exist
    in number -- its viewed total drops by far more than a handful when they are zeroed -- so a sign-extended read of
    any of the forms cannot go unnoticed."""
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.ingest import prepare_scene_fast
    from beyond_fixed_forms_amd.projection import projection_back, projection_front, run_projection
    from beyond_fixed_forms_amd.scene import prepare_scene
    raw, host, low = scaled_scene(seed, scale)
    cfg = Config.with_defaults(width_2d=raw.width, height_2d=raw.height)
    exp, dbg = oracle(host, cfg, debug=True)
    _exp_low, dbg_low = oracle(low, cfg, debug=True)
    viewed, viewed_low = int(dbg["viewed_counts"].sum()), int(dbg_low["viewed_counts"].sum())
    masked, masked_low = int(dbg["masked_counts_raw"].sum()), int(dbg_low["masked_counts_raw"].sum())
    assert max(int(m.max()) for m in raw.depths_raw.values()) >= 40000
    # "more than a handful": a hundred viewed pairs and a score of mask votes hang on the high values
    assert viewed - viewed_low >= 100 and masked - masked_low >= 20, (viewed, viewed_low, masked, masked_low)
    assert len(exp["conf"]) >= 1
    n = raw.points.shape[0]
    old = os.environ.get("BFF_DEPTH_TILES")
    try:
        for form in ("f32", "u16", "0", "resize_pass"):
            if form != "resize_pass":
                os.environ["BFF_DEPTH_TILES"] = form
            else:
                os.environ.pop("BFF_DEPTH_TILES", None)
            ds = prepare_scene(raw, cfg, device=DEV, raw_depth_resident=form != "resize_pass")
            if form == "resize_pass":
                assert ds.depth_raw is None and ds.depth.dtype == torch.float32
            else:
                assert ds.depth is None and ds.depth_raw.dtype == (torch.float32 if form == "f32" else torch.int16)
                assert (ds.depth_size is None) == (form == "0")
            res = run_projection(ds, cfg, debug_out=True)
            bits = np.unpackbits(res.debug["raw_rows"].cpu().numpy().view(np.uint8), axis=-1, bitorder="little")[:, :n].astype(bool)
            assert np.array_equal(bits, dbg["raw_ins"].numpy()), form
            assert np.array_equal(res.debug["masked_counts_raw"].cpu().numpy(), dbg["masked_counts_raw"].numpy().astype(np.int32)), form
            assert np.array_equal(res.debug["viewed_counts"].cpu().numpy(), dbg["viewed_counts"].numpy().astype(np.int32)), form
            assert list(res.groups) == dbg["groups"], form
            same(res.to_dict(), exp)
            if form != "resize_pass":                            # the one-call path on the same form
                prod = projection_back(projection_front(prepare_scene_fast(raw, cfg, DEV), cfg))
                assert prod.debug["path"] == "fast"
                same(prod.to_dict(), exp)
        os.environ["BFF_DEPTH_RESIZE_PASS"] = "1"
        try:
            ds = prepare_scene_fast(raw, cfg, DEV)
            assert ds.depth_raw is None
            prod = projection_back(projection_front(ds, cfg))
        finally:
            del os.environ["BFF_DEPTH_RESIZE_PASS"]
        assert prod.debug["path"] == "fast"
        same(prod.to_dict(), exp)
    finally:
        os.environ.pop("BFF_DEPTH_TILES", None)
        if old is not None:
            os.environ["BFF_DEPTH_TILES"] = old
