"""Depth frames rendered from the cloud with a surfel footprint per point (bff_render_splat_depth_u16) on the GPU: the
kernel against its NumPy statement (tests/splat_depth_ref.py) byte for byte and against the plain point z-buffer, and
scenes without depth frames with the config key `cloud_splat_radius` against the oracle fed with the statement's frames.
Everything is compared for equality."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import render_depth_ref as rd
import splat_depth_ref as sd
from oracle import geom_fma, projection_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N, N_PAD, F = 1500, 2048, 9
K33 = np.array([[64.0, 0.0, 34.5], [0.0, 64.0, 24.5], [0.0, 0.0, 1.0]])
R = 0.03125                                                              # 2^-5: Rx = 2 / c_2 pixels, exact for a power of two
WHOLE = 2                                                                # the frame one crafted point covers entirely
# (height, width, stride, frames): both images at strides 1, 2, 3 (does not divide either size) and 8
CASES = [(50, 70, 1, 3), (50, 70, 2, 9), (50, 70, 3, 5), (50, 70, 8, 9), (48, 64, 1, 4), (48, 64, 2, 3), (48, 64, 3, 9),
         (48, 64, 8, 6)]


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def at_pixel(u, v, z):
    """A point (camera 0 = world coordinates) that projects to pixel (u, v) at depth z."""
    return [(u - K33[0, 2]) * z / 64.0, (v - K33[1, 2]) * z / 64.0, z]


CRAFTED = [
    at_pixel(30, 20, 1.0),                                               # 0: Rx = Ry = 2.0 exactly
    at_pixel(12, 30, 2.001),                                             # 1: Rx just below one pixel: its own sample point only
    at_pixel(0, 0, 0.5), at_pixel(69, 49, 0.5), at_pixel(63, 47, 0.5), at_pixel(35, 0, 0.5), at_pixel(0, 25, 0.5),
    at_pixel(69, 25, 0.5), at_pixel(35, 49, 0.5),                        # 2..8: Rx = 4, clipped at every border and corner
    at_pixel(50, 35, 0.25),                                              # 9: Rx = 8: 17 x 17 pixels, the wave's walk
    None,                                                                # 10: covers frame WHOLE entirely (set in cloud())
    [0.1, 0.1, -1.0], [0.0, 0.0, 0.0],                                   # 11, 12: behind / in the camera
    at_pixel(70, 10, 0.5), at_pixel(64, 12, 0.5), at_pixel(-1, 30, 0.5), at_pixel(20, -1, 0.5), at_pixel(20, 50, 0.5),
    at_pixel(22, 48, 0.5),                                               # 13..18: a pixel just outside (of one image or both)
    at_pixel(40, 5, 0.0004), at_pixel(5, 40, 65.536),                    # 19, 20: m = 0, m = 65536
    [np.nan, 0.0, 1.0], [0.0, 0.0, np.nan], [0.0, np.inf, 1.0],          # 21..23
]


@functools.lru_cache(maxsize=None)
def cloud():
    """1500 points: one full block of 1024 and a ragged one (476 = 7 words and 28 lanes), the crafted points first, then
    random points sorted along x; 9 poses, the first the identity, the last full of NaN.  Padding lanes hold a point
    that would cover much of frame 0 if it were read."""
    rng = np.random.default_rng(11)
    inv = np.zeros((F, 16))
    inv[0] = np.eye(4).reshape(-1)
    poses = [np.eye(4)]
    for f in range(1, F - 1):
        a = rng.uniform(-1.2, 1.2)
        pose = np.eye(4)
        pose[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        pose[:3, 3] = rng.uniform(-1, 1, 3)
        poses.append(pose)
        inv[f] = np.linalg.inv(pose).reshape(-1)
    inv[F - 1] = np.nan
    crafted = list(CRAFTED)
    crafted[10] = (poses[WHOLE] @ np.array(at_pixel(34, 24, 0.05) + [1.0]))[:3].tolist()       # c_2 ~ 0.05 in frame WHOLE
    crafted = np.array(crafted, np.float64)
    n_rand = N - len(crafted)
    rnd = np.stack([rng.uniform(-6, 6, n_rand), rng.uniform(-2, 2, n_rand), rng.uniform(0.8, 5, n_rand)], 1)
    xyz = np.concatenate([crafted, rnd[np.argsort(rnd[:, 0])]])
    assert xyz.shape == (N, 3)
    soa = np.empty((3, N_PAD))
    soa[:, :N] = xyz.T
    soa[:, N:] = np.array([[0.0], [0.0], [0.1]])
    return xyz, inv, soa


@functools.lru_cache(maxsize=None)
def reference(h, w, stride, nf=F, radius=R):
    """(the statement's frames, per frame the footprint rectangles' texel counts) -- computed once, never written to."""
    xyz, inv, _ = cloud()
    boxes = []
    ref = sd.render_splat_ref(xyz, inv[:nf], K33, h, w, *rd.rendered_size(h, w, stride), radius, boxes)
    ref.setflags(write=False)
    return ref, boxes


def taking_part(f, h, w):
    """Indices of the points that take part in frame f, in the order of the statement's boxes."""
    xyz, inv, _ = cloud()
    pts, pix, _ = geom_fma.view(xyz, inv[f].reshape(4, 4), K33, np.zeros((1, 1), np.float32))
    with np.errstate(all="ignore"):
        m = np.rint(pts[:, 2] * 1000.0)
        return np.flatnonzero((pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h) & (pts[:, 2] > 0) &
                              (m >= 1) & (m <= 65535))


def test_crafted_points_are_what_they_claim(lib):
    lane = lib.load().bff_splat_lane_box()
    ref, boxes = reference(50, 70, 1)
    part = taking_part(0, 50, 70)
    box = dict(zip(part.tolist(), boxes[0].tolist()))
    assert box[0] == 25 and box[1] == 1                                  # Rx exactly 2: 5 x 5; just below a pixel: 1 x 1
    assert [box[k] for k in range(2, 9)] == [25, 25, 63, 45, 45, 45, 45]  # 9 x 9 clipped; (63, 47) is a corner of the 48 x 64 image
    assert box[9] == 17 * 17 and box[9] > lane >= box[0]                 # the wave's walk and the lane's both happen
    assert all(k not in box for k in range(11, 24) if k not in (14, 18))  # behind, outside, out of range, NaN: no part
    small, _ = reference(48, 64, 1, 4)
    part48 = set(taking_part(0, 48, 64).tolist())
    assert 3 not in part48 and 4 in part48 and 14 not in part48 and 18 not in part48 and 17 not in part48
    assert 14 in box and 18 in box                                       # in bounds of the larger image only
    assert ((ref[0, 18:23, 28:33] != 0) & (ref[0, 18:23, 28:33] <= 1000)).all() and (ref[0, 18:23, 28:33] == 1000).any()
    # frame WHOLE: the point at c_2 ~ 0.05 covers every texel, in every case; the other frames hold many depths
    for h, w, stride, nf in CASES:
        r, b = reference(h, w, stride, nf)
        assert len(np.unique(r[WHOLE])) == 1 and 49 <= r[WHOLE, 0, 0] <= 51 and b[WHOLE].max() == r[WHOLE].size
        assert all(len(np.unique(r[f])) > 20 for f in range(nf) if f not in (WHOLE, F - 1)) or stride == 8
        assert (r[0] == 0).any() or stride > 1                           # fine frames keep empty texels: both outcomes occur
    assert not ref[F - 1].any()                                          # the NaN pose sees nothing
    assert not (ref[0] == 100).any()                                     # the padding's point is never read


def render(lib, h, w, stride, nf=F, bounds=False, radius=R, **kw):
    _, inv, soa = cloud()
    dh, dw = rd.rendered_size(h, w, stride)
    xyz = torch.from_numpy(soa).to(DEV)
    tb = lib.point_tile_bounds(xyz, N) if bounds else None
    out = lib.render_depth(xyz, N, torch.from_numpy(inv[:nf].copy()).to(DEV), K33, h, w, dh, dw, tile_bounds=tb,
                           splat_radius=radius, **kw)
    assert out.dtype == torch.int16 and tuple(out.shape) == (nf, dh, dw)
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("h,w,stride,nf", CASES)
def test_kernel_equals_statement(lib, h, w, stride, nf, monkeypatch):
    names = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    ref, _ = reference(h, w, stride, nf)
    got = render(lib, h, w, stride, nf)
    assert names == ["bff_render_splat_depth_u16"]
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:10]
    culled = render(lib, h, w, stride, nf, bounds=True)
    assert np.array_equal(culled, ref), np.argwhere(culled != ref)[:10]  # same frames with and without the culling table
    assert render(lib, h, w, stride, nf, bounds=True).tobytes() == culled.tobytes()      # and on every run


@pytest.mark.parametrize("tile", [2, 3, 8, 9])
@pytest.mark.parametrize("h,w,stride", [(50, 70, 2), (48, 64, 3)])
def test_frame_tiles_equal_statement(lib, h, w, stride, tile):
    """The 9 frames with a block visiting several of them: ragged tiles (2, 3), one full culling group of 8 and one
    frame over (8, 9), with and without the culling table."""
    ref, _ = reference(h, w, stride)
    for bounds in (False, True):
        got = render(lib, h, w, stride, bounds=bounds, frames_per_block=tile)
        assert np.array_equal(got, ref), (bounds, np.argwhere(got != ref)[:10])


def test_scratch_smaller_than_the_frames(lib):
    """A scratch that holds 4 of the 9 frames: three runs (4, 4, 1), the same frames; and frame by frame."""
    ref, _ = reference(50, 70, 8)
    assert np.array_equal(render(lib, 50, 70, 8, bounds=True, scratch_texels=4 * 7 * 9 + 5), ref)
    assert np.array_equal(render(lib, 50, 70, 8, scratch_texels=1, frames_per_block=8), ref)


@pytest.mark.parametrize("h,w,stride", [(50, 70, 1), (50, 70, 3), (48, 64, 2), (48, 64, 8)])
def test_monotone_against_the_plain_z_buffer(lib, h, w, stride):
    """Wherever bff_render_depth_u16's frame holds a depth the splat frame holds one that is not larger; with a radius
    below every texel pitch a point reaches at most the sample point of its own texel: equal bytes."""
    plain = render(lib, h, w, stride, radius=0.0)
    assert np.array_equal(plain, rd.render_depth_ref(cloud()[0], cloud()[1], K33, h, w, *rd.rendered_size(h, w, stride)))
    splat = render(lib, h, w, stride)
    held = plain != 0
    assert held.any() and (splat[held] != 0).all() and (splat[held] <= plain[held]).all() and (splat != plain).any()
    assert render(lib, h, w, stride, radius=1e-6).tobytes() == plain.tobytes()


def test_bad_arguments_launch_nothing(lib):
    """r of 0, negative, NaN or inf and a non-positive K00 or K11: BFF_E_ARG, and the frames are not touched."""
    _, inv, soa = cloud()
    xyz, poses = torch.from_numpy(soa).to(DEV), torch.from_numpy(inv).to(DEV)
    scratch = torch.full((F * 7 * 9,), 7, dtype=torch.int32, device=DEV)
    out = torch.full((F, 7, 9), 7, dtype=torch.int16, device=DEV)
    fn, p = lib.load().bff_render_splat_depth_u16, lambda t: ctypes.c_void_p(t.data_ptr())
    k9 = lambda k: (ctypes.c_double * 9)(*[float(v) for v in np.asarray(k).reshape(-1)])

    def rc(radius, k=K33):
        return fn(p(xyz), N, N_PAD, p(poses), ctypes.cast(k9(k), ctypes.c_void_p), F, 50, 70, 7, 9, radius, 0, p(scratch), p(out),
                  None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    for bad in (0.0, -0.0, -R, float("nan"), float("inf"), -float("inf")):
        assert rc(bad) == -1 and b"splat_radius" in lib.load().bff_last_error()
    for i, v in ((0, 0.0), (0, -64.0), (4, 0.0), (4, float("nan")), (0, float("inf"))):
        k = K33.copy()
        k.reshape(-1)[i] = v
        assert rc(R, k) == -1 and b"K00" in lib.load().bff_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((scratch == 7).all())
    assert rc(R) == 0                                                    # the same call with good arguments renders
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), reference(50, 70, 8)[0])
    for bad in (float("nan"), -R, float("inf")):                         # through the wrapper: the library's error
        with pytest.raises(RuntimeError, match="splat_radius"):
            render(lib, 50, 70, 8, radius=bad)


def test_empty_inputs_return_cleanly(lib):
    _, inv, soa = cloud()
    xyz = torch.from_numpy(soa).to(DEV)
    none = lib.render_depth(xyz, N, torch.zeros((0, 16), dtype=torch.float64, device=DEV), K33, 50, 70, 7, 9, splat_radius=R)
    assert tuple(none.shape) == (0, 7, 9)
    with pytest.raises(RuntimeError, match="splat_radius"):              # checked before the early return, as the sizes are
        lib.render_depth(xyz, N, torch.zeros((0, 16), dtype=torch.float64, device=DEV), K33, 50, 70, 7, 9, splat_radius=-1.0)
    out = lib.render_depth(xyz, 0, torch.from_numpy(inv).to(DEV), K33, 50, 70, 7, 9, splat_radius=R)   # no points
    torch.cuda.synchronize()
    assert tuple(out.shape) == (F, 7, 9) and int(out.count_nonzero()) == 0


# ------------------------------------------------------------------ scenes without depth frames against the oracle
SEED, STRIDE, RADIUS = 74, 4, 0.03


def cfg_for(scene, **over):
    from beyond_fixed_forms_amd.config import Config
    return Config.with_defaults(width_2d=scene.width, height_2d=scene.height, **over)


def same(got, exp):
    assert got["ins"].dtype == exp["ins"].dtype and tuple(got["ins"].shape) == tuple(exp["ins"].shape)
    assert torch.equal(got["ins"].cpu(), exp["ins"].cpu())
    assert got["conf"].dtype == exp["conf"].dtype and torch.equal(got["conf"].cpu(), exp["conf"].cpu())
    assert list(got["final_class"]) == list(exp["final_class"])


def test_occlusion_by_hand(lib):
    """render_depth_ref.two_plane_scene at stride 1 with r = 0.015625 (Rx = 1 on the near plane, test_splat_depth_host):
    the near plane's silhouette grows by one pixel on every side, so the far points of the rectangle v 15..32, u 19..44
    are hidden and every other point is seen -- the hand statement is certain for every point."""
    from beyond_fixed_forms_amd.projection import project_scene
    scene, far_px, n_far = rd.two_plane_scene()
    over = dict(min_aggragated_masks=1, if_detected_ratio_threshold=False)
    got = project_scene(scene, cfg_for(scene, depth_from_cloud=1, cloud_splat_radius=0.015625, **over), DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pref.project_scene_ref(sd.scene_with_rendered_depth(scene, 1, 0.015625), cfg_for(scene, **over))
    same(got, exp)
    assert got["ins"].shape[0] == 1
    u, v = far_px[:, 0], far_px[:, 1]
    hidden = (v >= 15) & (v < 33) & (u >= 19) & (u < 45)
    row = got["ins"][0].cpu().numpy().astype(bool)
    assert hidden.sum() == 18 * 26 and np.array_equal(row, np.concatenate([~hidden, np.ones(len(row) - n_far, bool)]))
    plain = project_scene(scene, cfg_for(scene, depth_from_cloud=1, **over), DEV)["ins"][0].cpu().numpy().astype(bool)
    assert int(plain.sum()) - int(row.sum()) == 84                       # the key is what hides the ring


@functools.lru_cache(maxsize=None)
def generated():
    """(the generated scene without depth, the same scene with the depth images the reference would read from the
    statement's frames)."""
    from beyond_fixed_forms_amd.synthetic import make_scene
    scene = make_scene("tiny", seed=SEED)
    return rd.without_depth(scene), sd.scene_with_rendered_depth(scene, STRIDE, RADIUS)


def test_generated_scene_equals_oracle(lib, monkeypatch):
    """project_scene (the one-call path behind prepare_scene_fast, and debug_out=True behind prepare_scene),
    prepare_scene_fast itself with the frames resident row-major, and project_scene_classes with two classes, which
    renders once: all equal the oracle fed with the statement's frames."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.ingest import prepare_scene_fast
    from beyond_fixed_forms_amd.projection import project_scene, project_scene_classes, run_projection
    from beyond_fixed_forms_amd.synthetic import class_scene
    scene, ref_scene = generated()
    assert scene.depths == {} and scene.depths_raw is None
    cfg = cfg_for(scene, depth_from_cloud=STRIDE, cloud_splat_radius=RADIUS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pref.project_scene_ref(ref_scene, cfg_for(ref_scene))
        plain = pref.project_scene_ref(rd.scene_with_rendered_depth(scene, STRIDE), cfg_for(ref_scene))
    assert exp["ins"].dim() == 2 and exp["ins"].shape[0] >= 1 and len(exp["final_class"]) >= 1     # the oracle keeps an instance
    print("splat and plain frames give", "the same" if exp["ins"].shape == plain["ins"].shape and
          torch.equal(exp["ins"], plain["ins"]) else "different", "instances")
    calls = []
    real = _lib.render_depth
    monkeypatch.setattr(_lib, "render_depth", lambda *a, **k: (calls.append(k.get("splat_radius")), real(*a, **k))[1])
    same(project_scene(scene, cfg, DEV), exp)
    same(project_scene(scene, cfg, DEV, debug_out=True), exp)
    assert calls == [RADIUS] * 2
    # prepare_scene_fast: the resident frames are the statement's, texel for texel
    monkeypatch.setenv("BFF_DEPTH_TILES", "0")
    ds = prepare_scene_fast(scene, cfg, device=DEV)
    assert calls == [RADIUS] * 3 and ds.depth is None and ds.depth_raw is not None
    dh, dw = rd.rendered_size(scene.height, scene.width, STRIDE)
    ids = list(dict.fromkeys([fr["frame_id"][:-4] for fr in scene.mask_2d if len(fr["labels"])] +
                             pref.viewed_frame_ids(scene.color_files, cfg.downsample_ratio)))
    inv = np.stack([np.linalg.inv(scene.poses[f]) for f in ids])
    frames = sd.render_splat_ref(scene.points, inv, scene.cam_intr[:3, :3], scene.height, scene.width, dh, dw, RADIUS)
    assert np.array_equal(ds.depth_raw.cpu().numpy().view(np.uint16), frames)
    assert not np.array_equal(frames, rd.render_depth_ref(scene.points, inv, scene.cam_intr[:3, :3], scene.height, scene.width,
                                                          dh, dw))               # the key is what changes the frames
    same(run_projection(ds, cfg).to_dict(), exp)
    monkeypatch.delenv("BFF_DEPTH_TILES")
    # two classes: one render per scene
    del calls[:]
    masks = {"table": scene.mask_2d,
             "chair": [dict(fr, labels=["chair"] * len(fr["labels"])) for fr in scene.mask_2d[1:]]}
    for debug_out in (False, True):
        got = project_scene_classes(scene, masks, cfg, DEV, debug_out=debug_out)
        assert calls == [RADIUS] * (1 + debug_out)
        for c, m in masks.items():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                e = pref.project_scene_ref(class_scene(ref_scene, m), cfg_for(ref_scene))
            assert len(e["final_class"]) >= 1
            same(got[c], e)


def test_key_off_makes_the_plain_call(lib, monkeypatch):
    """cloud_splat_radius absent or 0: render_depth is called exactly as before the key existed."""
    from beyond_fixed_forms_amd import _lib
    from beyond_fixed_forms_amd.ingest import prepare_geometry_fast
    from beyond_fixed_forms_amd.scene import prepare_geometry
    scene = generated()[0]
    seen = []
    real = _lib.render_depth
    monkeypatch.setattr(_lib, "render_depth", lambda *a, **k: (seen.append((len(a), sorted(k))), real(*a, **k))[1])
    for cfg in (cfg_for(scene, depth_from_cloud=STRIDE), cfg_for(scene, depth_from_cloud=STRIDE, cloud_splat_radius=0.0)):
        for prep in (prepare_geometry, prepare_geometry_fast):
            prep(scene, cfg, [scene.mask_2d], DEV, with_viewed=False)
    assert seen == [(9, [])] * 4
    for prep in (prepare_geometry, prepare_geometry_fast):
        with pytest.raises(ValueError, match="depth_from_cloud"):
            prep(scene, cfg_for(scene, cloud_splat_radius=RADIUS), [scene.mask_2d], DEV, with_viewed=False)


def test_repeat_run_gives_identical_bytes(lib, monkeypatch):
    from beyond_fixed_forms_amd.scene import prepare_geometry
    scene = generated()[0]
    cfg = cfg_for(scene, depth_from_cloud=STRIDE, cloud_splat_radius=RADIUS)
    monkeypatch.setenv("BFF_DEPTH_TILES", "0")
    a = prepare_geometry(scene, cfg, [scene.mask_2d], DEV, with_viewed=False).depth_raw.cpu().numpy().tobytes()
    b = prepare_geometry(scene, cfg, [scene.mask_2d], DEV, with_viewed=False).depth_raw.cpu().numpy().tobytes()
    assert a == b
    assert render(lib, 50, 70, 1, 3).tobytes() == render(lib, 50, 70, 1, 3).tobytes()
