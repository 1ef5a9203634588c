"""The masks' row directory (bff_mask_row_directory) entry for entry against NumPy, and the sweep's look-up mode against
the dense decode: every pixel of hand-made views, and whole scene calls under both values of BFF_MASK_LOOKUP.

Run as a script (`python tests/test_gpu_mask_rows.py OUT.npz`) this file is the scene test's worker: the switch is read
once per process, so each value gets a fresh child."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_rows_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = mr.H, mr.W


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def run_tables(views):
    """list of dense bool [m][H * W] -> (rs, re, offs, view_mask_offs) host arrays over all masks of all views."""
    dense = np.concatenate(views, axis=0) if views else np.zeros((0, H * W), bool)
    rs, re, offs = mr.runs_of(dense)
    voffs = np.concatenate([[0], np.cumsum([v.shape[0] for v in views])]).astype(np.int32)
    return dense, rs, re, offs, voffs


# ------------------------------------------------------------------ 1. the directory, entry for entry
@pytest.mark.parametrize("name", ["hand+second", "full64", "none"])
def test_directory_equals_reference(lib, name):
    views = {"hand+second": [mr.hand_view(34), mr.second_view()], "full64": [mr.full_box_view(64)], "none": []}[name]
    _, rs, re, offs, _ = run_tables(views)
    n = len(offs) - 1
    exp_tab, exp_dir = mr.row_directory_ref(rs, re, offs, H, W)
    tab, directory = lib.mask_row_directory(dev_i32(rs), dev_i32(re), dev_i32(offs), n, H, W,
                                            mask_dir=torch.full((max(n * H, 1),), -1, dtype=torch.int32, device=DEV))
    assert np.array_equal(u32(tab), exp_tab)
    got = u32(directory)
    assert np.array_equal(got[:exp_dir.size], exp_dir)
    assert (got[exp_dir.size:] == 0xFFFFFFFF).all()                  # nothing written past the last box


# ------------------------------------------------------------------ 2. / 4. every pixel looked up, both modes
def pixel_cloud(reps):
    """One point per pixel on the plane z = 1 (reps copies of the image): identity pose and intrinsics send point
    (u, v, 1) to pixel (u, v) exactly."""
    v, u = np.divmod(np.arange(H * W), W)
    xyz = np.tile(np.stack([u, v, np.ones_like(u)]).astype(np.float64), (1, reps))
    n = xyz.shape[1]
    soa = np.zeros((3, (n + 1023) // 1024 * 1024))
    soa[:, :n] = xyz
    return torch.from_numpy(soa).to(DEV), n


def sweep_both_modes(lib, views, frame_views, reps=1):
    """frame_views: per frame the index of its view or -1.  Returns the dense masks, the frames' row bases and the
    (rows, chunk_mask, masked, viewed) of the dense and of the look-up sweep."""
    dense, rs, re, offs, voffs = run_tables(views)
    wb = 32 if max(v.shape[0] for v in views) <= 32 else 64
    n_frames = len(frame_views)
    nmask = [views[v].shape[0] if v >= 0 else 0 for v in frame_views]
    rowbase = np.concatenate([[0], np.cumsum(nmask)])[:-1]
    n_rows = int(np.sum(nmask))
    soa, n = pixel_cloud(reps)
    nw = (n + 63) // 64
    pose = torch.eye(4, dtype=torch.float64).reshape(1, 16).repeat(n_frames, 1).to(DEV)
    depth = torch.ones((1, H * W), dtype=torch.float32, device=DEV)
    t = dict(rs=dev_i32(rs), re=dev_i32(re), offs=dev_i32(offs), voffs=dev_i32(voffs))
    frames = (dev_i32(frame_views), dev_i32(rowbase), dev_i32(nmask), dev_i32([1] * n_frames))
    head = (soa, n, pose, np.eye(3), depth, dev_i32([0] * n_frames), H, W, 0.08)
    bits = torch.zeros((len(views), H * W), dtype=torch.int32 if wb == 32 else torch.int64, device=DEV)
    lib.rle_to_maskbits(t["rs"], t["re"], t["offs"], t["voffs"], len(views), H * W, wb, bits)
    tab, directory = lib.mask_row_directory(t["rs"], t["re"], t["offs"], len(offs) - 1, H, W)
    out = []
    for mode in ("dense", "rows"):
        rows = torch.zeros((n_rows, nw), dtype=torch.int64, device=DEV)
        cm = lib.chunk_mask_buffer(n_rows, nw, DEV).zero_()
        mc = torch.zeros(n, dtype=torch.int32, device=DEV)
        vc = torch.zeros(n, dtype=torch.int32, device=DEV)
        if mode == "dense":
            lib.project_views(*head, bits, wb, *frames, rows, mc, vc, chunk_mask=cm)
        else:
            lib.project_views_lookup(*head, tab, directory, t["rs"], t["re"], t["voffs"], wb, *frames, rows, mc, vc,
                                     chunk_mask=cm)
        out.append((rows, cm, mc, vc))
    torch.cuda.synchronize()
    return dense, voffs, rowbase, out


def unpack(rows, n):
    return np.unpackbits(rows.cpu().numpy().view(np.uint8), axis=-1, bitorder="little")[:, :n].astype(bool)


CASES = {
    # 64-bit words: 34 masks, a second view with 3, a frame without masks
    "w64": (lambda: [mr.hand_view(34), mr.second_view()], [0, 1, -1], 1),
    "w32": (lambda: [mr.hand_view(30), mr.second_view()], [0, 1, -1], 1),
    # every mask a candidate at every pixel: the upper end of the candidate loop
    "full64": (lambda: [mr.full_box_view(64)], [0], 1),
    "full32": (lambda: [mr.full_box_view(32)], [0], 1),
    # 9 blocks of points x 999 frames: blocks take tiles of two frames, so the LDS tables hold more than one frame
    "tiles": (lambda: [mr.hand_view(34), mr.second_view()], [0, 1, -1] * 333, 10),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_pixel_looked_up(lib, case):
    make, frame_views, reps = CASES[case]
    views = make()
    dense, voffs, rowbase, (a, b) = sweep_both_modes(lib, views, frame_views, reps)
    for x, y, what in zip(a, b, ("rows", "chunk_mask", "masked_count", "viewed_count")):
        assert torch.equal(x, y), what
    n = reps * H * W
    cover = np.zeros(H * W, np.int64)
    for k, v in enumerate(frame_views):
        if v >= 0:
            cover += dense[voffs[v]:voffs[v + 1]].sum(0)
    for rows, _, mc, vc in (a, b):
        assert np.array_equal(mc.cpu().numpy(), np.tile(cover, reps))
        assert (vc.cpu().numpy() == len(frame_views)).all()
        bits = unpack(rows, n)
        for k, v in enumerate(frame_views[:3]):
            if v >= 0:
                assert np.array_equal(bits[rowbase[k]:rowbase[k] + views[v].shape[0]], np.tile(dense[voffs[v]:voffs[v + 1]], (1, reps)))


# ------------------------------------------------------------------ 3. whole scene calls under both switch values
MANY = dict(cut_masks=False, n_objects=40, distinct_masks=True, dilate=False)        # bench.py's "many" keywords
SCENES = {"tiny": dict(seed=3), "tiny40": dict(seed=4, n_masks=40), "many": dict(seed=1, **MANY)}


def worker(out_path):
    """Every scene of SCENES, with float32 (H, W) depth and with 16-bit sensor depth in tiles, through the scene call of
    this process (BFF_MASK_LOOKUP as inherited) -> one .npz of everything the call delivers."""
    os.environ["BFF_DEPTH_TILES"] = "u16"
    from beyond_fixed_forms_amd import _lib, pipeline
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.projection import projection_back, projection_front
    from beyond_fixed_forms_amd.scene import DEPTH_THRESH, prepare_scene, with_viewed_counts
    from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth
    _lib.load()
    out = {}
    for name, kw in SCENES.items():
        for form in ("f32", "u16"):
            scene = make_scene("tiny", **kw)
            cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
            if form == "u16":
                scene = with_sensor_depth(scene)
            ds = prepare_scene(scene, cfg, device=DEV, raw_depth_resident=True if form == "u16" else None)
            assert (ds.depth_raw is not None and ds.depth_raw.dtype == torch.int16 and ds.depth_size is not None) == (form == "u16")
            key = f"{name}_{form}_"
            out[key + "lookup"] = np.asarray(_lib.mask_lookup_rows(ds.height, ds.width, ds.n_rows))
            out[key + "word_bits"] = np.asarray(ds.word_bits)
            h = pipeline.issue(ds, cfg, DEPTH_THRESH, None, ds.n_frames if with_viewed_counts(cfg) else ds.n_mask_frames, None)
            out[key + "hdr"] = pipeline.collect(h)
            ws = h["ws"]
            out[key + "both"] = h["both"].cpu().numpy()
            out[key + "masked"] = ws.view("masked", ds.n_points).cpu().numpy()
            out[key + "viewed"] = ws.view("viewed", ds.n_points).cpu().numpy()
            res = projection_back(projection_front(ds, cfg))
            out[key + "rows"] = np.zeros((0, ds.nw), np.int64) if res.rows is None else res.rows.cpu().numpy()
            out[key + "conf"] = np.zeros(0, np.float32) if res.conf is None else res.conf.float().cpu().numpy()
            out[key + "final_class"] = np.asarray(res.final_class)
    np.savez(out_path, **out)


def test_scene_call_is_the_same_under_both_switch_values(tmp_path):
    got = {}
    for mode in ("rows", "dense"):
        path = str(tmp_path / f"{mode}.npz")
        env = dict(os.environ, BFF_MASK_LOOKUP=mode)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, cwd=root, timeout=300)
        got[mode] = np.load(path)
    a, b = got["rows"], got["dense"]
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 9 * 2 * len(SCENES)
    for k in a.files:
        if k.endswith("_lookup"):
            assert bool(a[k]) and not bool(b[k]), k               # each child really took its path
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert int(a["tiny_f32_word_bits"]) == 32 and int(a["tiny40_u16_word_bits"]) == 64
    assert any(a[f"{s}_{f}_rows"].shape[0] > 0 for s in SCENES for f in ("f32", "u16"))


if __name__ == "__main__":
    worker(sys.argv[1])
