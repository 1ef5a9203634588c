"""3-D instances rendered back into the views, the parts that need no GPU: the NumPy statements of tests/label_render_ref.py
pinned against the depth renderers' statements, a brute-force loop per texel and the RLE oracle; the config keys; the
header, the binding table and the library's exports.  Every comparison is for equality."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import label_render_ref as lr
import mesh_depth_ref as md
import render_depth_ref as rd
import splat_depth_ref as sd
from oracle import geom_fma, rle_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K33 = np.array([[64.0, 0.0, 34.5], [0.0, 64.0, 24.5], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def cloud70():
    return lr.label_cloud(70)


@pytest.mark.parametrize("h,w,stride,nf,radius", [(50, 70, 1, 3, 0.0), (50, 70, 3, 4, lr.R), (48, 64, 2, 3, lr.R),
                                                   (48, 64, 8, 9, 0.0)])
def test_depth_half_is_the_depth_renderers_statement(h, w, stride, nf, radius):
    xyz, inv, _, lab = cloud70()
    n = xyz.shape[0]
    dh, dw = rd.rendered_size(h, w, stride)
    labels, depth = lr.render_labels_ref(xyz, lab[:n], inv[:nf], K33, h, w, dh, dw, radius)
    exp = sd.render_splat_ref(xyz, inv[:nf], K33, h, w, dh, dw, radius) if radius else \
        rd.render_depth_ref(xyz, inv[:nf], K33, h, w, dh, dw)
    assert depth.dtype == np.uint16 and np.array_equal(depth, exp)
    assert not labels[depth == 0].any() and labels.max() <= 70 and len(np.unique(labels)) > 10
    assert (labels[depth != 0] == 0).any()                              # background points hold texels of their own


def test_crafted_pairs_by_hand():
    """Frame 0 (the identity pose) at stride 1, radius 0: the four crafted pixels of label_cloud, for K = 3 and 70."""
    for k in (3, 70):
        xyz, inv, _, lab = lr.label_cloud(k)
        n, hi = xyz.shape[0], min(5, k)
        assert (lab[:n] == 0).sum() > n // 3 and (lab[:n] != 0).sum() > n // 3 and lab[:n].max() == k
        for h, w in ((50, 70), (48, 64)):
            labels, depth = lr.render_labels_ref(xyz, lab[:n], inv[:1], K33, h, w, h, w)
            at = lambda px, img: int(img[0, px[1], px[0]])
            assert at(lr.PIX_TIE, labels) == 2 and at(lr.PIX_TIE, depth) == 300
            assert at(lr.PIX_TIE_BG, labels) == 0 and at(lr.PIX_TIE_BG, depth) == 300
            assert at(lr.PIX_BEHIND, labels) == 0 and at(lr.PIX_BEHIND, depth) == 300
            assert at(lr.PIX_FRONT, labels) == hi and at(lr.PIX_FRONT, depth) == 300
            assert not (depth == 100).any()                              # the padding's point is never read


@pytest.mark.parametrize("radius", [0.0, lr.R, 0.25])
def test_label_half_equals_a_loop_per_texel(radius):
    """A 12 x 16 frame of a 48 x 64 image (stride 4): for every texel, every point that takes part is asked whether it
    offers its key there -- own texel, or sample point within the footprint, the header's comparison taken literally."""
    xyz, inv, _, lab = cloud70()
    n = xyz.shape[0]
    h, w, dh, dw = 48, 64, 12, 16
    X, Y = md.sample_points(h, w, dh, dw)
    for f in (0, 3):
        pts, pix, _ = geom_fma.view(xyz, inv[f].reshape(4, 4), K33, np.zeros((1, 1), np.float32))
        part = lr.taking_part(xyz, inv[f], K33, h, w)
        exp_l, exp_d = np.zeros((dh, dw), np.uint16), np.zeros((dh, dw), np.uint16)
        for i in range(dh):
            for j in range(dw):
                best = None
                for p in part:
                    u, v, cz = int(pix[p, 0]), int(pix[p, 1]), pts[p, 2]
                    own = (v * dh) // h == i and (u * dw) // w == j
                    foot = radius > 0 and abs(X[j] - float(u)) <= (K33[0, 0] * radius) / cz and \
                        abs(Y[i] - float(v)) <= (K33[1, 1] * radius) / cz
                    if own or foot:
                        key = (int(np.rint(cz * 1000.0)), int(lab[p]))
                        best = key if best is None or key < best else best
                if best is not None:
                    exp_d[i, j], exp_l[i, j] = best
        labels, depth = lr.render_labels_ref(xyz, lab[:n], inv[f:f + 1], K33, h, w, dh, dw, radius)
        assert np.array_equal(labels[0], exp_l) and np.array_equal(depth[0], exp_d)
        assert exp_l.any() and (exp_d != 0).sum() > 20


def test_point_labels_statement():
    rng = np.random.default_rng(5)
    dense = rng.random((5, 200)) < 0.3
    dense[3] = False                                                    # an empty row
    lab = lr.point_labels_ref(dense)
    for p in range(200):
        held = np.flatnonzero(dense[:, p])
        assert lab[p] == (held[0] + 1 if len(held) else 0)
    assert (dense.sum(0) > 1).any() and (lab == 0).any() and 4 not in lab
    perm = rng.permutation(200)
    unsort = np.empty(200, np.int64)
    unsort[perm] = np.arange(200)
    assert np.array_equal(lr.point_labels_ref(dense, unsort), lab[perm])          # sorted position s holds point perm[s]


def label_images():
    """(label frames, height, width, min_pixels) of the runs statement's cases."""
    xyz, inv, _, lab = cloud70()
    n = xyz.shape[0]
    rendered, _ = lr.render_labels_ref(xyz, lab[:n], inv[:3], K33, 50, 70, 17, 24, lr.R)
    hand = np.zeros((5, 6, 8), np.uint16)
    hand[0] = 3                                                          # a whole frame of one label
    hand[1, 5, 7] = 2                                                    # a single last pixel
    hand[3].reshape(-1)[::2] = 1                                         # alternating every pixel ...
    hand[3].reshape(-1)[1::2] = 4
    hand[4, 2, 3:5] = 9                                                  # present in one frame only, 2 pixels
    hand[4, 0:2] = 1
    return [(rendered, 50, 70, 1), (hand, 6, 8, 1), (hand, 6, 8, 3), (hand, 13, 20, 1), (hand, 4, 5, 1)]


@pytest.mark.parametrize("case", range(5))
def test_runs_statement_equals_the_rle_oracle(case):
    from beyond_fixed_forms_amd.scene import runs_from_rles
    labels, h, w, min_pixels = label_images()[case]
    start, end, offs, mask_label, frame_offs = lr.label_runs_ref(labels, h, w, min_pixels)
    up = lr.upsample(labels, h, w)
    assert up.shape == (labels.shape[0], h, w)
    dense, names, per_frame = [], [], [0]
    for f in range(up.shape[0]):
        for lab in range(1, int(up.max()) + 1):
            m = up[f] == lab
            if m.sum() >= max(1, min_pixels):
                dense.append(m.reshape(-1)), names.append(lab - 1)
        per_frame.append(len(names))
    rles = rle_ref.rle_encode_batch_ref(torch.from_numpy(np.stack(dense)))
    s, e, o = runs_from_rles(rles)
    assert np.array_equal(start, s) and np.array_equal(end, e) and np.array_equal(offs, o)
    assert mask_label.tolist() == names and frame_offs == per_frame
    assert start.dtype == end.dtype == offs.dtype == mask_label.dtype == np.int32
    if case == 1:
        assert (start[0], end[0]) == (0, 48) and offs[1] == 1           # one run across every row end
        assert (start[1], end[1]) == (47, 48) and frame_offs[:4] == [0, 1, 2, 2]
        assert offs[3] - offs[2] == 24 and 8 in names                   # 24 one-pixel runs; the 2-pixel mask is kept ...
    if case == 2:
        assert 8 not in names and len(names) == 4                        # ... and dropped, with the single pixel, at 3


def test_config_keys():
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    from beyond_fixed_forms_amd import reproject as rp
    assert (DEFAULTS["reproject_stride"], DEFAULTS["reproject_splat_radius"], DEFAULTS["reproject_min_pixels"],
            DEFAULTS["reprojected_2d_dir"]) == (1, 0.0, 1, None)
    assert rp.reproject_stride(Config()) == 1 and rp.reproject_splat_radius(Config()) == 0.0 and rp.reproject_min_pixels(Config()) == 1
    cfg = Config.with_defaults(reproject_stride=4, reproject_splat_radius=0.02, reproject_min_pixels=10)
    assert (rp.reproject_stride(cfg), rp.reproject_splat_radius(cfg), rp.reproject_min_pixels(cfg)) == (4, 0.02, 10)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="reproject_stride"):
            rp.reproject_stride(Config(reproject_stride=bad))
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reproject_splat_radius"):
            rp.reproject_splat_radius(Config(reproject_splat_radius=bad))
    assert rp.rendered_size(50, 70, 3) == (17, 24) == rd.rendered_size(50, 70, 3)
    text = open(os.path.join(ROOT, "configs", "config.yaml")).read()
    for key in ("reproject_stride", "reproject_splat_radius", "reproject_min_pixels", "reprojected_2d_dir"):
        assert re.search(rf"^# {key}:", text, re.M), key                # documented, commented out


def test_no_cpu_path():
    from beyond_fixed_forms_amd import reproject as rp
    with pytest.raises(ValueError, match="no CPU"):
        rp.point_labels(torch.zeros((2, 4), dtype=torch.int64), 200)
    with pytest.raises(ValueError, match="no CPU"):
        rp.label_runs(torch.zeros((1, 4, 4), dtype=torch.int16), 4, 4)
    scene, _, _ = rd.two_plane_scene()
    with pytest.raises(ValueError, match="GPU"):
        rp.geometry_for_frames(scene, dict(height_2d=48, width_2d=64), ["0"], device="cpu")


def header_args(header, name):
    m = re.search(rf"int {name}\(([^;]*)\);", header)
    assert m, f"{name} is not declared"
    from beyond_fixed_forms_amd import _lib
    kinds, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(arg.split()[-1].lstrip("*"))
        kinds.append(_lib._P if "*" in arg else {"int64_t": _lib._L, "int32_t": _lib._I, "double": _lib._D,
                                                 "float": _lib._F}[arg.split()[0]])
    return kinds, names


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 16
    for name in ("bff_point_labels", "bff_render_labels_u16", "bff_label_runs_count", "bff_label_runs_emit"):
        kinds, _ = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
    kinds, names = header_args(header, "bff_render_labels_u16")
    splat, _ = header_args(header, "bff_render_splat_depth_u16")
    # the splat renderer's arguments with `lab` after n_pad and a second frame pointer after the first
    assert names[3] == "lab" and names[-4:-2] == ["labels_u16", "depth_u16"]
    assert kinds[:3] + kinds[4:-3] + kinds[-2:] == splat
    assert _lib.PLAIN["bff_label_runs_tile_pixels"] == (_lib.c_int32, [])
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\brender_labels\.hip\b", makefile, re.M)
    assert re.search(r"^_obj/.*render_labels\.o.*:.*geom\.h", makefile, re.M)


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU."""
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_abi_version() == 16 and lib.bff_label_runs_tile_pixels() == 8192
    N = None
    # (rows, n_rows, nw, n_points, unsort, lab, stream)
    assert lib.bff_point_labels(N, 3, 4, 0, N, N, N) == 0               # no points: nothing to do
    assert lib.bff_point_labels(N, 65535, 4, 0, N, N, N) == -2 and b"65534" in lib.bff_last_error()
    assert lib.bff_point_labels(N, 3, 3, 200, N, N, N) == -1            # 200 points need 4 words
    assert lib.bff_point_labels(N, 3, 4, 200, N, N, N) == -1 and b"null" in lib.bff_last_error()
    # (xyz, n_points, n_pad, lab, inv_pose, K, n_frames, H, W, dh, dw, splat_radius, frames_per_block, scratch, labels, depth,
    #  tile_bounds, stream)
    fn = lib.bff_render_labels_u16
    for ok in (0.0, 0.02):
        assert fn(N, 0, 0, N, N, N, 0, 50, 70, 7, 9, ok, 0, N, N, N, N, N) == 0          # no frames: nothing to do
    for bad in (-0.02, float("nan"), float("inf"), -float("inf")):
        assert fn(N, 0, 0, N, N, N, 0, 50, 70, 7, 9, bad, 0, N, N, N, N, N) == -1 and b"splat_radius" in lib.bff_last_error()
    assert fn(N, 0, 0, N, N, N, 65536, 50, 70, 7, 9, 0.0, 0, N, N, N, N, N) == -2       # the depth renderer's limits
    assert fn(N, 0, 0, N, N, N, 1, 50, 70, 7, 9, 0.0, 0, N, N, N, N, N) == -1           # frames but no output pointer
    # (labels, n_frames, dh, dw, H, W, n_labels, n_runs, n_pix, stream)
    assert lib.bff_label_runs_count(N, 0, 7, 9, 50, 70, 3, N, N, N) == 0
    assert lib.bff_label_runs_count(N, 2, 7, 9, 50, 70, 3, N, N, N) == -1
    assert lib.bff_label_runs_count(N, 2, 7, 9, 65536, 32768, 3, N, N, N) == -2         # H * W = 2^31
    assert lib.bff_label_runs_count(N, 65536, 7, 9, 50, 70, 3, N, N, N) == -2
    # (labels, n_frames, dh, dw, H, W, n_labels, mask_index, total_runs, cursor, start_keys, end_keys, stream)
    assert lib.bff_label_runs_emit(N, 2, 7, 9, 50, 70, 3, N, 0, N, N, N, N) == 0
    assert lib.bff_label_runs_emit(N, 2, 7, 9, 50, 70, 3, N, 1 << 31, N, N, N, N) == -2
    assert lib.bff_label_runs_emit(N, 2, 7, 9, 50, 70, 3, N, 5, N, N, N, N) == -1
