"""The views of 3-D instances, the parts that need no GPU: the NumPy statement of tests/views_ref.py against a literal
per-point loop on the synthetic tables of tests/vis_table_synth.py; the order of the top views; the crops by hand; the
header, the binding table, the library's exports and host-side argument checks; the config keys; the tool's parser.
Every comparison is for equality."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import views_ref as wr
import vis_table_synth as vs
from test_spatial_host import header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bff_instance_views", "bff_select_views")
SENT = lambda h, w: [w, h, -1, -1]


def random_rows(rng, k, n):
    """uint64 [k][nw]: random densities; row 0 empty, row 1 (if any) all ones, the last two equal."""
    bits = rng.random((k, n)) < rng.choice([0.02, 0.2, 0.7], size=(k, 1))
    bits[0] = False
    if k > 1:
        bits[1] = True
    if k > 3:
        bits[-1] = bits[-2]
    return wr.pack(bits)


@pytest.mark.parametrize("n,h,w", [(1, 3, 5), (63, 7, 9), (64, 4, 4), (65, 30, 50), (200, 37, 41), (1025, 16, 300)])
def test_statement_equals_the_point_loop(n, h, w):
    rng = np.random.default_rng(n)
    mask, off, pix = vs.synthetic_table(n, [0.5, 0.0, 1.0, 0.1], h, w, rng, hot_share=0.3, hot_pixels=5)
    assert mask.shape == (4, (n + 1023) // 1024 * 16) and mask.shape[1] > (n + 63) // 64 - 1
    rows = random_rows(rng, 5, n)
    visible, box, area = wr.instance_views(rows, mask, off, pix, n, h, w)
    lv, lb = wr.instance_views_loop(rows, mask, off, pix, n, h, w)
    assert visible.dtype == box.dtype == area.dtype == np.int32 and box.shape == (5, 4, 4)
    assert np.array_equal(visible, lv) and np.array_equal(box, lb)
    # the identity: visible = popcount(row & mask), area = popcount(row)
    nw = (n + 63) // 64
    both = rows[:, None, :] & mask[None, :, :nw]
    assert np.array_equal(visible, wr.unpack(both.reshape(-1, nw), nw * 64).sum(axis=1).reshape(5, 4))
    assert area.tolist() == wr.unpack(rows, n).sum(axis=1).tolist() and area[0] == 0 and area[1] == n
    # the empty row and the slot without a pair keep the sentinel; the row of all ones sees every pair of a slot
    assert (box[0] == SENT(h, w)).all() and (box[:, 1] == SENT(h, w)).all() and not visible[0].any() and not visible[:, 1].any()
    assert visible[1, 2] == n and np.array_equal(visible[-1], visible[-2]) and np.array_equal(box[-1], box[-2])
    assert ((box[..., 2] < w) & (box[..., 3] < h)).all()
    seen = visible > 0
    assert (box[seen][:, 0] <= box[seen][:, 2]).all() and (box[seen][:, 1] <= box[seen][:, 3]).all()


def test_table_from_dense_is_the_synthetic_layout():
    rng = np.random.default_rng(3)
    n, h, w = 130, 9, 11
    mask, off, pix = vs.synthetic_table(n, [0.4, 1.0, 0.0], h, w, rng)
    vis = np.stack([wr.slot_pixels(mask, off, pix, s, n)[0] for s in range(3)])
    u = np.stack([wr.slot_pixels(mask, off, pix, s, n)[1] for s in range(3)])
    v = np.stack([wr.slot_pixels(mask, off, pix, s, n)[2] for s in range(3)])
    again = wr.table_from_dense(vis, u, v, mask.shape[1])
    for a, b in zip(again, (mask, off, pix)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def boxes_for(visible, h, w):
    """A distinct valid box per (instance, slot) with a count, the sentinel elsewhere."""
    k, f = visible.shape
    box = np.tile(np.array(SENT(h, w), np.int32), (k, f, 1))
    for i in range(k):
        for s in range(f):
            if visible[i, s] > 0:
                box[i, s] = [s % w, i % h, min(w - 1, s % w + 3), min(h - 1, i % h + 2)]
    return box


def test_top_view_order():
    h, w = 40, 60
    visible = np.array([[5, 9, 9, 0, 2, 9, 1],           # ties go to the earlier slot
                        [0, 0, 0, 0, 0, 0, 0],           # no candidate at all
                        [3, 3, 3, 3, 3, 3, 3],           # a pure tie
                        [0, 1, 0, 0, 4, 0, 0]], np.int32)
    box = boxes_for(visible, h, w)
    top, tv, crops = wr.select_views(visible, box, h, w, top_k=5, min_points=1, levels=2, expand=0.0)
    assert top.tolist() == [[1, 2, 5, 0, 4], [-1] * 5, [0, 1, 2, 3, 4], [4, 1, -1, -1, -1]]
    assert tv.tolist() == [[9, 9, 9, 5, 2], [0] * 5, [3] * 5, [4, 1, 0, 0, 0]]
    assert (crops[1] == SENT(h, w)).all() and (crops[3, 2:] == SENT(h, w)).all()
    assert crops[0, 0].tolist() == [box[0, 1].tolist()] * 2 and crops[3, 1, 1].tolist() == box[3, 1].tolist()    # r = 0: the box
    # min_points cuts candidates; 0 and negative values still ask for one point
    top, tv, _ = wr.select_views(visible, box, h, w, top_k=3, min_points=3, levels=1, expand=0.1)
    assert top.tolist() == [[1, 2, 5], [-1, -1, -1], [0, 1, 2], [4, -1, -1]] and tv[3].tolist() == [4, 0, 0]
    for need in (0, -7, 1):
        assert wr.select_views(visible, box, h, w, 7, need, 1, 0.1)[0][0].tolist() == [1, 2, 5, 0, 4, 6, -1]
    # T larger than F
    top, tv, crops = wr.select_views(visible[:, :2], box[:, :2], h, w, top_k=64, min_points=1, levels=3, expand=0.1)
    assert top.shape == (4, 64) and crops.shape == (4, 64, 3, 4)
    assert top[0].tolist() == [1, 0] + [-1] * 62 and tv[0].tolist() == [9, 5] + [0] * 62 and (crops[0, 2:] == SENT(h, w)).all()
    # no slot at all
    top, tv, crops = wr.select_views(np.zeros((2, 0), np.int32), np.zeros((2, 0, 4), np.int32), h, w, 2, 1, 2, 0.1)
    assert top.tolist() == [[-1, -1]] * 2 and not tv.any() and (crops == SENT(h, w)).all()


# (box, H, W, r) -> the crops of levels 0, 1, 2, worked out by hand
CROP_CASES = [
    # one pixel column: u1 == u0, so ex = 0 at every level; v: floor(20 * 0.1) = 2
    ((7, 10, 7, 30), 100, 100, 0.1, [(7, 10, 7, 30), (7, 8, 7, 32), (7, 6, 7, 34)]),
    # r = 0: the box at every level
    ((5, 6, 50, 60), 100, 100, 0.0, [(5, 6, 50, 60)] * 3),
    # clipping at all four borders: floor(90 * 0.5) = 45, floor(70 * 0.5) = 35
    ((3, 2, 93, 72), 75, 96, 0.5, [(3, 2, 93, 72), (0, 0, 95, 74), (0, 0, 95, 74)]),
    # clipping left and top only / right and bottom only: floor(10 * 0.4) = 4
    ((2, 3, 12, 13), 100, 100, 0.4, [(2, 3, 12, 13), (0, 0, 16, 17), (0, 0, 20, 21)]),
    ((88, 87, 98, 97), 100, 100, 0.4, [(88, 87, 98, 97), (84, 83, 99, 99), (80, 79, 99, 99)]),
    # sides of 29 and 30: 29 * 0.1 = 2.9000000000000004 -> 2; 30 * 0.1 = 3.0 exactly -> 3 (IEEE float64: the double nearest 0.1
    # lies above it by 5.6e-18; 30 times that is 1.7e-16 above 3, less than half the spacing 4.4e-16 of the doubles there,
    # so the product rounds to 3.0 and not to 3.0000000000000004)
    ((100, 100, 129, 130), 480, 640, 0.1, [(100, 100, 129, 130), (98, 97, 131, 133), (96, 94, 133, 136)]),
    # a one-pixel box; an expand far beyond the image (cut at 2^15: the whole side either way)
    ((4, 4, 4, 4), 10, 10, 3.0, [(4, 4, 4, 4)] * 3),
    ((4, 4, 5, 6), 10, 12, 1e300, [(4, 4, 5, 6), (0, 0, 11, 9), (0, 0, 11, 9)]),
]


def test_ieee_products_are_pinned():
    assert 29 * 0.1 == 2.9000000000000004 and math.floor(29 * 0.1) == 2
    assert 30 * 0.1 == 3.0 and 30 * 0.1 != 3.0000000000000004 and math.floor(30 * 0.1) == 3
    assert 3 * 0.1 == 0.30000000000000004 and 0.1 * 3 != 0.3                          # the product that does round up
    assert wr.expansion(29, 0.1, 1) == 2 and wr.expansion(30, 0.1, 1) == 3 and wr.expansion(30, 0.1, 2) == 6
    assert wr.expansion(0, 0.1, 2) == 0 and wr.expansion(7, 0.0, 2) == 0 and wr.expansion(50, 0.1, 0) == 0
    assert wr.expansion(3, 1e300, 1) == 32768 and wr.expansion(32766, 1.0, 2) == 65532


@pytest.mark.parametrize("case", range(len(CROP_CASES)))
def test_crops_by_hand(case):
    b, h, w, r, want = CROP_CASES[case]
    assert [wr.crop(b, h, w, r, l) for l in range(3)] == want
    visible = np.array([[0, 6]], np.int32)
    box = np.array([[SENT(h, w), list(b)]], np.int32)
    top, tv, crops = wr.select_views(visible, box, h, w, top_k=2, min_points=1, levels=3, expand=r)
    assert top.tolist() == [[1, -1]] and tv.tolist() == [[6, 0]]
    assert crops[0, 0].tolist() == [list(c) for c in want] and (crops[0, 1] == SENT(h, w)).all()


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name in NAMES:
        kinds, names = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
        assert names[-1] == "stream"
    assert header_args(header, "bff_instance_views")[1] == ["rows", "n_rows", "nw", "vis_mask", "vis_off", "vis_pix", "n_slots",
                                                           "stride", "n_pixels", "height", "width", "visible", "box", "stream"]
    kinds, names = header_args(header, "bff_select_views")
    assert names == ["visible", "box", "n_rows", "n_slots", "height", "width", "top_k", "min_points", "levels", "expand", "top",
                     "top_visible", "crops", "stream"]
    assert kinds[9] is _lib._D                                                        # expand is a double
    assert re.search(r"int32_t bff_instance_views_lds_words\(void\);", header)
    assert _lib.PLAIN["bff_instance_views_lds_words"] == (ctypes.c_int32, [])
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bviews\.hip\b", makefile, re.M)
    assert "-ffp-contract=off" in makefile


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU.  A non-null pointer here is never
    followed: every call below returns before its launch."""
    from beyond_fixed_forms_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)                                                  # the symbols resolve without a GPU
    assert all(hasattr(raw, name) for name in NAMES + ("bff_instance_views_lds_words",))
    lib = _lib.load()
    assert _lib.instance_views_lds_words() == lib.bff_instance_views_lds_words() > 0
    N, X = None, 64
    err = lambda: lib.bff_last_error()
    # (rows, n_rows, nw, vis_mask, vis_off, vis_pix, n_slots, stride, n_pixels, height, width, visible, box, stream)
    fn = lib.bff_instance_views
    assert fn(N, 0, 4, N, N, N, 3, 16, 0, 8, 8, N, N, N) == 0 and fn(N, 3, 4, N, N, N, 0, 16, 0, 8, 8, N, N, N) == 0    # K or F = 0
    assert fn(X, -1, 4, X, X, X, 3, 16, 9, 8, 8, X, X, N) == -1 and fn(X, 3, 4, X, X, X, -1, 16, 9, 8, 8, X, X, N) == -1
    assert fn(X, 3, 4, X, X, X, 3, 16, 9, 0, 8, X, X, N) == -1 and b"image" in err()
    assert fn(X, 3, 17, X, X, X, 3, 16, 9, 8, 8, X, X, N) == -1 and b"stride" in err()          # stride < nw
    assert fn(X, 3, 4, X, X, X, 3, 16, -1, 8, 8, X, X, N) == -1
    assert fn(X, 3, 4, X, X, X, 65536, 16, 9, 8, 8, X, X, N) == -2 and b"65536" in err() and b"65535" in err()
    assert fn(X, 3, 4, X, X, X, 3, 16, 9, 1 << 15, 8, X, X, N) == -2 and fn(X, 3, 4, X, X, X, 3, 16, 9, 8, 1 << 15, X, X, N) == -2
    assert b"packed" in err()
    assert fn(X, 1 << 14, 4, X, X, X, 1 << 15, 16, 9, 8, 8, X, X, N) == -2 and b"2^31" in err()     # K F 4 = 2^31
    assert fn(N, 3, 4, X, X, X, 3, 16, 9, 8, 8, X, X, N) == -1 and b"null" in err()
    assert fn(X, 3, 4, X, X, N, 3, 16, 9, 8, 8, X, X, N) == -1 and fn(X, 3, 4, X, X, X, 3, 16, 9, 8, 8, X, N, N) == -1
    assert fn(X, 3, 4, X, X, X, 3, 16, 9, 8, 8, X, 68, N) == -1 and b"aligned" in err()
    # (visible, box, n_rows, n_slots, height, width, top_k, min_points, levels, expand, top, top_visible, crops, stream)
    fn = lib.bff_select_views
    assert fn(N, N, 0, 3, 8, 8, 5, 1, 3, 0.1, N, N, N, N) == 0 and fn(N, N, 3, 0, 8, 8, 5, 1, 3, 0.1, N, N, N, N) == 0
    assert fn(X, X, -1, 3, 8, 8, 5, 1, 3, 0.1, X, X, X, N) == -1
    for bad in (float("nan"), float("inf"), -0.5):
        assert fn(X, X, 2, 3, 8, 8, 5, 1, 3, bad, X, X, X, N) == -1 and b"expand" in err()
    for top_k in (0, 65, -1):
        assert fn(X, X, 2, 3, 8, 8, top_k, 1, 3, 0.1, X, X, X, N) == -2 and b"top_k" in err()
    for levels in (0, 9):
        assert fn(X, X, 2, 3, 8, 8, 5, 1, levels, 0.1, X, X, X, N) == -2 and b"levels" in err()
    assert fn(X, X, 2, 65536, 8, 8, 5, 1, 3, 0.1, X, X, X, N) == -2 and fn(X, X, 2, 3, 1 << 15, 8, 5, 1, 3, 0.1, X, X, X, N) == -2
    assert fn(X, X, 1 << 14, 1 << 15, 8, 8, 5, 1, 3, 0.1, X, X, X, N) == -2 and b"2^31" in err()
    assert fn(X, X, 2, 3, 8, 8, 5, 1, 3, 0.1, N, X, X, N) == -1 and b"null" in err()
    assert fn(N, X, 2, 3, 8, 8, 5, 1, 3, 0.1, X, X, X, N) == -1 and fn(X, X, 2, 3, 8, 8, 5, 1, 3, 0.1, X, X, N, N) == -1
    assert fn(X, X, 2, 3, 8, 8, 5, 1, 3, 0.1, X, X, 72, N) == -1 and b"aligned" in err()


def test_config_keys():
    from beyond_fixed_forms_amd import views
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    want = dict(top_k=5, min_points=1, levels=3, expand=0.1)                           # OpenMask3D's, untuned here
    assert views.check_config(Config.with_defaults()) == want == views.check_config({})
    assert DEFAULTS["views_output_dir"] is None
    assert views.check_config({"views_top_k": 64, "views_min_points": 200, "views_crop_levels": 8, "views_crop_expand": 0}) == \
        dict(top_k=64, min_points=200, levels=8, expand=0.0)
    assert views.views_crop_expand({"views_crop_expand": 2}) == 2.0
    for key, bad in (("views_top_k", 0), ("views_top_k", 65), ("views_top_k", 2.5), ("views_top_k", True), ("views_top_k", "5"),
                     ("views_min_points", 0), ("views_min_points", -1), ("views_min_points", 1.5),
                     ("views_crop_levels", 0), ("views_crop_levels", 9), ("views_crop_levels", "3"),
                     ("views_crop_expand", -0.1), ("views_crop_expand", float("nan")), ("views_crop_expand", float("inf")),
                     ("views_crop_expand", "0.1"), ("views_crop_expand", True)):
        with pytest.raises(ValueError, match=key):
            views.check_config({key: bad})
    text = open(os.path.join(ROOT, "configs", "config.yaml")).read()
    for key in ("views_output_dir", "views_top_k", "views_min_points", "views_crop_levels", "views_crop_expand"):
        assert re.search(rf"^# {key}:", text, re.M), key


def test_no_cpu_path_and_input_kinds():
    from beyond_fixed_forms_amd import views
    rows = torch.zeros((2, 1), dtype=torch.int64)
    table = (torch.zeros((3, 16), dtype=torch.int64), torch.zeros((3, 16), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="no CPU"):
        views.instance_views(table, rows, 40, 8, 8)
    with pytest.raises(TypeError, match="VisibilityTable"):
        views.instance_views(table[:3], rows, 40, 8, 8)
    with pytest.raises(ValueError, match="no CPU"):
        views.select_views(torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3, 4), dtype=torch.int32), 8, 8)
    geom = type("G", (), dict(geometry=None, slot={}, sweep_depth=None))()
    with pytest.raises(ValueError, match="views_top_k"):                              # the config is read first
        views.scene_views(geom, None, {"views_top_k": 0})
    with pytest.raises(ValueError, match="depth frames"):
        views.scene_views(geom, None, {})


def test_tool_parser_and_missing_keys(tmp_path, capsys):
    from beyond_fixed_forms_amd import cli
    p = cli._select_views_parser()
    args = p.parse_args(["--config", "c.yaml", "--cls", "office chair"])
    assert (args.config, args.cls, args.stage, args.every, args.assembled) == ("c.yaml", "office chair", "final", None, False)
    args = p.parse_args(["--config", "c", "--cls", "x", "--stage", "mask_3d", "--every", "4"])
    assert (args.stage, args.every) == ("mask_3d", 4)
    args = p.parse_args(["--config", "c", "--assembled"])
    assert (args.cls, args.assembled) == (None, True)
    for bad in (["--cls", "x"], ["--config", "c", "--cls", "x", "--stage", "s"], ["--config", "c", "--cls", "x", "--every", "n"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    cfg = tmp_path / "config.yaml"
    base = f"final_output_dir: {tmp_path}/final\nmask_3d_dir: {tmp_path}/mask_3d\nscene_npy_dir: {tmp_path}/npy\n" \
           f"scene_2d_dir: {tmp_path}/2d\ndownsample_ratio: 10\n"
    out = f"views_output_dir: {tmp_path}/views\n"
    cfg.write_text(base + out)
    with pytest.raises(SystemExit):                                                   # neither --cls nor --assembled
        cli.select_views_main(["--config", str(cfg)])
    capsys.readouterr()
    assert cli.select_views_main(["--config", str(cfg), "--cls", "table"]) == 1
    assert "not a directory" in capsys.readouterr().err
    with pytest.raises(ValueError, match="assembled_output_dir"):
        cli.select_views_main(["--config", str(cfg), "--assembled"])
    (tmp_path / "final" / "table").mkdir(parents=True)
    for text, key in (("", "views_output_dir"), (out + "views_top_k: 0\n", "views_top_k"),
                      (out + "views_min_points: 0\n", "views_min_points"), (out + "views_crop_levels: 9\n", "views_crop_levels"),
                      (out + "views_crop_expand: -1\n", "views_crop_expand")):
        cfg.write_text(base + text)
        with pytest.raises(ValueError, match=key):                                    # before the first scene
            cli.select_views_main(["--config", str(cfg), "--cls", "table"])
    cfg.write_text(base + out)
    with pytest.raises(ValueError, match="--every"):
        cli.select_views_main(["--config", str(cfg), "--cls", "table", "--every", "0"])
    assert "select_views_main" in open(os.path.join(ROOT, "tools", "select_views_3d.py")).read()
