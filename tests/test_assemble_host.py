"""A scene's prediction assembled from all query classes, the parts that need no GPU: the NumPy statement of
tests/assemble_ref.py against the greedy loop the reference left at tools/refinement_single.py:71-86 (restated in torch,
with a stable sort); the config keys; the header, the binding table, the library's exports and host-side argument
checks; the tool's parser.  Every comparison is for equality."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import assemble_ref as ar
from test_spatial_host import header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bff_nms_pairs", "bff_nms_greedy")


def reference_loop(ins, conf, nms_thres):
    """The reference's loop on dense bool rows: sort by confidence (stable, so that ties have an order), take the best,
    keep the rest whose IoU with it is below the threshold -- torch's int / int division and its float32 comparison.
    -> the input indices of the kept rows, in the order they were taken."""
    idx = torch.argsort(conf, descending=True, stable=True)
    ins = ins[idx]
    keep = []
    while len(ins) > 0:
        keep.append(int(idx[0]))
        iou = (ins[0] & ins[1:]).sum(dim=-1) / (ins[0] | ins[1:]).sum(dim=-1)
        assert iou.dtype == torch.float32
        ins, idx = ins[1:][iou < nms_thres], idx[1:][iou < nms_thres]
    return keep


def random_rows(rng, k, n):
    """Non-empty rows from a few bases with flips, so that every IoU range occurs; exact duplicates among them."""
    bases = rng.random((max(1, k // 4), n)) < rng.uniform(0.1, 0.6)
    rows = bases[rng.integers(0, len(bases), k)] ^ (rng.random((k, n)) < rng.choice([0.0, 0.02, 0.1, 0.3], size=(k, 1)))
    rows[:, 0] |= ~rows.any(axis=1)
    return rows


@pytest.mark.parametrize("thres", [0.1, 0.3, 0.5, 0.7, 1.0])
def test_statement_equals_the_reference_loop(thres):
    rng = np.random.default_rng(int(thres * 10))
    seen_removed = seen_tie = 0
    for _ in range(60):
        k, n = int(rng.integers(1, 41)), int(rng.integers(1, 201))
        rows = random_rows(rng, k, n)
        score = rng.integers(0, 6, k) / 8.0 if rng.random() < 0.7 else rng.random(k)      # tied scores
        kept, removed_by = ar.nms(rows, score, np.zeros(k, np.int32), thres)
        assert kept.tolist() == reference_loop(torch.from_numpy(rows), torch.from_numpy(score), thres)
        gone = np.flatnonzero(removed_by >= 0)
        assert sorted(kept.tolist() + gone.tolist()) == list(range(k)) and set(removed_by[gone].tolist()) <= set(kept.tolist())
        seen_removed += len(gone)
        seen_tie += len(set(score.tolist())) < k
    assert seen_tie > 20 and (seen_removed > 50 or thres == 1.0)


def boundary_pair(inter, union):
    """Two rows with |a & b| = inter and |a | b| = union."""
    a, b = np.zeros(union, bool), np.zeros(union, bool)
    a[:inter + (union - inter) // 2] = True
    b[:inter] = True
    b[inter + (union - inter) // 2:] = True
    assert (a & b).sum() == inter and (a | b).sum() == union
    return np.stack([a, b])


def test_the_boundary_pair_is_suppressed_in_float32():
    rows = boundary_pair(7, 10)
    score, cls = np.array([0.9, 0.8]), np.zeros(2, np.int32)
    v = np.float32(7) / np.float32(10)
    assert float(v) < 0.7 and not v < np.float32(0.7)                                 # a float64 comparison keeps it
    kept, removed_by = ar.nms(rows, score, cls, 0.7)
    assert kept.tolist() == [0] == reference_loop(torch.from_numpy(rows), torch.from_numpy(score), 0.7)
    assert removed_by.tolist() == [-1, 0]
    rows = boundary_pair(3, 10)                                                       # float32(3 / 10) > float32(0.3): either way
    assert ar.nms(rows, score, cls, 0.3)[0].tolist() == [0] == reference_loop(torch.from_numpy(rows), torch.from_numpy(score), 0.3)


def test_statement_by_hand():
    n = 12
    rows = np.zeros((6, n), bool)
    rows[0, 0:6] = True            # A
    rows[1, 0:5] = True            # inside A: IoU 5/6, containment 1
    rows[2, 4:8] = True            # IoU with A 2/8, with row 1 1/8
    rows[3, 8:12] = True           # apart
    rows[5, 0:6] = True            # A again, lower score; row 4 is empty
    score = np.array([0.9, 0.8, 0.7, 0.7, 1.0, 0.1])
    cls = np.array([0, 1, 0, 1, 0, 1], np.int32)
    assert ar.rank(score).tolist() == [4, 0, 1, 2, 3, 5]
    kept, by = ar.nms(rows, score, cls, 0.5)
    assert kept.tolist() == [0, 2, 3] and by.tolist() == [-1, 0, -1, -1, -2, 0]
    kept, by = ar.nms(rows, score, cls, 0.5, scope="class")                           # rows 1 and 5 are of another class than A
    assert kept.tolist() == [0, 1, 2, 3] and by.tolist() == [-1, -1, -1, -1, -2, 1]
    assert ar.nms(rows, score, cls, 0.25)[0].tolist() == [0, 3]                       # 2/8 is not < 0.25
    assert ar.nms(rows, score, cls, 0.5, criterion="containment")[0].tolist() == [0, 3]   # row 2: 2 of its 4 points in A
    for off in (None, 0, 0.0):
        assert ar.nms(rows, score, cls, off)[0].tolist() == [0, 1, 2, 3, 5]
    out, source, points, _ = ar.assemble(rows, score, cls, None, exclusive=True)
    assert source.tolist() == [0, 2, 3] and points.tolist() == [6, 2, 4]             # rows 1 and 5 are left without a point
    assert np.flatnonzero(out[1]).tolist() == [6, 7]
    assert ar.assemble(rows, score, cls, None, exclusive=True, min_points=3)[1].tolist() == [0, 3]
    assert ar.assemble(rows, score, cls, None, min_points=5)[1].tolist() == [0, 1, 5]
    inst, sem = ar.point_labels(out, cls[source])
    assert inst.tolist() == [1] * 6 + [2] * 2 + [3] * 4 and sem.tolist() == [0] * 8 + [1] * 4
    # the chain: q hits r, r hits s, q does not hit s -> s survives
    h = np.zeros((3, 3), bool)
    h[0, 1] = h[1, 2] = True
    keep, by = ar.greedy(h)
    assert keep.tolist() == [True, False, True] and by.tolist() == [-1, 0, -1]
    words = ar.pack_bits(np.triu(np.ones((70, 70), bool), 1))
    assert words.shape == (70, 2) and words[0, 0] == np.uint64(2 ** 64 - 2) and words[69].tolist() == [0, 0]
    assert np.array_equal(ar.unpack_bits(words, 70), np.triu(np.ones((70, 70), bool), 1))
    with pytest.raises(ValueError, match="NaN"):
        ar.nms(rows, np.array([0.9, np.nan, 0.7, 0.7, 1.0, 0.1]), cls, 0.5)


def test_config_keys():
    from beyond_fixed_forms_amd import assemble as am
    from beyond_fixed_forms_amd.config import Config
    cfg = Config.with_defaults()
    assert am.check_config(cfg) == dict(thres=None, criterion="iou", scope="all", exclusive=False, min_points=1)
    assert am.check_config({}) == am.check_config(cfg) and cfg.get("assembled_output_dir") is None
    for off in (0, 0.0, None):
        assert am.assemble_nms_thres({"assemble_nms_thres": off}) is None
    assert am.assemble_nms_thres({"assemble_nms_thres": 0.5}) == 0.5 and am.assemble_nms_thres({"assemble_nms_thres": 1}) == 1.0
    for bad in (-0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="assemble_nms_thres"):
            am.assemble_nms_thres({"assemble_nms_thres": bad})
    assert am.assemble_criterion({"assemble_criterion": "containment"}) == "containment"
    assert am.assemble_scope({"assemble_scope": "class"}) == "class"
    assert am.assemble_exclusive({"assemble_exclusive": True}) is True and am.assemble_min_points({"assemble_min_points": 50}) == 50
    for key, bad in (("assemble_criterion", "giou"), ("assemble_scope", "scene"), ("assemble_exclusive", 1),
                     ("assemble_exclusive", "yes"), ("assemble_min_points", 0), ("assemble_min_points", 1.5)):
        with pytest.raises(ValueError, match=key):
            am.check_config({key: bad})


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 16
    for name in NAMES:
        kinds, names = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
        assert names[-1] == "stream"
    assert header_args(header, "bff_nms_pairs")[1] == ["inter", "area", "order", "cls", "k", "criterion", "thres", "sup", "stream"]
    assert header_args(header, "bff_nms_pairs")[0][6] is _lib._F                      # the threshold is a float
    assert header_args(header, "bff_nms_greedy")[1] == ["sup", "k", "keep_bits", "by", "n_kept", "stream"]
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bnms\.hip\b", makefile, re.M)


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU.  A non-null pointer here is never
    followed: every call below returns before its launch."""
    from beyond_fixed_forms_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)                                                  # the symbols resolve without a GPU
    assert all(hasattr(raw, name) for name in NAMES)
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION == 16
    N, X = None, 64
    err = lambda: lib.bff_last_error()
    limit = lib.bff_resolve_overlaps_max_rows()
    assert limit == 4096
    # (inter, area, order, cls, k, criterion, thres, sup, stream)
    fn = lib.bff_nms_pairs
    assert fn(N, N, N, N, 0, 0, 0.5, N, N) == 0 and fn(N, N, N, N, 0, 1, 0.5, N, N) == 0      # K = 0: no launch
    assert fn(N, N, N, N, -1, 0, 0.5, N, N) == -1
    assert fn(X, X, X, N, 3, 2, 0.5, X, N) == -1 and b"criterion" in err()
    assert fn(X, X, X, N, 3, 0, float("nan"), X, N) == -1 and b"NaN" in err()
    assert fn(X, X, X, N, limit + 1, 0, 0.5, X, N) == -2 and b"4097" in err() and b"4096" in err()
    assert fn(N, X, X, N, 3, 0, 0.5, X, N) == -1 and b"null" in err() and fn(X, X, X, N, 3, 0, 0.5, N, N) == -1
    # (sup, k, keep_bits, by, n_kept, stream)
    fn = lib.bff_nms_greedy
    assert fn(N, 0, N, N, N, N) == 0 and fn(N, -1, N, N, N, N) == -1
    assert fn(X, limit + 1, X, X, X, N) == -2 and b"4097" in err() and b"4096" in err()
    assert fn(N, 3, X, X, X, N) == -1 and b"null" in err() and fn(X, 3, X, X, N, N) == -1


def test_no_cpu_path_and_input_kinds():
    from beyond_fixed_forms_amd import assemble as am
    with pytest.raises(ValueError, match="no CPU"):
        am.nms_rows(torch.zeros((2, 4), dtype=torch.int64), 200, [0.5, 0.5], [0, 0], 0.5)
    with pytest.raises(ValueError, match="no CPU"):
        am.assemble_rows(torch.zeros((2, 4), dtype=torch.int64), 200, [0.5, 0.5], [0, 0])
    with pytest.raises(ValueError, match="no CPU"):
        am.assemble_scene({}, 200, {}, "cpu")
    with pytest.raises(ValueError, match="assemble_scope"):                           # the config is read first
        am.assemble_scene({}, 200, {"assemble_scope": "x"}, "cuda")


def test_tool_parser_and_missing_keys(tmp_path, capsys):
    from beyond_fixed_forms_amd import cli
    p = cli._assemble_parser()
    args = p.parse_args(["--config", "c.yaml", "--cls", "office chair", "--cls", "chair"])
    assert (args.config, args.cls, args.all_classes, args.stage, args.point_labels) == \
        ("c.yaml", ["office chair", "chair"], False, "final", False)
    args = p.parse_args(["--config", "c", "--all-classes", "--stage", "mask_3d", "--point-labels"])
    assert (args.cls, args.all_classes, args.stage, args.point_labels) == (None, True, "mask_3d", True)
    for bad in (["--config", "c"], ["--config", "c", "--cls", "x", "--all-classes"], ["--config", "c", "--cls", "x", "--stage", "s"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    ev = cli._evaluation_parser().parse_args(["--cls", "x", "--label-table", "t.json"])
    assert (ev.assembled, ev.use_conf) == (False, False)
    ev = cli._evaluation_parser().parse_args(["--cls", "x", "--label-table", "t.json", "--assembled", "--use-conf"])
    assert (ev.assembled, ev.use_conf) == (True, True)
    cfg = tmp_path / "config.yaml"
    base = f"final_output_dir: {tmp_path}/final\nmask_3d_dir: {tmp_path}/mask_3d\nscene_npy_dir: {tmp_path}/npy\n"
    out = f"assembled_output_dir: {tmp_path}/assembled\n"
    cfg.write_text(base + out)
    assert cli.assemble_main(["--config", str(cfg), "--all-classes"]) == 1
    assert "not a directory" in capsys.readouterr().err
    (tmp_path / "final" / "table").mkdir(parents=True)
    assert cli.assemble_main(["--config", str(cfg), "--cls", "table", "--cls", "chair"]) == 1
    assert "chair" in capsys.readouterr().err
    for text, key in (("", "assembled_output_dir"), (out + "assemble_nms_thres: 1.5\n", "assemble_nms_thres"),
                      (out + "assemble_criterion: giou\n", "assemble_criterion"), (out + "assemble_scope: scene\n", "assemble_scope"),
                      (out + "assemble_exclusive: 2\n", "assemble_exclusive"), (out + "assemble_min_points: 0\n", "assemble_min_points")):
        cfg.write_text(base + text)
        with pytest.raises(ValueError, match=key):                                    # before the first scene
            cli.assemble_main(["--config", str(cfg), "--all-classes"])
    assert "assemble_main" in open(os.path.join(ROOT, "tools", "assemble_scene_3d.py")).read()
