"""3-D instances snapped to superpoints, the parts that need no GPU: the NumPy statement of tests/superpoints_ref.py
against a hand-made case; the `need` table; the config keys; the header, the binding table, the library's exports and
host-side argument checks; the tool's parser.  Every comparison is for equality."""
import os
import re

import numpy as np
import pytest
import torch

import superpoints_ref as pr
from test_spatial_host import header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bff_spp_count", "bff_spp_owner", "bff_spp_fill")

# 12 points: superpoint 3 = {4, 5, 6}, 7 = {0, 1, 2, 3, 11}, 50 = {8, 9}; points 7 and 10 are free
HAND_SPP = np.array([7, 7, 7, 7, 3, 3, 3, -1, 50, 50, -5, 7], dtype=np.int64)
HAND_ROWS = [{0, 1, 2, 4, 7}, {1, 2, 3, 11, 5, 6, 8}, {9, 10, 4}]


def hand_rows():
    dense = np.zeros((3, 12), bool)
    for k, pts in enumerate(HAND_ROWS):
        dense[k, sorted(pts)] = True
    return pr.pack(dense)


def as_sets(rows, n=12):
    return [set(np.flatnonzero(r).tolist()) for r in pr.unpack(rows, n)]


def test_index_by_hand():
    ix = pr.index_ref(HAND_SPP)
    assert ix["ids"].tolist() == [3, 7, 50] and ix["seg"].tolist() == [1, 1, 1, 1, 0, 0, 0, -1, 2, 2, -1, 1]
    assert ix["size"].tolist() == [3, 5, 2] and ix["offs"].tolist() == [0, 3, 8, 10]
    assert ix["order"].tolist() == [4, 5, 6, 0, 1, 2, 3, 11, 8, 9]         # ascending point index within a superpoint
    assert np.flatnonzero(ix["free"]).tolist() == [7, 10]
    big = pr.index_ref(np.array([1 << 62, -1, 5, 1 << 62], dtype=np.int64))  # ids are values, not indices
    assert big["ids"].tolist() == [5, 1 << 62] and big["seg"].tolist() == [1, -1, 0, 1]
    none = pr.index_ref(np.array([-1, -2], dtype=np.int32))
    assert len(none["ids"]) == 0 and none["offs"].tolist() == [0] and none["free"].all()


def test_statement_by_hand():
    rows = hand_rows()
    ix = pr.index_ref(HAND_SPP)
    count = pr.count_ref(ix["seg"], 3, pr.unpack(rows, 12))
    assert count.tolist() == [[1, 3, 0], [2, 4, 1], [1, 0, 1]]
    need = pr.need_ref(ix["size"], 0.5)
    assert need.tolist() == [2, 3, 1]
    assert pr.owner_ref(count, need).tolist() == [1, 1, 1]                  # superpoint 50: rows 1 and 2 tie at 1 -> row 1
    out, parent, points = pr.snap_ref(HAND_SPP, rows, 12, 0.5, "snap")
    assert as_sets(out) == [{0, 1, 2, 3, 11, 7}, {0, 1, 2, 3, 11, 4, 5, 6, 8, 9}, {8, 9, 10}]
    assert parent.tolist() == [0, 1, 2] and points.tolist() == [6, 10, 3] and out.dtype == np.int64 and out.shape == (3, 1)
    out, parent, points = pr.snap_ref(HAND_SPP, rows, 12, 0.5, "exclusive")
    assert as_sets(out) == [{7}, {0, 1, 2, 3, 11, 4, 5, 6, 8, 9}, {10}] and points.tolist() == [1, 10, 1]
    out, parent, points = pr.snap_ref(HAND_SPP, rows, 12, 0.5, "exclusive", min_points=2)
    assert as_sets(out) == [{0, 1, 2, 3, 11, 4, 5, 6, 8, 9}] and parent.tolist() == [1] and points.tolist() == [10]
    out, parent, _ = pr.snap_ref(HAND_SPP, rows, 12, 0.5, "snap", min_points=11)
    assert out.shape == (0, 1) and len(parent) == 0
    # ratio 1.0: only a superpoint held whole stays; 1e-9: any hit takes it
    whole = pr.snap_ref(HAND_SPP, rows, 12, 1.0)                            # row 1 holds no superpoint whole: empty, dropped
    assert as_sets(whole[0]) == [{7}, {10}] and whole[1].tolist() == [0, 2]
    assert as_sets(pr.snap_ref(HAND_SPP, rows, 12, 1e-9)[0]) == [{0, 1, 2, 3, 11, 4, 5, 6, 7}, set(range(12)) - {7, 10},
                                                                 {4, 5, 6, 8, 9, 10}]
    garbage = rows.copy()
    garbage[:, 0] |= np.int64(-1) << np.int64(12)                           # bits at positions >= N are ignored, zero in the output
    for mode in ("snap", "exclusive"):
        assert np.array_equal(pr.snap_ref(HAND_SPP, garbage, 12, 0.5, mode)[0], pr.snap_ref(HAND_SPP, rows, 12, 0.5, mode)[0])


def test_need_table():
    from beyond_fixed_forms_amd import superpoints as spp
    table = [(0.55, 100, 56), (0.35, 180, 63), (0.5, 3, 2), (1e-9, 500, 1), (1.0, 7, 7)]
    for ratio, size, want in table:
        assert pr.need_ref([size], ratio).tolist() == [want], (ratio, size)
        got = spp.need_points(np.array([size]), ratio)
        assert got.tolist() == [want] and got.dtype == np.int32
    assert 0.55 * 100 > 55.0                                                # why 56: the product is taken in float64


@pytest.mark.parametrize("mode", ["snap", "exclusive"])
def test_statement_is_idempotent(mode):
    rng = np.random.default_rng(21)
    n = 500
    spp = rng.integers(-2, 40, n) * 1000003
    dense = rng.random((6, n)) < np.array([0.0, 0.05, 0.3, 0.5, 0.7, 1.0])[:, None]
    for ratio in (0.3, 0.5, 1.0):
        once = pr.snap_ref(spp, pr.pack(dense), n, ratio, mode)
        twice = pr.snap_ref(spp, once[0], n, ratio, mode)
        assert np.array_equal(once[0], twice[0]) and np.array_equal(once[2], twice[2])
        assert twice[1].tolist() == list(range(len(once[1])))
        if mode == "exclusive":                                             # no superpoint point in two rows
            got = pr.unpack(once[0], n)
            assert (got[:, spp >= 0].sum(0) <= 1).all()


def test_config_keys():
    from beyond_fixed_forms_amd import superpoints as spp
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    assert (DEFAULTS["superpoint_dir"], DEFAULTS["snap_ratio"], DEFAULTS["snap_mode"], DEFAULTS["snap_min_points"],
            DEFAULTS["snap_output_dir"]) == (None, 0.5, "snap", 1, None)
    assert (spp.snap_ratio(Config()), spp.snap_mode(Config()), spp.snap_min_points(Config())) == (0.5, "snap", 1)
    assert (spp.snap_ratio({}), spp.snap_mode({}), spp.snap_min_points({})) == (0.5, "snap", 1)
    cfg = Config.with_defaults(snap_ratio=0.35, snap_mode="exclusive", snap_min_points=20)
    assert (spp.snap_ratio(cfg), spp.snap_mode(cfg), spp.snap_min_points(cfg)) == (0.35, "exclusive", 20)
    assert spp.snap_ratio(Config(snap_ratio=1)) == 1.0
    for bad in (0, 0.0, -0.1, 1.0000001, 2, True, float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError, match="snap_ratio"):
            spp.snap_ratio(Config(snap_ratio=bad))
    for bad in (0, -1, 1.5, True, float("nan"), "3"):
        with pytest.raises(ValueError, match="snap_min_points"):
            spp.snap_min_points(Config(snap_min_points=bad))
    for bad in ("split", True, 1):
        with pytest.raises(ValueError, match="snap_mode"):
            spp.snap_mode(Config(snap_mode=bad))
    text = open(os.path.join(ROOT, "configs", "config.yaml")).read()
    for key in ("superpoint_dir", "snap_ratio", "snap_mode", "snap_min_points", "snap_output_dir"):
        assert re.search(rf"^# {key}:", text, re.M), key                    # documented, commented out


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 16
    for name in NAMES:
        kinds, names = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
        assert names[-1] == "stream"
    assert header_args(header, "bff_spp_count")[1] == ["rows", "n_rows", "nw", "n_points", "seg", "n_segments", "count", "stream"]
    assert header_args(header, "bff_spp_owner")[1] == ["count", "n_rows", "n_segments", "need", "owner", "stream"]
    assert header_args(header, "bff_spp_fill")[1] == ["count", "n_rows", "n_segments", "need", "owner", "order", "offs", "out",
                                                     "nw", "stream"]
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bsuperpoints\.hip\b", makefile, re.M)
    assert re.search(r"^_obj/.*superpoints\.o.*:.*rows\.h", makefile, re.M)


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU.  A non-null pointer here is never
    followed: every call below returns before its launch."""
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION
    N, X = None, 64                                                          # X: some non-null address
    err = lambda: lib.bff_last_error()
    # (rows, n_rows, nw, n_points, seg, n_segments, count, stream)
    fn = lib.bff_spp_count
    assert fn(N, 0, 4, 200, N, 50, N, N) == 0 and fn(N, 3, 4, 200, N, 0, N, N) == 0          # zero sizes: no launch
    assert fn(N, 3, 4, 200, N, 50, N, N) == -1 and b"null" in err() and b"count" in err()
    assert fn(N, 3, 4, 200, X, 50, X, N) == -1 and b"rows" in err()
    assert fn(X, 3, 4, 200, N, 50, X, N) == -1 and b"seg" in err()
    assert fn(N, -1, 4, 200, N, 50, N, N) == -1 and b"n_rows" in err()
    assert fn(N, 3, -1, 200, N, 50, N, N) == -1 and fn(N, 3, 4, -1, N, 50, N, N) == -1 and fn(N, 3, 4, 200, N, -1, N, N) == -1
    assert fn(N, 3, 3, 200, N, 50, N, N) == -1 and b"nw" in err()                            # 200 points need 4 words
    assert fn(N, 1 << 11, 4, 200, N, 1 << 20, N, N) == -2 and b"2^31" in err()                # K * S = 2^31
    assert fn(N, (1 << 11) - 1, 4, 200, N, 1 << 20, N, N) == -1                               # just below: on to the pointers
    assert fn(N, 1, 1 << 26, 1 << 31, N, 5, N, N) == -2 and fn(N, 1, 4, 200, N, 1 << 31, N, N) == -2
    # (count, n_rows, n_segments, need, owner, stream)
    fn = lib.bff_spp_owner
    assert fn(N, 3, 0, N, N, N) == 0
    assert fn(N, 3, 50, N, N, N) == -1 and b"owner" in err()
    assert fn(N, 3, 50, X, X, N) == -1 and b"count" in err()
    assert fn(X, 3, 50, N, X, N) == -1 and b"need" in err()
    assert fn(N, -1, 50, N, N, N) == -1 and fn(N, 3, -1, N, N, N) == -1
    assert fn(N, 1 << 11, 1 << 20, N, N, N) == -2 and b"2^31" in err()
    # (count, n_rows, n_segments, need, owner /* NULL = snap */, order, offs, out, nw, stream)
    fn = lib.bff_spp_fill
    assert fn(N, 0, 50, N, N, N, N, N, 4, N) == 0 and fn(N, 3, 0, N, N, N, N, N, 4, N) == 0 and fn(N, 3, 50, N, N, N, N, N, 0, N) == 0
    assert fn(N, 3, 50, N, N, N, N, N, 4, N) == -1 and b"out" in err()
    assert fn(N, 3, 50, X, N, X, X, X, 4, N) == -1 and b"need" in err()                       # snap: count and need
    assert fn(X, 3, 50, N, N, X, X, X, 4, N) == -1
    assert fn(N, 3, 50, N, X, N, X, X, 4, N) == -1 and b"order" in err()                      # exclusive: owner is enough
    assert fn(N, 3, 50, N, X, X, N, X, 4, N) == -1 and b"offs" in err()
    assert fn(N, -1, 50, N, N, N, N, N, 4, N) == -1 and fn(N, 3, -1, N, N, N, N, N, 4, N) == -1
    assert fn(N, 3, 50, N, N, N, N, N, -1, N) == -1 and b"nw" in err()
    assert fn(N, 1 << 11, 1 << 20, N, N, N, N, N, 4, N) == -2 and b"2^31" in err()


def test_no_cpu_path_and_input_kinds():
    from types import SimpleNamespace

    from beyond_fixed_forms_amd import superpoints as spp
    with pytest.raises(ValueError, match="no CPU"):
        spp.superpoint_index(HAND_SPP, device="cpu")
    with pytest.raises(ValueError, match="no CPU"):
        spp.superpoint_index(torch.from_numpy(HAND_SPP), device="cpu")
    for floats in (HAND_SPP.astype(np.float32), torch.from_numpy(HAND_SPP).double(), HAND_SPP > 0):
        with pytest.raises(TypeError, match="integer"):
            spp.superpoint_index(floats)
    index = spp.SuperpointIndex(200, 0, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="no CPU"):
        spp.snap_rows(index, torch.zeros((2, 4), dtype=torch.int64), 200)
    empty = SimpleNamespace(rows=None, conf=[], final_class=[])
    assert spp.snap_instances(index, empty, {}) is empty                    # nothing to snap: back as it is
    with pytest.raises(ValueError, match="no CPU"):
        spp.superpoints_from_grid(SimpleNamespace(vox=torch.zeros(5, dtype=torch.int32)))


def test_tool_parser_and_missing_directory(tmp_path, capsys):
    from beyond_fixed_forms_amd import cli
    args = cli._snap_parser().parse_args(["--config", "c.yaml", "--cls", "office chair"])
    assert (args.config, args.cls, args.stage) == ("c.yaml", "office chair", "final")
    assert cli._snap_parser().parse_args(["--config", "c", "--cls", "x", "--stage", "mask_3d"]).stage == "mask_3d"
    with pytest.raises(SystemExit):
        cli._snap_parser().parse_args(["--config", "c", "--cls", "x", "--stage", "stage1"])
    cfg = tmp_path / "config.yaml"
    base = f"final_output_dir: {tmp_path}/final\nmask_3d_dir: {tmp_path}/mask_3d\n"
    cfg.write_text(base + f"snap_output_dir: {tmp_path}/snap\nsuperpoint_dir: {tmp_path}/spp\n")
    assert cli.snap_main(["--config", str(cfg), "--cls", "table"]) == 1
    assert "not a directory" in capsys.readouterr().err
    (tmp_path / "final" / "table").mkdir(parents=True)                      # a bad or missing key: before the first scene
    for text, key in ((f"superpoint_dir: {tmp_path}/spp\n", "snap_output_dir"), (f"snap_output_dir: {tmp_path}/snap\n", "superpoint_dir"),
                      (f"snap_output_dir: {tmp_path}/snap\nsuperpoint_dir: {tmp_path}/spp\nsnap_ratio: 1.5\n", "snap_ratio"),
                      (f"snap_output_dir: {tmp_path}/snap\nsuperpoint_dir: {tmp_path}/spp\nsnap_mode: both\n", "snap_mode"),
                      (f"snap_output_dir: {tmp_path}/snap\nsuperpoint_dir: {tmp_path}/spp\nsnap_min_points: 0\n", "snap_min_points")):
        cfg.write_text(base + text)
        with pytest.raises(ValueError, match=key):
            cli.snap_main(["--config", str(cfg), "--cls", "table"])
    tool = open(os.path.join(ROOT, "tools", "snap_instances_3d.py")).read()
    assert "snap_main" in tool
