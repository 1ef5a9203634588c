"""3-D instances lifted from a subsampled cloud to the full cloud, the parts that need no GPU: the NumPy statement of
tests/lift_ref.py against an unrestricted brute force and by hand; the config keys; the header, the binding table, the
library's exports and host-side argument checks; the tools' parsers.  Every comparison is for equality."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import lift_ref as lr
from test_spatial_host import header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bff_nn_search", "bff_rows_to_columns", "bff_lift_bits")
V = 0.125


@functools.lru_cache(maxsize=None)
def cloud(lattice):
    pts = lr.three_planes(3000, lattice)
    sample = lr.subsample_ref(pts, V)
    return pts, sample


@pytest.mark.parametrize("radius", [V, 2 * V])
def test_27_cells_equal_brute_force_on_the_lattice(radius):
    pts, sample = cloud(True)
    nn, d2 = lr.nearest_ref(pts[sample], radius, pts)
    bn, bd = lr.brute_ref(pts[sample], radius, pts)
    assert np.array_equal(nn, bn) and np.array_equal(d2, bd)
    assert nn.dtype == np.int32 and d2.dtype == np.float64


@pytest.mark.parametrize("lattice", [False, True])
def test_subsample_and_the_radius(lattice):
    pts, sample = cloud(lattice)
    assert sample.dtype == np.int32 and (np.diff(sample) > 0).all() and 500 < len(sample) <= 3 * 17 * 17
    key = np.floor((pts - pts.min(0)) / V).astype(np.int64) @ np.array([1, 1 << 21, 1 << 42])
    assert np.array_equal(np.sort(np.unique(key, return_index=True)[1]), sample)
    near, d_near = lr.nearest_ref(pts[sample], V, pts)
    far, d_far = lr.nearest_ref(pts[sample], 2 * V, pts)
    for nn, d2 in ((near, d_near), (far, d_far)):                           # a sampled point's nearest source is itself
        assert np.array_equal(nn[sample], np.arange(len(sample))) and (d2[sample] == 0).all()
    assert (far >= 0).all() and np.isfinite(d_far).all()                    # 2 v >= sqrt(3) v: everybody has a source
    assert 0 < (near < 0).sum() < 100                                       # the own cell's representative can be sqrt(3) v away
    assert np.array_equal(np.isinf(d_near), near < 0)
    keep = near >= 0
    assert np.array_equal(near[keep], far[keep]) and np.array_equal(d_near[keep], d_far[keep])


def test_statement_by_hand():
    # cells of 1 m from lo = (0, 0, 0); sources 1 and 2 are equidistant from the first query in different cells,
    # sources 3 and 4 share coordinates
    src = np.array([[0.0, 0.0, 0.0], [1.5, 0.5, 0.5], [0.5, 0.5, 0.5], [3.0, 3.0, 3.0], [3.0, 3.0, 3.0],
                    [np.nan, 0.0, 0.0], [2.0, 0.0, np.inf]])
    qs = np.array([[1.0, 0.5, 0.5], [3.0, 3.0, 3.0], [3.0, 3.0, 4.0], [3.0, 3.0, 4.0 + 2.0 ** -40], [-0.5, 0.0, 0.0],
                   [-1.0, 0.0, 0.0], [-1.5, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf],
                   [1e300, 0.0, 0.0], [-1e300, 0.0, 0.0], [2.0, 0.0, 0.5]])
    nn, d2 = lr.nearest_ref(src, 1.0, qs)
    assert nn.tolist() == [1, 3, 3, -1, 0, 0, -1, -1, -1, -1, -1, -1, 1]
    assert d2[:6].tolist() == [0.25, 0.0, 1.0, np.inf, 0.25, 1.0] and d2[12] == 0.5
    bn, bd = lr.brute_ref(src, 1.0, qs)
    assert np.array_equal(nn, bn) and np.array_equal(d2, bd)
    none, d_none = lr.nearest_ref(np.zeros((0, 3)), 1.0, qs)
    assert (none == -1).all() and np.isinf(d_none).all()
    rows = lr.pack(np.array([[1, 0, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 1, 1]], bool))
    rows[:, 0] |= np.int64(-1) << np.int64(7)                               # garbage in the padding is ignored
    bad = nn.copy()
    bad[4], bad[5] = 7, -2                                                  # out of range: 0, never followed
    out = lr.lift_ref(bad, rows, 7, len(qs))
    assert out.shape == (2, 1) and out.dtype == np.int64
    assert lr.unpack(out, 64).nonzero()[1].tolist() == [1, 2, 0, 12] and (lr.unpack(out, 64)[:, 13:] == 0).all()


def test_config_keys():
    from beyond_fixed_forms_amd import lift
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    keys = ("subsample_voxel", "subsample_npy_dir", "lift_max_dist", "lift_target_npy_dir", "lift_output_dir")
    assert all(k in DEFAULTS and DEFAULTS[k] is None for k in keys)
    cfg = Config.with_defaults(subsample_voxel=0.05)
    assert lift.subsample_voxel(cfg) == 0.05 and lift.lift_max_dist(cfg) == 0.1 and lift.lift_max_dist(cfg) == 2 * 0.05
    assert lift.lift_max_dist(Config.with_defaults(subsample_voxel=0.05, lift_max_dist=0.3)) == 0.3
    assert lift.lift_max_dist({"lift_max_dist": 1}) == 1.0 and lift.subsample_voxel({"subsample_voxel": 2}) == 2.0
    with pytest.raises(ValueError, match="subsample_voxel is not set"):
        lift.subsample_voxel(Config.with_defaults())
    with pytest.raises(ValueError, match="lift_max_dist is not set"):
        lift.lift_max_dist(Config.with_defaults())
    with pytest.raises(ValueError, match="lift_max_dist is not set"):
        lift.lift_max_dist({})
    for bad in (0, 0.0, -0.1, True, float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError, match="subsample_voxel"):
            lift.subsample_voxel(Config(subsample_voxel=bad))
        with pytest.raises(ValueError, match="subsample_voxel"):
            lift.lift_max_dist(Config(subsample_voxel=bad))                 # the default radius comes from it
        with pytest.raises(ValueError, match="lift_max_dist"):
            lift.lift_max_dist(Config(subsample_voxel=0.05, lift_max_dist=bad))
    text = open(os.path.join(ROOT, "configs", "config.yaml")).read()
    for key in keys:
        assert re.search(rf"^# {key}:", text, re.M), key                    # documented, commented out


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 16
    for name in NAMES:
        kinds, names = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
        assert names[-1] == "stream"
    assert header_args(header, "bff_nn_search")[1] == ["src", "keys", "offs", "order", "n_voxels", "n_source", "lo_host", "cell",
                                                      "radius", "queries", "n_queries", "stride", "nn", "d2", "stream"]
    assert header_args(header, "bff_rows_to_columns")[1] == ["rows_in", "n_rows", "nw_in", "n_source", "cols", "stream"]
    assert header_args(header, "bff_lift_bits")[1] == ["cols", "n_source", "n_rows", "nn", "n_target", "rows_out", "stream"]
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bnearest\.hip\b", makefile, re.M)
    assert re.search(r"^_obj/.*nearest\.o.*:.*rows\.h", makefile, re.M)


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU.  A non-null pointer here is never
    followed: every call below returns before its launch."""
    import ctypes

    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION
    N, X = None, 64                                                          # X: some non-null address
    err = lambda: lib.bff_last_error()
    lo = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_lo = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    # (src, keys, offs, order, n_voxels, n_source, lo_host, cell, radius, queries, n_queries, stride, nn, d2, stream)
    fn = lib.bff_nn_search
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, N, 0, 3, N, N, N) == 0                           # no query: no launch
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, N, 7, 3, N, N, N) == -1 and b"null" in err() and b"queries" in err()
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, X, 7, 3, N, N, N) == -1 and b"(nn)" in err()
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, X, 7, 3, X, N, N) == -1 and b"lo_host" in err()
    assert fn(N, N, N, N, 5, 9, lo, 0.5, 0.5, X, 7, 3, X, N, N) == -1 and b"keys" in err()
    assert fn(N, X, N, N, 5, 9, lo, 0.5, 0.5, X, 7, 3, X, N, N) == -1 and b"offs" in err()
    assert fn(N, X, X, X, 5, 9, lo, 0.5, 0.5, X, 7, 3, X, N, N) == -1 and b"src" in err()
    assert fn(X, X, X, N, 5, 9, lo, 0.5, 0.5, X, 7, 3, X, N, N) == -1 and b"order" in err()
    assert fn(X, X, X, X, 5, 9, bad_lo, 0.5, 0.5, X, 7, 3, X, N, N) == -1 and b"finite" in err()
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, N, 7, 2, N, N, N) == -1 and b"stride" in err()
    for cell, radius, word in ((0.0, 0.5, b"cell"), (float("nan"), 0.5, b"cell"), (float("inf"), 0.5, b"cell"), (0.5, 0.0, b"radius"),
                               (0.5, -1.0, b"radius"), (0.5, float("nan"), b"radius"), (0.5, float("inf"), b"radius")):
        assert fn(N, N, N, N, 5, 9, N, cell, radius, N, 7, 3, N, N, N) == -1 and word in err()
    assert fn(N, N, N, N, -1, 9, N, 0.5, 0.5, N, 7, 3, N, N, N) == -1 and fn(N, N, N, N, 5, -1, N, 0.5, 0.5, N, 7, 3, N, N, N) == -1
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, N, -1, 3, N, N, N) == -1
    assert fn(N, N, N, N, 10, 9, N, 0.5, 0.5, N, 7, 3, N, N, N) == -1 and b"n_voxels" in err()   # more cells than points
    assert fn(N, N, N, N, 5, 9, N, 0.5, 0.5, N, 1 << 31, 3, N, N, N) == -2 and b"2^31" in err()
    assert fn(N, N, N, N, 5, 1 << 31, N, 0.5, 0.5, N, 7, 3, N, N, N) == -2
    # (rows_in, n_rows, nw_in, n_source, cols, stream)
    fn = lib.bff_rows_to_columns
    assert fn(N, 0, 4, 200, N, N) == 0 and fn(N, 3, 0, 0, N, N) == 0                          # zero sizes: no launch
    assert fn(N, 3, 4, 200, N, N) == -1 and b"null" in err() and b"rows_in" in err()
    assert fn(X, 3, 4, 200, N, N) == -1 and b"cols" in err()
    assert fn(N, 3, 3, 200, N, N) == -1 and b"nw_in" in err()                                 # 200 points need 4 words
    assert fn(N, -1, 4, 200, N, N) == -1 and fn(N, 3, -1, 200, N, N) == -1 and fn(N, 3, 4, -1, N, N) == -1
    assert fn(N, 65, 1 << 24, 1 << 30, N, N) == -2 and b"2^31" in err()                       # M * ceil(K / 64) = 2^31 words
    assert fn(N, 64, 1 << 24, 1 << 30, N, N) == -1                                            # just below: on to the pointers
    assert fn(N, 1, 1 << 25, 1 << 31, N, N) == -2
    # (cols, n_source, n_rows, nn, n_target, rows_out, stream)
    fn = lib.bff_lift_bits
    assert fn(N, 200, 0, N, 500, N, N) == 0 and fn(N, 200, 3, N, 0, N, N) == 0                # zero sizes: no launch
    assert fn(N, 200, 3, N, 500, N, N) == -1 and b"null" in err() and b"rows_out" in err()
    assert fn(N, 200, 3, N, 500, X, N) == -1 and b"(nn)" in err()
    assert fn(N, 200, 3, X, 500, X, N) == -1 and b"cols" in err()
    assert fn(N, -1, 3, N, 500, N, N) == -1 and fn(N, 200, -1, N, 500, N, N) == -1 and fn(N, 200, 3, N, -1, N, N) == -1
    assert fn(N, 200, 1 << 11, N, 1 << 26, N, N) == -2 and b"2^31" in err()                   # K * ceil(N / 64) = 2^31 words
    assert fn(N, 200, (1 << 11) - 1, N, 1 << 26, N, N) == -1
    assert fn(N, 1 << 30, 65, N, 500, N, N) == -2 and fn(N, 200, 3, N, 1 << 31, N, N) == -2


def test_no_cpu_path_and_input_kinds():
    from types import SimpleNamespace

    from beyond_fixed_forms_amd import lift
    pts = lr.three_planes(50)
    for fn in (lambda p, d: lift.subsample(p, 0.1, d), lambda p, d: lift.nearest_index(p, 0.1, d)):
        with pytest.raises(ValueError, match="no CPU"):
            fn(pts, "cpu")
        with pytest.raises(ValueError, match="no CPU"):
            fn(torch.from_numpy(pts), "cuda")
        with pytest.raises(TypeError):
            fn(pts[:, :2], "cuda")
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            lift.nearest_index(pts, bad)
        with pytest.raises(ValueError, match="voxel"):
            lift.subsample(pts, bad)
    with pytest.raises(ValueError, match="no CPU"):
        lift.lift_rows(torch.zeros(5, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64), 10, 5)
    empty = SimpleNamespace(rows=None, conf=[], final_class=[])
    assert lift.lift_instances(None, empty, 10, 5) is empty                 # nothing to lift: back as it is


def test_tool_parsers_and_missing_keys(tmp_path, capsys):
    from beyond_fixed_forms_amd import cli
    args = cli._subsample_parser().parse_args(["--config", "c.yaml"])
    assert (args.config, args.scene) == ("c.yaml", None)
    assert cli._subsample_parser().parse_args(["--config", "c", "--scene", "a", "--scene", "b"]).scene == ["a", "b"]
    for bad in ([], ["--config", "c", "--cls", "x"], ["--config", "c", "--scene"]):
        with pytest.raises(SystemExit):
            cli._subsample_parser().parse_args(bad)
    args = cli._lift_parser().parse_args(["--config", "c.yaml", "--cls", "office chair"])
    assert (args.config, args.cls, args.stage) == ("c.yaml", "office chair", "final")
    assert cli._lift_parser().parse_args(["--config", "c", "--cls", "x", "--stage", "mask_3d"]).stage == "mask_3d"
    for bad in (["--config", "c"], ["--config", "c", "--cls", "x", "--stage", "stage1"]):
        with pytest.raises(SystemExit):
            cli._lift_parser().parse_args(bad)
    capsys.readouterr()
    cfg = tmp_path / "config.yaml"
    npy = f"scene_npy_dir: {tmp_path}/npy\n"
    for text, key in ((npy + "subsample_voxel: 0.05\n", "subsample_npy_dir"), (npy + f"subsample_npy_dir: {tmp_path}/small\n", "subsample_voxel"),
                      (npy + f"subsample_npy_dir: {tmp_path}/small\nsubsample_voxel: 0\n", "subsample_voxel"),
                      (npy + f"subsample_npy_dir: {tmp_path}/npy\nsubsample_voxel: 0.05\n", "scene_npy_dir itself")):
        (tmp_path / "npy").mkdir(exist_ok=True)
        cfg.write_text(text)
        with pytest.raises(ValueError, match=key):
            cli.subsample_main(["--config", str(cfg)])
    cfg.write_text(f"scene_npy_dir: {tmp_path}/nowhere\nsubsample_npy_dir: {tmp_path}/small\nsubsample_voxel: 0.05\n")
    assert cli.subsample_main(["--config", str(cfg)]) == 1 and "not a directory" in capsys.readouterr().err
    base = npy + f"final_output_dir: {tmp_path}/final\nmask_3d_dir: {tmp_path}/mask_3d\n"
    cfg.write_text(base + f"lift_output_dir: {tmp_path}/lift\nlift_target_npy_dir: {tmp_path}/full\nsubsample_voxel: 0.05\n")
    assert cli.lift_main(["--config", str(cfg), "--cls", "table"]) == 1 and "not a directory" in capsys.readouterr().err
    (tmp_path / "final" / "table").mkdir(parents=True)                      # a bad or missing key: before the first scene
    both = f"lift_output_dir: {tmp_path}/lift\nlift_target_npy_dir: {tmp_path}/full\n"
    for text, key in ((f"lift_target_npy_dir: {tmp_path}/full\nsubsample_voxel: 0.05\n", "lift_output_dir"),
                      (f"lift_output_dir: {tmp_path}/lift\nsubsample_voxel: 0.05\n", "lift_target_npy_dir"),
                      (both, "lift_max_dist"), (both + "lift_max_dist: -1\n", "lift_max_dist"),
                      (both + "subsample_voxel: nan\n", "subsample_voxel")):
        cfg.write_text(base + text)
        with pytest.raises(ValueError, match=key):
            cli.lift_main(["--config", str(cfg), "--cls", "table"])
    for tool, main in (("subsample_cloud.py", "subsample_main"), ("lift_instances_3d.py", "lift_main")):
        assert main in open(os.path.join(ROOT, "tools", tool)).read()
    assert cli._saved_mask_length({"ins": [], "conf": [], "final_class": []}) is None
    assert cli._saved_mask_length({"ins": torch.tensor([[]])}) is None
    assert cli._saved_mask_length({"ins": torch.zeros((2, 70), dtype=torch.bool)}) == 70
    assert cli._saved_mask_length({"ins": [{"length": 90, "counts": []}]}) == 90
