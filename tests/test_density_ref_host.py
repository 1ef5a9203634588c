"""3-D instances clustered by density, the parts that need no GPU: the NumPy statement of tests/density_ref.py against
sklearn.cluster.DBSCAN (where it imports) and by hand; the config keys; the header, the binding table, the library's
exports and host-side argument checks; the tool's parser.  Every comparison is for equality."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import density_cases as dc
import density_ref as dr
from test_spatial_host import header_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bff_dbscan_elements", "bff_dbscan_core", "bff_dbscan_link")


def lattice_cloud(n=1500, seed=2):
    """Blobs and noise snapped to a 1/8 lattice, duplicates removed: with eps = 0.3 every d2 is a multiple of 1/64 and
    |d2 - eps^2| >= 0.00375 (5/64 = 0.078125 and 6/64 = 0.09375 around 0.09)."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [3, 3, 3]], dtype=np.float64)
    pts = centres[rng.integers(0, 4, n - n // 4)] + 0.3 * rng.standard_normal((n - n // 4, 3))
    pts = np.concatenate([pts, rng.random((n // 4, 3)) * 5 - 1])
    return np.unique(np.round(pts * 8) / 8, axis=0)


@pytest.mark.parametrize("name,eps,min_samples", [("lattice", 0.3, 4), ("lattice", 0.3, 8), ("blobs", 0.1, 8), ("blobs", 0.1, 4)])
def test_statement_against_sklearn(name, eps, min_samples):
    cluster = pytest.importorskip("sklearn.cluster")
    pts = lattice_cloud() if name == "lattice" else dr.blobs(3000, seed=1)
    n = len(pts)
    label, core = dr.labels_ref(pts, eps, min_samples, np.ones(n, bool))
    sk = cluster.DBSCAN(eps=eps, min_samples=min_samples, algorithm="brute").fit(pts)
    sk_core = np.zeros(n, bool)
    sk_core[sk.core_sample_indices_] = True
    assert np.array_equal(core, sk_core) and 0 < core.sum() < n                               # the same core set
    assert np.array_equal(label < 0, sk.labels_ < 0) and (label < 0).any()                    # the same noise set
    pairs = set(zip(label[core].tolist(), sk.labels_[core].tolist()))                         # the same partition of the
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) > 1         # core points, up to renaming
    border = np.flatnonzero(~core & (label >= 0))
    assert len(border) > 10
    eps2 = np.float64(eps) * np.float64(eps)
    for p in border.tolist():                                  # a border point's cluster holds a core neighbour of it
        near = (dr.d2_ref(pts[p:p + 1], pts)[0] <= eps2) & core
        assert (label[near] == label[p]).any()
    assert all(label[a] == a and core[a] for a in np.unique(label[label >= 0]).tolist())      # an anchor is a core point
    assert all(a == np.flatnonzero(core & (label == a)).min() for a in np.unique(label[label >= 0]).tolist())


def test_statement_by_hand():
    ones = lambda pts: np.ones(len(pts), bool)
    pts = dc.exact_boundary()
    assert dr.d2_ref(pts[:1], pts)[0].tolist() == [0.0, 0.0625, 0.0625 + 2.0 ** -55]
    label, core = dr.labels_ref(pts, dc.EPS, 2, ones(pts))
    assert label.tolist() == [0, 0, -1] and core.tolist() == [True, True, False]               # d2 == eps^2 is a neighbour
    label, core = dr.labels_ref(pts, dc.EPS, 1, ones(pts))
    assert label.tolist() == [0, 0, 2] and core.all()                                          # min_samples 1: everybody is core
    assert (dr.labels_ref(pts, dc.EPS, 3, ones(pts))[0] == -1).all()                           # above every count: noise only
    for tie in (True, False):
        pts, x, anchor = dc.two_clusters(tie)
        label, core = dr.labels_ref(pts, dc.EPS, 5, ones(pts))
        assert not core[x] and core.sum() == 10 and label[x] == anchor
        assert sorted(set(label.tolist())) == [0, anchor] and (label == anchor).sum() == 6 and (label == 0).sum() == 5
    pts, centre = dc.all_directions()
    label, core = dr.labels_ref(pts, dc.EPS, 27, ones(pts))
    assert np.flatnonzero(core).tolist() == [centre] and label[:27].tolist() == [centre] * 27 and label[27] == -1
    pts = dc.chain(300)
    label, core = dr.labels_ref(pts, dc.EPS, 2, ones(pts))
    assert core.all() and (label == 0).all()
    label, core = dr.labels_ref(pts, dc.EPS, 3, ones(pts))                                     # the two ends: border points
    assert core.sum() == 298 and (label == label[0]).all() and label[0] == np.flatnonzero(core).min()
    # rows are independent; points outside the row, non-finite points and bits >= n are nobody's neighbour
    pts, x, _ = dc.two_clusters(True)
    pts = np.concatenate([pts, [[np.nan, 0.0, 0.0]], [[0.5, np.inf, 0.0]]])
    n = len(pts)
    rows = dc.garbage(dr.pack(np.array([[1] * 11 + [1, 1], [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1], [0] * 13], bool)), n)
    out, parent, count = dr.cluster_ref(pts, dc.EPS, 5, rows, n)
    assert out.shape == (3, 2) and parent.tolist() == [0, 0, 1] and count.tolist() == [6, 5, 6]
    dense = dr.unpack(out, 128)
    assert dense[0].nonzero()[0].tolist() == [4, 5, 6, 7, 8, 10] and dense[1].nonzero()[0].tolist() == [0, 1, 2, 3, 9]
    assert dense[2].nonzero()[0].tolist() == [0, 1, 2, 3, 9, 10]                               # without B, X follows P_A
    out, parent, count = dr.cluster_ref(pts, dc.EPS, 5, rows, n, mode="largest")
    assert parent.tolist() == [0, 1] and count.tolist() == [6, 6]
    out, parent, count = dr.cluster_ref(pts, dc.EPS, 5, rows, n, min_points=6)
    assert parent.tolist() == [0, 1] and count.tolist() == [6, 6]
    assert dr.cluster_ref(pts, dc.EPS, 5, rows, n, min_points=7)[0].shape == (0, 2)
    assert dr.cluster_ref(pts, dc.EPS, 5, rows[:0], n)[0].shape == (0, 2)


def test_config_keys():
    from beyond_fixed_forms_amd import density as dn
    from beyond_fixed_forms_amd.config import DEFAULTS, Config
    assert (DEFAULTS["cluster_eps"], DEFAULTS["cluster_min_samples"], DEFAULTS["cluster_min_points"], DEFAULTS["cluster_mode"],
            DEFAULTS["cluster_output_dir"]) == (None, None, 1, "split", None)
    assert dn.cluster_min_points(Config()) == 1 and dn.cluster_mode(Config()) == "split"
    cfg = Config.with_defaults(cluster_eps=0.1, cluster_min_samples=8, cluster_min_points=10, cluster_mode="largest")
    assert (dn.cluster_eps(cfg), dn.cluster_min_samples(cfg), dn.cluster_min_points(cfg), dn.cluster_mode(cfg)) == \
        (0.1, 8, 10, "largest")
    assert dn.cluster_eps(Config(cluster_eps=1)) == 1.0 and dn.cluster_min_samples({"cluster_min_samples": 3.0}) == 3
    for bad in (None, 0, -0.1, True, float("nan"), float("inf"), "0.1"):
        with pytest.raises(ValueError, match="cluster_eps"):
            dn.cluster_eps(Config(cluster_eps=bad))
    with pytest.raises(ValueError, match="cluster_eps is not set"):
        dn.cluster_eps(Config.with_defaults())
    with pytest.raises(ValueError, match="cluster_min_samples is not set"):
        dn.cluster_min_samples(Config.with_defaults())
    for bad in (0, -1, 1.5, True, float("nan"), "3"):
        with pytest.raises(ValueError, match="cluster_min_samples"):
            dn.cluster_min_samples(Config(cluster_min_samples=bad))
        with pytest.raises(ValueError, match="cluster_min_points"):
            dn.cluster_min_points(Config(cluster_min_points=bad))
    for bad in ("dbscan", True, 1):
        with pytest.raises(ValueError, match="cluster_mode"):
            dn.cluster_mode(Config(cluster_mode=bad))
    text = open(os.path.join(ROOT, "configs", "config.yaml")).read()
    for key in ("cluster_eps", "cluster_min_samples", "cluster_min_points", "cluster_mode", "cluster_output_dir"):
        assert re.search(rf"^# {key}:", text, re.M), key                    # documented, commented out


def test_binding_mirrors_the_header():
    from beyond_fixed_forms_amd import _lib
    header = open(os.path.join(ROOT, "include", "bff_hip.h")).read()
    assert int(re.search(r"#define BFF_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 16
    for name in NAMES:
        kinds, names = header_args(header, name)
        assert kinds == _lib.SIGNATURES[name], name
        assert names[-1] == "stream"
    index = ["cloud", "keys", "offs", "order", "n_voxels", "n_source", "lo_host", "cell", "eps"]
    assert header_args(header, "bff_dbscan_elements")[1] == ["rows", "n_rows", "nw", "n_points", "finite", "set", "prefix",
                                                            "row_total", "stream"]
    assert header_args(header, "bff_dbscan_core")[1] == ["set", "n_rows", "n_points", "points", "stride", *index, "min_samples",
                                                        "core", "stream"]
    assert header_args(header, "bff_dbscan_link")[1] == ["set", "core", "prefix", "elem_offs", "n_rows", "n_points", "points",
                                                        "stride", *index, "n_elems", "parent", "stream"]
    makefile = open(os.path.join(ROOT, "beyond_fixed_forms_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bdensity\.hip\b", makefile, re.M)
    assert re.search(r"^_obj/.*density\.o.*:.*rows\.h", makefile, re.M)


def test_library_exports_and_checks_arguments():
    """The argument checks run on the host, before any launch: they need no GPU.  A non-null pointer here is never
    followed: every call below returns before its launch."""
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_abi_version() == _lib.ABI_VERSION == 16
    N, X = None, 64                                                          # X: some non-null address
    err = lambda: lib.bff_last_error()
    lo = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_lo = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    # (rows, n_rows, nw, n_points, finite, set, prefix, row_total, stream)
    fn = lib.bff_dbscan_elements
    assert fn(N, 0, 4, 200, N, N, N, N, N) == 0 and fn(N, 3, 0, 0, N, N, N, N, N) == 0        # zero sizes: no launch
    assert fn(N, 3, 4, 200, N, N, N, N, N) == -1 and b"null" in err() and b"rows" in err()
    assert fn(X, 3, 4, 200, X, N, N, N, N) == -1 and b"null" in err() and b"set" in err()
    assert fn(N, 3, 3, 200, N, N, N, N, N) == -1 and b"nw" in err()                           # 200 points need 4 words
    assert fn(N, -1, 4, 200, N, N, N, N, N) == -1 and fn(N, 3, -1, 200, N, N, N, N, N) == -1 and fn(N, 3, 4, -1, N, N, N, N, N) == -1
    assert fn(N, 1 << 12, 1 << 13, 1 << 19, N, N, N, N, N) == -2 and b"2^31" in err()         # K * N = 2^31 bits
    assert fn(N, (1 << 12) - 1, 1 << 13, 1 << 19, N, N, N, N, N) == -1                        # just below: on to the pointers
    assert fn(N, 1, 1 << 25, 1 << 31, N, N, N, N, N) == -2
    # (set, n_rows, n_points, points, stride, cloud, keys, offs, order, n_voxels, n_source, lo_host, cell, eps, min_samples, core, stream)
    fn = lib.bff_dbscan_core
    assert fn(N, 0, 200, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == 0                   # zero sizes: no launch
    assert fn(N, 3, 0, N, 3, N, N, N, N, 0, 0, N, 0.5, 0.5, 4, N, N) == 0
    assert fn(N, 3, 200, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == -1 and b"null" in err() and b"core" in err()
    assert fn(N, 3, 200, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, X, N) == -1 and b"null" in err() and b"set" in err()
    assert fn(X, 3, 200, X, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, X, N) == -1 and b"null" in err() and b"cloud" in err()
    assert fn(X, 3, 200, X, 3, X, X, X, X, 5, 9, bad_lo, 0.5, 0.5, 4, X, N) == -1 and b"finite" in err()   # all before the clear
    assert fn(N, 3, 200, N, 2, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == -1 and b"stride" in err()
    assert fn(N, 3, 200, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 0, N, N) == -1 and b"min_samples" in err()
    for cell, eps, word in ((0.5, 0.0, b"eps"), (0.5, -1.0, b"eps"), (0.5, float("nan"), b"eps"), (0.5, float("inf"), b"eps"),
                            (0.25, 0.5, b"cell"), (float("nan"), 0.5, b"cell"), (float("inf"), 0.5, b"cell")):
        assert fn(N, 3, 200, N, 3, N, N, N, N, 5, 9, N, cell, eps, 4, N, N) == -1 and word in err()
    assert fn(N, 3, 200, N, 3, N, N, N, N, 10, 9, N, 0.5, 0.5, 4, N, N) == -1 and b"n_voxels" in err()   # more cells than points
    assert fn(N, 3, 200, N, 3, N, N, N, N, 5, 201, N, 0.5, 0.5, 4, N, N) == -1                # more finite points than points
    assert fn(N, -1, 200, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == -1 and fn(N, 3, -1, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == -1
    assert fn(N, 1 << 12, 1 << 19, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == -2 and b"2^31" in err()
    assert fn(N, 1, 1 << 31, N, 3, N, N, N, N, 5, 9, N, 0.5, 0.5, 4, N, N) == -2
    # (set, core, prefix, elem_offs, n_rows, n_points, points, stride, cloud, keys, offs, order, n_voxels, n_source, lo_host,
    #  cell, eps, n_elems, parent, stream)
    fn = lib.bff_dbscan_link
    tail = lambda n_elems, parent: (5, 9, lo, 0.5, 0.5, n_elems, parent, N)
    assert fn(N, N, N, N, 0, 200, N, 3, N, N, N, N, *tail(7, N)) == 0 and fn(N, N, N, N, 3, 200, N, 3, N, N, N, N, *tail(0, N)) == 0
    assert fn(N, N, N, N, 3, 200, N, 3, N, N, N, N, 0, 0, N, 0.5, 0.5, 7, N, N) == 0          # no finite point: no element
    assert fn(N, N, N, N, 3, 200, N, 3, N, N, N, N, *tail(7, N)) == -1 and b"null" in err() and b"parent" in err()
    assert fn(N, N, N, N, 3, 200, N, 3, N, N, N, N, *tail(7, X)) == -1 and b"null" in err() and b"set" in err()
    assert fn(X, X, X, X, 3, 200, X, 3, N, N, N, N, *tail(7, X)) == -1 and b"null" in err() and b"cloud" in err()
    assert fn(X, X, X, X, 3, 200, X, 3, X, X, X, X, 5, 9, bad_lo, 0.5, 0.5, 7, X, N) == -1 and b"finite" in err()
    assert fn(N, N, N, N, 3, 200, N, 3, N, N, N, N, *tail(-1, N)) == -1 and fn(N, N, N, N, 3, 200, N, 2, N, N, N, N, *tail(7, N)) == -1
    assert fn(N, N, N, N, 3, 200, N, 3, N, N, N, N, 5, 9, lo, 0.5, 0.0, 7, N, N) == -1 and b"eps" in err()
    assert fn(N, N, N, N, 1 << 12, 1 << 19, N, 3, N, N, N, N, *tail(7, N)) == -2 and b"2^31" in err()


def test_no_cpu_path_and_input_kinds():
    from types import SimpleNamespace

    from beyond_fixed_forms_amd import density as dn
    pts = dr.blobs(50)
    with pytest.raises(ValueError, match="no CPU"):
        dn.density_index(pts, 0.1, "cpu")
    with pytest.raises(ValueError, match="no CPU"):
        dn.density_index(torch.from_numpy(pts), 0.1)
    with pytest.raises(TypeError):
        dn.density_index(pts[:, :2], 0.1)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            dn.density_index(pts, bad)
    index = dn.DensityIndex(0.1, 200, None, None, None, None)
    with pytest.raises(ValueError, match="no CPU"):
        dn.cluster_rows(index, torch.zeros((2, 4), dtype=torch.int64), 200, 4)
    empty = SimpleNamespace(rows=None, conf=[], final_class=[])
    assert dn.cluster_instances(index, empty, {}) is empty                  # nothing to cluster: back as it is


def test_tool_parser_and_missing_keys(tmp_path, capsys):
    from beyond_fixed_forms_amd import cli
    args = cli._cluster_parser().parse_args(["--config", "c.yaml", "--cls", "office chair"])
    assert (args.config, args.cls, args.stage) == ("c.yaml", "office chair", "final")
    assert cli._cluster_parser().parse_args(["--config", "c", "--cls", "x", "--stage", "mask_3d"]).stage == "mask_3d"
    for bad in (["--config", "c"], ["--config", "c", "--cls", "x", "--stage", "stage1"]):
        with pytest.raises(SystemExit):
            cli._cluster_parser().parse_args(bad)
    cfg = tmp_path / "config.yaml"
    base = f"final_output_dir: {tmp_path}/final\nmask_3d_dir: {tmp_path}/mask_3d\n"
    cfg.write_text(base + f"cluster_output_dir: {tmp_path}/cluster\ncluster_eps: 0.1\ncluster_min_samples: 8\n")
    assert cli.cluster_main(["--config", str(cfg), "--cls", "table"]) == 1
    assert "not a directory" in capsys.readouterr().err
    (tmp_path / "final" / "table").mkdir(parents=True)                      # a bad or missing key: before the first scene
    out = f"cluster_output_dir: {tmp_path}/cluster\n"
    for text, key in (("cluster_eps: 0.1\ncluster_min_samples: 8\n", "cluster_output_dir"), (out + "cluster_min_samples: 8\n", "cluster_eps"),
                      (out + "cluster_eps: 0.1\n", "cluster_min_samples"), (out + "cluster_eps: 0\ncluster_min_samples: 8\n", "cluster_eps"),
                      (out + "cluster_eps: 0.1\ncluster_min_samples: 0\n", "cluster_min_samples"),
                      (out + "cluster_eps: 0.1\ncluster_min_samples: 8\ncluster_min_points: 1.5\n", "cluster_min_points"),
                      (out + "cluster_eps: 0.1\ncluster_min_samples: 8\ncluster_mode: dbscan\n", "cluster_mode")):
        cfg.write_text(base + text)
        with pytest.raises(ValueError, match=key):
            cli.cluster_main(["--config", str(cfg), "--cls", "table"])
    assert "cluster_main" in open(os.path.join(ROOT, "tools", "cluster_instances_3d.py")).read()
