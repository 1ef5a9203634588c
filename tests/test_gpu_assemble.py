"""A scene's prediction assembled from all query classes, on the GPU: bff_nms_greedy on synthetic hit matrices,
bff_nms_pairs bit by bit, assemble.nms_rows / assemble_rows / assemble_scene / point_labels, the command-line tool and the
evaluator's --assembled, against the NumPy statement (tests/assemble_ref.py).  Everything is compared for equality."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import assemble_ref as ar
from test_assemble_host import boundary_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASE, K_CASE = 1000, 130


@pytest.fixture(scope="module")
def am():
    from beyond_fixed_forms_amd import _lib, assemble
    _lib.load()
    assert torch.cuda.is_available()
    return assemble


def to_dev(a, dtype):
    """uint64 words as the int64 the device tensors hold, anything else converted."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype) if a.dtype == np.uint64 else a.astype(dtype)).to(DEV)


# ------------------------------------------------------------------ bff_nms_greedy
def run_greedy(h):
    """h bool [K][K] by rank, upper triangle -> (keep bool [K], by, n_kept) from the device, the buffers pre-filled."""
    from beyond_fixed_forms_amd import _lib
    k = len(h)
    w = (k + 63) // 64
    sup = to_dev(ar.pack_bits(h), np.int64)
    keep_bits = torch.full((w,), -1, dtype=torch.int64, device=DEV)
    by = torch.full((k,), -7, dtype=torch.int32, device=DEV)
    n_kept = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.call("bff_nms_greedy", _lib._ptr(sup), k, _lib._ptr(keep_bits), _lib._ptr(by), _lib._ptr(n_kept))
    words = keep_bits.cpu().numpy()
    keep = ar.unpack_bits(words.reshape(1, w), k)[0]
    assert np.array_equal(words.view(np.uint64), ar.pack_bits(keep[None, :])[0])              # the bits >= K are zero
    return keep, by.cpu().numpy(), int(n_kept.item())


def check_greedy(h):
    keep, by, n_kept = run_greedy(h)
    exp_keep, exp_by = ar.greedy(h)
    assert np.array_equal(keep, exp_keep) and np.array_equal(by, exp_by) and n_kept == int(exp_keep.sum())
    return exp_keep


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128, 129, 4095, 4096])
def test_greedy_on_synthetic_matrices(am, k):
    rng = np.random.default_rng(k)
    assert check_greedy(np.zeros((k, k), bool)).all()                                          # nothing hits: all kept
    assert check_greedy(np.triu(np.ones((k, k), bool), 1)).sum() == 1                          # the best hits all
    for density in (1.0 / k, 0.5):
        kept = check_greedy(np.triu(rng.random((k, k)) < density, 1))
        assert k < 3 or 0 < kept.sum() < k or density < 0.5


@pytest.mark.parametrize("k", [3, 65, 66, 129, 4095, 4096])
def test_greedy_chains(am, k):
    """q hits r, r hits s, q does not hit s: s survives.  Along consecutive ranks every decision needs the one just before
    it, across the words' ends 63 -> 64 -> 65 and in the last word: a walk that reads `removed` early fails here."""
    chain = np.zeros((k, k), bool)
    chain[np.arange(k - 1), np.arange(1, k)] = True
    assert check_greedy(chain).tolist() == [r % 2 == 0 for r in range(k)]
    chain[0, 1] = False                                                                        # the same chain one rank later
    assert check_greedy(chain).tolist() == [r == 0 or r % 2 == 1 for r in range(k)]
    if k > 66:
        far = np.zeros((k, k), bool)                                                           # a chain of strides 63, 1, 1, 64
        for a, b in ((0, 63), (63, 64), (64, 65), (65, k - 1), (1, k - 1)):
            far[a, b] = True
        kept = check_greedy(far)
        assert not kept[63] and kept[64] and not kept[65] and not kept[k - 1]                  # k - 1: removed by rank 1, not 65


def test_greedy_limit_and_zero(am):
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    sup, keep_bits = (torch.full((n,), -7, dtype=torch.int64, device=DEV) for n in (4097 * 65, 65))
    by, n_kept = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (4097, 1))
    bufs, p = (sup, keep_bits, by, n_kept), _lib._ptr
    assert lib.bff_nms_greedy(p(sup), 4097, p(keep_bits), p(by), p(n_kept), _lib._stream()) == -2
    assert b"4097" in lib.bff_last_error() and b"4096" in lib.bff_last_error()
    assert lib.bff_nms_pairs(p(by), p(by), p(by), None, 4097, 0, 0.5, p(sup), _lib._stream()) == -2
    assert lib.bff_nms_greedy(p(sup), 0, p(keep_bits), p(by), p(n_kept), _lib._stream()) == 0      # K = 0: no launch
    assert lib.bff_nms_pairs(p(by), p(by), p(by), None, 0, 0, 0.5, p(sup), _lib._stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs)                                            # nothing was written


# ------------------------------------------------------------------ the rows of the other tests
@functools.lru_cache(maxsize=None)
def case():
    """K_CASE dense rows over N_CASE points: the boundary pairs 7 / 10 and 3 / 10, rows from a few bases with flips, exact
    duplicates, disjoint rows; scores with ties and three classes."""
    rng = np.random.default_rng(5)
    rows = np.zeros((K_CASE, N_CASE), bool)
    rows[0:2, 0:10] = boundary_pair(7, 10)
    rows[2:4, 10:20] = boundary_pair(3, 10)
    bases = np.zeros((5, N_CASE), bool)
    bases[:, 20:700] = rng.random((5, 680)) < rng.uniform(0.1, 0.4, size=(5, 1))
    n_based = K_CASE - 4 - 20
    flips = np.zeros((n_based, N_CASE), bool)
    flips[:, 20:700] = rng.random((n_based, 680)) < rng.choice([0.0, 0.0, 0.02, 0.1, 0.3], size=(n_based, 1))
    rows[4:4 + n_based] = bases[rng.integers(0, 5, n_based)] ^ flips
    for d in range(20):
        rows[4 + n_based + d, 700 + 15 * d:700 + 15 * d + 15] = True
    rows = rows[np.concatenate([[0, 1, 2, 3], 4 + rng.permutation(K_CASE - 4)])]
    assert rows.any(axis=1).all() and len({r.tobytes() for r in rows}) < K_CASE - 10
    score = rng.integers(0, 5, K_CASE) / 4.0
    score[0:4] = [0.9, 0.8, 0.9, 0.8]
    cls = rng.integers(0, 3, K_CASE).astype(np.int32)
    cls[0:4] = 1
    return rows, score, cls


def garbage_rows(dense, nw, seed=6):
    """int64 [K][nw] bit rows of dense bool [K][N] with random bits at every position >= N."""
    k, n = dense.shape
    junk = np.random.default_rng(seed).random((k, nw * 64)) < 0.5
    junk[:, :n] = dense
    return ar.pack_bits(junk).view(np.int64)


@pytest.mark.parametrize("criterion", ar.CRITERIA)
@pytest.mark.parametrize("scope", ar.SCOPES)
def test_pairs_every_bit(am, criterion, scope):
    from beyond_fixed_forms_amd import _lib
    rows, score, cls = case()
    order = ar.rank(score)
    assert (order != np.arange(K_CASE)).any()
    dev_rows = to_dev(ar.pack_bits(rows), np.int64)
    inter, area = _lib.cross_popcount(dev_rows, dev_rows), _lib.popcount_rows(dev_rows)
    assert np.array_equal(inter.cpu().numpy(), rows.astype(np.int64) @ rows.astype(np.int64).T)
    w = (K_CASE + 63) // 64
    order_dev, cls_dev = to_dev(order, np.int32), to_dev(cls, np.int32)
    for thres in (0.7, 0.3, 0.5, 1.0):
        sup = torch.full((K_CASE, w), -1, dtype=torch.int64, device=DEV)
        _lib.call("bff_nms_pairs", _lib._ptr(inter), _lib._ptr(area), _lib._ptr(order_dev),
                  _lib._ptr(cls_dev) if scope == "class" else None, K_CASE, ar.CRITERIA.index(criterion), float(thres), _lib._ptr(sup))
        h = ar.hits(inter.cpu().numpy(), area.cpu().numpy(), order, cls, thres, criterion, scope)
        assert np.array_equal(sup.cpu().numpy().view(np.uint64), ar.pack_bits(h))              # the zero bits included
        assert 0 < h.sum() < K_CASE * (K_CASE - 1) // 2
        pos = {int(i): r for r, i in enumerate(order)}
        if criterion == "iou" and thres in (0.7, 0.3):                                         # the boundary pairs are hit
            a, b = (0, 1) if thres == 0.7 else (2, 3)
            assert pos[a] < pos[b] and h[pos[a], pos[b]]


# ------------------------------------------------------------------ nms_rows / assemble_rows
def with_empties(rows, score, cls):
    """Three empty rows among the case's: first, in the middle, last."""
    at = [0, 60, len(rows)]
    return np.insert(rows, at, False, axis=0), np.insert(score, at, 2.0), np.insert(cls, at, 0).astype(np.int32)


@pytest.mark.parametrize("thres,criterion,scope", [(0.5, "iou", "all"), (0.7, "iou", "class"), (0.3, "containment", "all"),
                                                     (None, "iou", "all"), (0, "iou", "class")])
def test_rows_against_the_statement(am, thres, criterion, scope):
    rows, score, cls = with_empties(*case())
    k = len(rows)
    nw = (N_CASE + 63) // 64 + 2
    dev_rows = to_dev(garbage_rows(rows, nw), np.int64)
    before = dev_rows.clone()
    for sc in (score, np.full(k, 0.5)):                                                        # ties throughout
        kept, removed_by = am.nms_rows(dev_rows, N_CASE, sc, cls, thres, criterion, scope)
        exp_kept, exp_by = ar.nms(rows, sc, cls, thres, criterion, scope)
        assert kept.dtype == removed_by.dtype == torch.int64 and not kept.is_cuda
        assert np.array_equal(kept.numpy(), exp_kept) and np.array_equal(removed_by.numpy(), exp_by)
        assert (exp_by == -2).sum() == 3 and (not thres or 10 < len(exp_kept) < K_CASE)
        for exclusive in (False, True):
            for min_points in (1, 50):
                out, source, points, by = am.assemble_rows(dev_rows, N_CASE, sc, cls, thres, criterion, scope, exclusive, min_points)
                exp = ar.assemble(rows, sc, cls, thres, criterion, scope, exclusive, min_points)
                assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (len(exp[1]), (N_CASE + 63) // 64)
                assert np.array_equal(out.cpu().numpy().view(np.uint64), ar.pack_bits(exp[0]))   # the padding bits zero
                assert np.array_equal(source.numpy(), exp[1]) and np.array_equal(points.numpy(), exp[2])
                assert np.array_equal(by.numpy(), exp[3]) and 0 < len(exp[1]) and (min_points == 1 or len(exp[1]) < len(exp_kept))
    assert torch.equal(dev_rows, before)                                                       # the input is not edited


def test_rows_input_checks(am):
    rows, score, cls = case()
    dev_rows = to_dev(ar.pack_bits(rows), np.int64)
    bad = score.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        am.nms_rows(dev_rows, N_CASE, bad, cls, 0.5)
    with pytest.raises(ValueError, match="words"):
        am.nms_rows(dev_rows, N_CASE + 64, score, cls, 0.5)
    with pytest.raises(ValueError, match="scores"):
        am.nms_rows(dev_rows, N_CASE, score[:-1], cls, 0.5)
    with pytest.raises(ValueError, match="thres"):
        am.nms_rows(dev_rows, N_CASE, score, cls, 1.5)
    with pytest.raises(ValueError, match="criterion"):
        am.nms_rows(dev_rows, N_CASE, score, cls, 0.5, "giou")
    with pytest.raises(ValueError, match="min_points"):
        am.assemble_rows(dev_rows, N_CASE, score, cls, 0.5, min_points=0)
    many = torch.ones((4097, 1), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="4097.*4096"):
        am.nms_rows(many, 64, np.zeros(4097), np.zeros(4097, np.int32), 0.5)
    none = torch.zeros((0, 16), dtype=torch.int64, device=DEV)
    out, source, points, by = am.assemble_rows(none, N_CASE, [], [], 0.5)
    assert tuple(out.shape) == (0, 16) and len(source) == len(points) == len(by) == 0
    out, source, _, by = am.assemble_rows(torch.zeros((3, 16), dtype=torch.int64, device=DEV), N_CASE, [1, 2, 3], [0, 0, 0], 0.5)
    assert tuple(out.shape) == (0, 16) and len(source) == 0 and by.tolist() == [-2, -2, -2]


# ------------------------------------------------------------------ scenes, labels, the tool
CLASSES = ["chair", "office chair", "table"]


def scene_files(seed, n, rle_class=None, empty_class=None):
    """{class: saved file} of one scene: the case's kind of rows dealt to the three classes (so that duplicates sit in
    several of them), one class as RLE dicts, one in the reference's empty list form; and the dense rows, scores and
    class positions in gathering order."""
    from beyond_fixed_forms_amd.synthetic import _rle_from_dense
    rng = np.random.default_rng(seed)
    bases = rng.random((4, n)) < rng.uniform(0.05, 0.3, size=(4, 1))
    files, dense, score, cls = {}, [], [], []
    for ci, name in enumerate(CLASSES):
        if name == empty_class:
            files[name] = {"ins": [], "conf": [], "final_class": []}
            continue
        k = 5 + ci
        rows = bases[rng.integers(0, 4, k)] ^ (rng.random((k, n)) < rng.choice([0.0, 0.01, 0.2], size=(k, 1)))
        rows[0] = bases[0]                                                     # the same object in every class, bit for bit
        conf = torch.from_numpy(rng.integers(1, 9, k) / 8.0).to(torch.float16)
        ins = torch.from_numpy(rows)
        files[name] = {"ins": _rle_from_dense(ins) if name == rle_class else ins, "conf": conf, "final_class": [name] * k}
        dense.append(rows), score.append(conf.double().numpy()), cls.append(np.full(k, ci, np.int32))
    return files, np.concatenate(dense), np.concatenate(score), np.concatenate(cls)


def expected_scene(dense, score, cls, opts):
    """The statement's rows, (class, row) sources and removed_by pairs of a scene."""
    row = np.concatenate([np.arange((cls == c).sum()) for c in range(len(CLASSES))]) if len(cls) else np.zeros(0, np.int64)
    rows, source, _, removed = ar.assemble(dense, score, cls, opts.get("assemble_nms_thres"), opts.get("assemble_criterion", "iou"),
                                           opts.get("assemble_scope", "all"), opts.get("assemble_exclusive", False),
                                           opts.get("assemble_min_points", 1))
    by = np.stack([removed, removed], axis=1)
    gone = removed >= 0
    by[gone, 0], by[gone, 1] = cls[removed[gone]], row[removed[gone]]
    return rows, np.stack([cls[source].astype(np.int64), row[source]], axis=1), score[source], by


@pytest.mark.parametrize("opts", [dict(assemble_nms_thres=0.5), dict(assemble_nms_thres=0.5, assemble_scope="class", assemble_min_points=40),
                                  dict(assemble_nms_thres=0.6, assemble_criterion="containment", assemble_exclusive=True), dict()])
def test_assemble_scene_and_point_labels(am, opts):
    from beyond_fixed_forms_amd import cli, evaluation, instances3d
    n = 1500 + 13
    files, dense, score, cls = scene_files(21, n, rle_class="office chair")
    results = dict(files)
    results["table"] = cli._saved_instances(files["table"], n, DEV)                             # a namespace with device rows
    got = am.assemble_scene(results, n, opts, DEV)
    rows, source, conf, by = expected_scene(dense, score, cls, opts)
    assert np.array_equal(got.rows.cpu().numpy().view(np.uint64), ar.pack_bits(rows)) and 3 < len(rows)
    assert (len(rows) < len(dense)) == bool(opts)
    assert np.array_equal(torch.stack([got.source_class, got.source_row], 1).numpy(), source)
    assert np.array_equal(got.conf.numpy(), conf) and got.conf.dtype == torch.float64 and got.n_points == n
    assert got.final_class == [CLASSES[c] for c in source[:, 0]] and got.classes == CLASSES
    assert np.array_equal(got.removed_by.numpy(), by)
    instance, semantic = am.point_labels(got)
    exp_instance, exp_semantic = ar.point_labels(rows, source[:, 0])
    assert instance.dtype == torch.uint16 and semantic.dtype == torch.int32 and instance.is_cuda
    assert np.array_equal(instance.cpu().numpy(), exp_instance) and np.array_equal(semantic.cpu().numpy(), exp_semantic)
    assert (exp_instance == 0).any() and 1 < exp_instance.max() <= len(rows)
    # what reads a stage's result reads this one: the saved form through the evaluator's file reader, replace_rows
    saved = cli.assembled_dict(got)
    preds, pred_rows = evaluation.final_file_predictions(saved, "s", CLASSES, n, DEV)
    assert torch.equal(pred_rows, got.rows) and [p["label_id"] for p in preds] == [c + 1.0 for c in source[:, 0]]
    again = instances3d.replace_rows(got, got.rows[:2], torch.tensor([1, 0]))
    assert again.final_class == got.final_class[1::-1] and torch.equal(again.conf, got.conf[[1, 0]])


def tool_tree(tmp_path):
    """Three classes, two scenes and a third whose every file is empty: scene_a with one class as RLE, scene_b with one class
    missing and one in the empty list form."""
    from beyond_fixed_forms_amd.config import Config
    scenes = {"scene_a": scene_files(31, 900, rle_class="chair") + (900,),
              "scene_b": scene_files(32, 1100 + 5, empty_class="office chair") + (1105,),
              "scene_c": ({c: {"ins": [], "conf": [], "final_class": []} for c in CLASSES}, np.zeros((0, 70), bool), np.zeros(0),
                          np.zeros(0, np.int32), 70)}
    (tmp_path / "npy").mkdir()
    for scene_id, (files, _, _, _, n) in scenes.items():
        np.save(tmp_path / "npy" / f"{scene_id}.npy", np.zeros((n, 6), np.float32))
        for name, f in files.items():
            if scene_id == "scene_b" and name == "chair":                      # this class has no file for the scene
                continue
            (tmp_path / "final" / name).mkdir(parents=True, exist_ok=True)
            torch.save(f, tmp_path / "final" / name / f"{scene_id}.pth")
    files, dense, score, cls, n = scenes["scene_b"]                            # without chair: its rows are not gathered
    scenes["scene_b"] = (files, dense[cls != 0], score[cls != 0], cls[cls != 0], n)
    opts = dict(assemble_nms_thres=0.5, assemble_min_points=5)
    cfg = Config.with_defaults(scene_npy_dir=str(tmp_path / "npy"), final_output_dir=str(tmp_path / "final"),
                               mask_3d_dir=str(tmp_path / "m3d"), assembled_output_dir=str(tmp_path / "assembled"), **opts)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    return scenes, opts


@pytest.mark.parametrize("rle", [False, True])
def test_tool_in_a_child_process(am, tmp_path, rle):
    from oracle import rle_ref
    scenes, opts = tool_tree(tmp_path)
    env = dict(os.environ, BFF_SAVE_RLE="1" if rle else "0")
    which = ["--all-classes"] if rle else [x for c in CLASSES for x in ("--cls", c)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "assemble_scene_3d.py"), "--config", str(tmp_path / "config.yaml"),
                        *which, *([] if rle else ["--point-labels"])], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "assembled")) == ["scene_a.pth", "scene_b.pth", "scene_c.pth"]
    for scene_id, (files, dense, score, cls, n) in scenes.items():
        out = torch.load(tmp_path / "assembled" / f"{scene_id}.pth", weights_only=False)
        rows, source, conf, by = expected_scene(dense, score, cls, opts)
        assert out["classes"] == CLASSES and np.array_equal(out["source"].numpy(), source) and np.array_equal(out["removed_by"].numpy(), by)
        if scene_id == "scene_c":
            assert (out["ins"], out["conf"], out["final_class"]) == ([], [], []) and tuple(out["source"].shape) == (0, 2)
        else:
            if rle:
                assert isinstance(out["ins"], list) and all(int(x["length"]) == n for x in out["ins"])
                ins = rle_ref.rle_decode_batch_ref(out["ins"]).bool().numpy()
            else:
                assert out["ins"].dtype == torch.bool and not out["ins"].is_cuda
                ins = out["ins"].numpy()
            assert np.array_equal(ins, rows) and 2 < len(rows) < len(dense)
            assert np.array_equal(out["conf"].numpy(), conf) and out["final_class"] == [CLASSES[c] for c in source[:, 0]]
            results = {c: files[c] for c in CLASSES if not (scene_id == "scene_b" and c == "chair")}
            same = am.assemble_scene(results, n, opts, DEV)                    # the files equal assemble_scene's result
            assert np.array_equal(ar.unpack_bits(same.rows.cpu().numpy(), n), ins) and torch.equal(same.conf, out["conf"])
        assert ("point_instance" in out) == ("point_semantic" in out) == (not rle)
        if not rle:
            instance, semantic = ar.point_labels(rows, source[:, 0])
            assert np.array_equal(out["point_instance"].numpy(), instance) and np.array_equal(out["point_semantic"].numpy(), semantic)


def test_evaluator_reads_assembled_files(am, tmp_path):
    """NMS off, exclusive off: `--assembled --cls X` gives the six values of X's own per-class run, for each class X -- the same
    NaN pattern, the values within 1e-12 (all counts are integers; the margin only covers the summation order of np.dot, the
    k 2^-52 of DESIGN.md section 1)."""
    from beyond_fixed_forms_amd import cli
    from beyond_fixed_forms_amd.config import Config
    from test_gpu_evaluation import CLASS_LABELS, SEMANTIC_IDS, cli_scene
    (tmp_path / "gt").mkdir()
    (tmp_path / "npy").mkdir()
    for k in range(2):
        scene_id = f"scene{80 + k:04d}_00"
        sem, ins, masks, classes = cli_scene(80 + k, 2500 + 11 * k)
        torch.save((np.zeros((len(sem), 3), np.float32), np.zeros((len(sem), 3), np.float32), sem, ins), tmp_path / "gt" / f"{scene_id}.pth")
        np.save(tmp_path / "npy" / f"{scene_id}.npy", np.zeros((len(sem), 3), np.float32))
        for cls in ("chair", "table"):
            own = [i for i, c in enumerate(classes) if c == cls]
            (tmp_path / "final" / cls).mkdir(parents=True, exist_ok=True)
            torch.save({"ins": torch.from_numpy(masks[own]), "conf": torch.linspace(0.2, 0.9, len(own)), "final_class": [cls] * len(own)},
                       tmp_path / "final" / cls / f"{scene_id}.pth")
    cfg = Config.with_defaults(final_output_dir=str(tmp_path / "final"), scene_npy_dir=str(tmp_path / "npy"),
                               assembled_output_dir=str(tmp_path / "assembled"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    (tmp_path / "labels.json").write_text(json.dumps({"class_labels": CLASS_LABELS, "semantic_ids": SEMANTIC_IDS}))
    common = ["--config", str(tmp_path / "config.yaml"), "--gt-dir", str(tmp_path / "gt"), "--label-table", str(tmp_path / "labels.json")]

    def values(cls, *extra):
        results = tmp_path / f"results_{cls}_{len(extra)}" / "overall_results.txt"
        assert cli.evaluation_main(["--cls", cls, "--results-file", str(results), *common, *extra]) == 0
        line = [ln for ln in results.read_text().split("\n") if ln.startswith(f"{cls},")][0]
        return np.array([float(v) for v in line.split(",")[1:7]])

    threads = torch.get_num_threads()
    try:
        assert cli.assemble_main(["--config", str(tmp_path / "config.yaml"), "--cls", "chair", "--cls", "table"]) == 0
        for cls in ("chair", "table"):
            own, assembled = values(cls), values(cls, "--assembled")
            print(cls, own, assembled, np.abs(own - assembled))
            assert np.array_equal(np.isnan(own), np.isnan(assembled)) and not np.isnan(own).all() and 0 < own[0] < 1
            assert (np.abs(own - assembled)[~np.isnan(own)] <= 1e-12).all()
            ranked = values(cls, "--assembled", "--use-conf")                  # the files' confidences: runs, and ranks differently
            assert np.array_equal(np.isnan(ranked), np.isnan(own))
    finally:
        torch.set_num_threads(threads)
