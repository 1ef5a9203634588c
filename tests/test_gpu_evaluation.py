"""The evaluation stage on a GPU box: Evaluator (device assignment + AP / recall) against what the reference's ScanNetEval
computed (tests/golden/eval_ap.npz), ground truth kept resident across prediction lists, scoring straight from the
device rows of a refinement result, and tools/eval_scannet200.py run as the child process run_evl.py would start."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import eval_ap_case as case
import golden_io as gio
from oracle.eval_ref import flatten_assignment
from oracle.make_golden_shared import bank_encoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ev():
    from beyond_fixed_forms_amd import _lib, evaluation
    _lib.load()
    return evaluation


def device_rows(masks):
    from beyond_fixed_forms_amd import _lib
    return _lib.pack_rows(torch.from_numpy(np.ascontiguousarray(np.asarray(masks) != 0)).to(DEV))


def slim(preds):
    return [{k: v for k, v in p.items() if k != "pred_mask"} for p in preds]


@pytest.mark.parametrize("name", case.CASES)
def test_evaluator_golden(ev, name):
    """Every fixture case through Evaluator in three forms -- dense masks, pre-packed device rows, and GroundTruthScan
    objects built once and reused for two prediction lists over the same scans (the case's own confidences, then all
    1.0) -- each within the fixture's bounds of the reference's ap / rc / means (eval_ap_case.assert_scores)."""
    labels = case.class_labels()
    use_label, scans = case.scans(name)
    _, scans_one = case.scans(name, conf_one=True)

    def run(add):
        e = ev.Evaluator(labels, use_label=use_label, device=DEV)
        for i in range(len(scans)):
            add(e, i)
        ap, rc = e.ap_rc()
        assert list(e.matches) == [f"gt_{i}" for i in range(len(scans))]
        return ap, rc, e.evaluate()

    case.assert_scores(name, False, *run(lambda e, i: e.add_scan(scans[i][2], scans[i][0], scans[i][1])))
    rows = [device_rows([p["pred_mask"] for p in s[2]]) if s[2] else None for s in scans]
    case.assert_scores(name, False, *run(lambda e, i: e.add_scan(slim(scans[i][2]), scans[i][0], scans[i][1], pred_rows=rows[i])))
    truth = [ev.prepare_ground_truth(s[0], s[1], labels, device=DEV) for s in scans]
    for conf_one, lists in ((False, scans), (True, scans_one)):
        got = run(lambda e, i: e.add_scan(slim(lists[i][2]), ground_truth=truth[i], pred_rows=rows[i]) if rows[i] is not None
                  else e.add_scan([], ground_truth=truth[i]))
        case.assert_scores(name, conf_one, *got)


@pytest.mark.parametrize("name", ["labelled_a", "labelled_b", "agnostic", "no_preds"])
def test_assign_with_resident_ground_truth(ev, name, monkeypatch):
    """assign_instances_for_scan(ground_truth=...) returns the dicts of the call without it (and of the reference:
    eval_assign.npz), with gts_sem / gts_ins None, and derives nothing from the ground truth again: no encode, no
    np.unique / np.in1d, no ids_to_rows."""
    from beyond_fixed_forms_amd import _lib
    z = np.load(os.path.join(gio.GOLDEN_DIR, "eval_assign.npz"))
    labels = [str(s) for s in z["class_labels"]]
    preds, sem, ins, use_label, exp = gio.eval_case(z, name)
    ev_labels = labels if use_label else ["class_agnostic"]
    plain = flatten_assignment(*ev.assign_instances_for_scan(preds, sem, ins, labels, use_label=use_label, device=DEV), ev_labels)
    gio.same_assignment(plain, exp)
    truth = ev.prepare_ground_truth(sem, ins, labels, device=DEV)
    assert truth.rows.shape == (len(truth.instance_ids), (len(sem) + 63) // 64) and truth.void_row.shape[0] == 1
    assert np.array_equal(truth.vert_count, [(truth.gts == i).sum() for i in truth.instance_ids])
    assert np.array_equal(truth.label_ids, truth.instance_ids // 1000) and np.all(np.diff(truth.instance_ids) > 0)

    def forbidden(*a, **k):
        raise AssertionError("the ground truth was derived again")
    for mod, fn in ((np, "unique"), (np, "in1d"), (np, "isin"), (_lib, "ids_to_rows"), (ev, "encode_gt"),
                    (ev, "prepare_ground_truth")):
        monkeypatch.setattr(mod, fn, forbidden, raising=False)
    for _ in range(2):                                                    # the object is not consumed by a call
        got = ev.assign_instances_for_scan(preds, None, None, labels, use_label=use_label, device=DEV, ground_truth=truth)
        gio.same_assignment(flatten_assignment(*got, ev_labels), plain)
    if preds:
        rows = device_rows([p["pred_mask"] for p in preds])
        got = ev.assign_instances_for_scan(slim(preds), None, None, labels, use_label=use_label, device=DEV, pred_rows=rows,
                                           ground_truth=truth)
        gio.same_assignment(flatten_assignment(*got, ev_labels), plain)
    monkeypatch.undo()
    with pytest.raises(ValueError):
        ev.assign_instances_for_scan(preds, None, None, labels[:-1], use_label=use_label, device=DEV, ground_truth=truth)


def test_refined_scene_scored_from_device_rows(ev):
    """One small generator scene through project_scene + refine_class; the FinalResult's device rows go straight into
    Evaluator.add_scan and give the evaluation of the same result's to_dict() dense masks.  Ground truth: the
    generator's point_object -- every cuboid an instance of the query class, the room an instance of a second class."""
    from beyond_fixed_forms_amd import projection, refinement
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.synthetic import make_scene, make_text_bank
    scene = make_scene("tiny", seed=3, cut_masks=False)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
    bank, index = make_text_bank(64, seed=5)
    sim = refinement.TextSimilarity(bank_encoder(bank.float(), index), DEV)
    stage2 = projection.project_scene(scene, cfg, DEV, return_result=True)
    fin = refinement.refine_class([(scene.scene_id, scene.stage1, stage2)], cfg, "table", sim, DEV)[scene.scene_id]
    assert fin.rows is not None and fin.rows.shape[0] >= 1 and set(fin.final_class) == {"table"}
    labels = ["table", "room", "lamp"]
    obj = scene.point_object
    sem = np.where(obj >= 0, 2, 3).astype(np.int32)                       # scannet200: label id = sem - 1
    ins = (obj + 1).astype(np.int32)
    preds = [{"scan_id": scene.scene_id, "label_id": float(labels.index(c) + 1), "conf": 1.0} for c in fin.final_class]
    from_rows = ev.Evaluator(labels, device=DEV)
    from_rows.add_scan(preds, sem, ins, pred_rows=fin.rows)
    dense = fin.to_dict()["ins"].cpu().numpy()
    assert dense.shape == (len(preds), scene.points.shape[0])
    from_dense = ev.Evaluator(labels, device=DEV)
    from_dense.add_scan([dict(p, pred_mask=m) for p, m in zip(preds, dense)], sem, ins)
    (ap_r, rc_r), (ap_d, rc_d) = from_rows.ap_rc(), from_dense.ap_rc()
    assert np.array_equal(ap_r, ap_d, equal_nan=True) and np.array_equal(rc_r, rc_d, equal_nan=True)
    gio.same_assignment(flatten_assignment(from_rows.matches["gt_0"]["gt"], from_rows.matches["gt_0"]["pred"], labels),
                        flatten_assignment(from_dense.matches["gt_0"]["gt"], from_dense.matches["gt_0"]["pred"], labels))
    assert not np.isnan(ap_r[0, 0]).any() and np.all(ap_r[0, 1] == 0) and np.isnan(ap_r[0, 2]).all()
    assert from_rows.evaluate()["classes"]["table"] == from_dense.evaluate()["classes"]["table"]


SEMANTIC_IDS = [1, 3, 7, 11, 12, 20, 33, 40]              # the dataset's raw ids: wall, floor, then the six classes
CLASS_LABELS = ["chair", "table", "door", "couch", "armchair", "bed"]


def cli_scene(seed, n):
    """Blocky ground truth in the dataset's raw semantic ids (0 and an unlisted id among them) and predictions for
    two classes that cover their instances partly / wholly / not at all."""
    rng = np.random.default_rng(seed)
    sem, ins = np.zeros(n, np.float32), np.zeros(n, np.float32)
    at = k = 0
    while at < n:
        ln = int(rng.integers(80, 400))
        sem[at:at + ln] = rng.choice([0, 1, 3, 7, 7, 11, 11, 12, 20, 33, 40, 999])
        ins[at:at + ln] = k
        k, at = k + 1, at + ln
    perm = rng.permutation(n)
    sem, ins = sem[perm], ins[perm]
    masks, classes = [], []
    for raw, cls in ((7, "chair"), (11, "table")):
        for target in np.unique(ins[sem == raw]):
            m = (ins == target) & (rng.random(n) < rng.uniform(0.4, 1.0))
            m |= rng.random(n) < rng.uniform(0.0, 0.03)
            masks.append(m)
            classes.append(cls)
        masks.append(rng.random(n) < 0.05)
        classes.append(cls)
    return sem, ins, np.stack(masks), classes


def test_eval_script(ev, tmp_path):
    """tools/eval_scannet200.py as a child process: three scenes (final files with dense rows, with RLE dicts, with a
    class tensor), a made-up label table of six classes.  Exit code 0, the class's line = an in-process Evaluator's
    values, result.txt beside it, a second class leaves the first line alone, a class without output exits 1."""
    from beyond_fixed_forms_amd.config import Config
    from beyond_fixed_forms_amd.synthetic import _rle_from_dense
    scenes = {f"scene{70 + k:04d}_00": cli_scene(70 + k, 3000 + 7 * k) for k in range(3)}
    (tmp_path / "gt").mkdir()
    expected = {}
    for cls in ("chair", "table"):
        (tmp_path / "final" / cls).mkdir(parents=True)
        inproc = ev.Evaluator(CLASS_LABELS, device=DEV)
        for k, (scene_id, (sem, ins, masks, classes)) in enumerate(sorted(scenes.items())):
            torch.save((np.zeros((len(sem), 3), np.float32), np.zeros((len(sem), 3), np.float32), sem, ins),
                       tmp_path / "gt" / f"{scene_id}.pth")
            own = [i for i, c in enumerate(classes) if c == cls]
            dense = torch.from_numpy(masks[own])
            final_class = [cls.capitalize() if k == 0 else cls] * len(own)                 # the script lower-cases
            if k == 1:
                out = {"ins": _rle_from_dense(dense), "conf": torch.rand(len(own)), "final_class": final_class}
            elif k == 2:
                out = {"ins": dense.to(torch.uint8) * 1, "conf": torch.rand(len(own)),
                       "final_class": torch.tensor([CLASS_LABELS.index(cls)] * len(own))}
            else:
                out = {"ins": dense, "conf": torch.rand(len(own)), "final_class": final_class}
            torch.save(out, tmp_path / "final" / cls / f"{scene_id}.pth")
            positions = ev.semantic_positions(sem, SEMANTIC_IDS)
            inproc.add_scan([{"scan_id": scene_id, "label_id": float(CLASS_LABELS.index(cls) + 1), "conf": 1.0,
                              "pred_mask": m.astype(np.uint8)} for m in masks[own]], positions, ins.astype(np.int32))
        avgs = inproc.evaluate()
        expected[cls] = avgs
        values = [avgs["classes"][cls][key] for key in ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%")]
        assert 0 < values[0] < 1                                                           # a score worth comparing
    cfg = Config.with_defaults(final_output_dir=str(tmp_path / "final"))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(dict(cfg)))
    (tmp_path / "labels.json").write_text(json.dumps({"class_labels": CLASS_LABELS, "semantic_ids": SEMANTIC_IDS}))
    results = tmp_path / "eval_results" / "overall_results.txt"

    def run(cls):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_scannet200.py"), "--cls", cls,
                               "--config", str(tmp_path / "config.yaml"), "--gt-dir", str(tmp_path / "gt"),
                               "--results-file", str(results), "--label-table", str(tmp_path / "labels.json")],
                              cwd=tmp_path, capture_output=True, text=True, timeout=600)

    def line_of(cls):
        a = expected[cls]["classes"][cls]
        return ",".join([cls] + [str(a[key]) for key in ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%")] + [""])

    r = run("chair")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = results.read_text().split("\n")
    assert lines[0] == "class,class id,ap,ap50,ap25,rc,rc50,rc25" and lines[1] == line_of("chair")
    assert lines[2:] == [f"{c},-,-,-" for c in CLASS_LABELS[1:]] + [""]
    written = (tmp_path / "eval_results" / "result.txt").read_text().split("\n")
    assert written[0] == "class,class id,ap,ap50,ap25" and written[1] + "," == line_of("chair")
    assert len(written) == len(CLASS_LABELS) + 4
    r = run("table")
    assert r.returncode == 0, r.stderr[-2000:]
    lines2 = results.read_text().split("\n")
    assert lines2[2] == line_of("table") and lines2[:2] == lines[:2] and lines2[3:] == lines[3:]
    r = run("bed")                                                                         # no final/bed directory
    assert r.returncode == 1 and "bed" in r.stderr
    assert results.read_text().split("\n") == lines2
