"""The AP / recall half of the evaluation (evaluation.evaluate_matches, compute_averages, the result files and the
per-class script's host pieces) against what the reference's ScanNetEval computed: tests/golden/eval_ap.npz.  No GPU:
the matches come from oracle.eval_ref's CPU assignment, itself pinned to the reference by eval_assign.npz."""
import numpy as np
import pytest

import eval_ap_case as case
from beyond_fixed_forms_amd import evaluation as ev
from oracle.eval_ref import assign_instances_ref


def ref_matches(name, conf_one=False):
    use_label, scans = case.scans(name, conf_one)
    labels = case.class_labels()
    matches = {}
    for i, (sem, ins, preds) in enumerate(scans):
        gt2pred, pred2gt = assign_instances_ref(preds, sem, ins, labels, use_label=use_label)
        matches[f"gt_{i}"] = {"gt": gt2pred, "pred": pred2gt}
    return matches, (labels if use_label else ["class_agnostic"])


@pytest.mark.parametrize("conf_one", [False, True], ids=["conf", "conf1"])
@pytest.mark.parametrize("name", case.CASES)
def test_evaluate_matches_golden(name, conf_one):
    """Every fixture case, with its own confidences and with every confidence 1.0: NaN pattern and recall exactly, AP and
    the means within the summation-order bound (eval_ap_case.assert_scores)."""
    matches, eval_labels = ref_matches(name, conf_one)
    lengths = []
    ap, rc = ev.evaluate_matches(matches, eval_labels, curve_lengths=lengths)
    assert ap.shape == (1, len(eval_labels), 10)
    case.assert_scores(name, conf_one, ap, rc, ev.compute_averages(ap, rc, eval_labels))
    assert max(lengths) <= int(case.fixture()[f"{name}.k_max"])


def test_thresholds_are_the_reference_doubles():
    th = ev.iou_thresholds()
    assert th.shape == (10,) and th[-1] == 0.25 and th[0] == 0.5 and th[2] == 0.6000000000000001
    assert np.array_equal(th, np.append(np.arange(0.5, 0.95, 0.05), 0.25))


@pytest.mark.parametrize("confs, ap_expected", [((0.9, 0.4), 1.0), ((1.0, 1.0), 0.75)])
def test_hand_case(confs, ap_expected):
    """One ground-truth instance of 200 points, two predictions of IoU 1 and 0.975.  Confidences 0.9 / 0.4: the second
    is a false positive below the match, precision [0.5, 1, 1], recall [1, 1, 0], step widths [0, 0.5, 0.5]: AP 1.
    Both 1.0: one threshold, precision [0.5, 1], recall [1, 0], widths [0.5, 0.5]: AP 0.75.  Recall 1 in both."""
    n = 400
    sem, ins = np.zeros(n, np.int32), np.zeros(n, np.int32)
    sem[:200], ins[:200] = 2, 5
    masks = [np.arange(n) < 200, np.arange(n) < 195]
    preds = [{"scan_id": "hand_00", "label_id": 1.0, "conf": c, "pred_mask": m.astype(np.uint8)} for c, m in zip(confs, masks)]
    labels = case.class_labels()
    gt2pred, pred2gt = assign_instances_ref(preds, sem, ins, labels)
    ap, rc = ev.evaluate_matches({"gt_0": {"gt": gt2pred, "pred": pred2gt}}, labels)
    assert np.all(ap[0, 0] == ap_expected) and np.all(rc[0, 0] == 1.0)
    assert np.isnan(ap[0, 1:]).all() and np.isnan(rc[0, 1:]).all()
    avgs = ev.compute_averages(ap, rc, labels)
    assert avgs["all_ap"] == ap_expected and avgs["all_rc_25%"] == 1.0
    assert avgs["classes"][labels[0]]["ap50%"] == ap_expected and np.isnan(avgs["classes"][labels[1]]["ap"])


def test_loop_arrangement_does_not_change_the_result():
    """Labels without ground truth and predictions are written NaN without being walked; walking only a subset of the
    labels, or the scans under other keys, gives the same numbers for the labels that remain."""
    matches, eval_labels = ref_matches("labelled")
    ap, rc = ev.evaluate_matches(matches, eval_labels)
    live = [li for li, lab in enumerate(eval_labels) if any(m["gt"][lab] or m["pred"][lab] for m in matches.values())]
    assert 0 < len(live) < 20
    ap_s, rc_s = ev.evaluate_matches(matches, [eval_labels[li] for li in live])
    assert np.array_equal(ap_s[0], ap[0, live], equal_nan=True) and np.array_equal(rc_s[0], rc[0, live], equal_nan=True)
    dead = np.setdiff1d(np.arange(len(eval_labels)), live)
    assert np.isnan(ap[0, dead]).all() and np.isnan(rc[0, dead]).all()


def test_reference_shaped_dicts_with_extra_keys():
    """The dicts need only the reference's keys; more keys (per scan, per instance) and other scan keys change nothing."""
    matches, eval_labels = ref_matches("labelled")
    ap, rc = ev.evaluate_matches(matches, eval_labels)
    other = {}
    for k, m in matches.items():
        gt = {lab: [dict(g, note="x", matched_pred=[dict(p, extra=1) for p in g["matched_pred"]]) for g in lst]
              for lab, lst in m["gt"].items()}
        pred = {lab: [dict(p, colour=3, matched_gt=[dict(g, extra=2) for g in p["matched_gt"]]) for p in lst]
                for lab, lst in m["pred"].items()}
        gt["not a label"], pred["not a label"] = [], []
        other["scan " + k] = {"gt": gt, "pred": pred, "scene": k}
    ap2, rc2 = ev.evaluate_matches(other, eval_labels)
    assert np.array_equal(ap, ap2, equal_nan=True) and np.array_equal(rc, rc2, equal_nan=True)


@pytest.mark.parametrize("name", case.CASES)
def test_result_file_and_table(name, tmp_path):
    """write_result_file line by line against the file the reference wrote (its five-name header over seven values
    included), format_results against what the reference printed."""
    z = case.fixture()
    eval_labels = case.class_labels() if case.scans(name)[0] else ["class_agnostic"]
    # the golden arrays stand in for ours: the texts then depend on the formatting alone, not on BLAS's last bit
    e_ap, e_rc, _ = case.expected(name)
    avgs = ev.compute_averages(e_ap, e_rc, eval_labels)
    path = tmp_path / "result.txt"
    ev.write_result_file(avgs, eval_labels, str(path))
    got, exp = path.read_text().split("\n"), str(z[f"{name}.result_txt"]).split("\n")
    assert len(got) == len(exp) == len(eval_labels) + 4
    for a, b in zip(got, exp):
        assert a == b
    assert got[0] == "class,class id,ap,ap50,ap25" and len(got[1].split(",")) == 7
    table = ev.format_results(avgs, eval_labels)
    assert table == str(z[f"{name}.print_txt"])
    rows = table.split("\n")
    assert rows[1] == "#" * 64 and rows[3] == "#" * 64 and rows[-5] == "-" * 64
    for row in rows[4:4 + len(eval_labels)] + [rows[-4]]:
        what, values = row.split(":", 1)[0], row.split(":", 1)[1]
        assert len(what) >= 15 and len(values) == 6 * 8


def test_results_file_rule(tmp_path):
    """Create the summary file (header + one `name,-,-,-` line per class), replace one class's line, leave the rest."""
    labels = ["chair", "armchair", "table", "bed"]
    path = tmp_path / "sub" / "overall_results.txt"
    ev.update_results_file(str(path), "chair", [0.5, 0.25, 1.0, 0.125, 0.0, float("nan")], labels)
    lines = path.read_text().split("\n")
    assert lines == ["class,class id,ap,ap50,ap25,rc,rc50,rc25", "chair,0.5,0.25,1.0,0.125,0.0,nan,", "armchair,-,-,-",
                     "table,-,-,-", "bed,-,-,-", ""]
    ev.update_results_file(str(path), "table", [np.float64(0.1)] * 6, labels)
    lines2 = path.read_text().split("\n")
    assert lines2[3] == "table," + "0.1," * 6
    assert lines2[:3] == lines[:3] and lines2[4:] == lines[4:]            # "chair," does not match "armchair,..."
    ev.update_results_file(str(path), "chair", [1, 2, 3, 4, 5, 6], labels)
    lines3 = path.read_text().split("\n")
    assert lines3[1] == "chair,1,2,3,4,5,6," and lines3[2:] == lines2[2:]
    ev.update_results_file(str(path), "no such class", [0] * 6, labels)   # no line starts with it: nothing changes
    assert path.read_text().split("\n") == lines3


def test_semantic_positions_against_list_index():
    """The vectorised look-up against the reference's per-point formulation (eval_scannet200.py:92)."""
    rng = np.random.default_rng(0)
    table = [int(v) for v in rng.permutation(np.arange(1, 1200))[:200]]
    sem_gt = rng.choice(np.asarray([0] + table[:60] + [5000, 1201, 7]), 5000).astype(np.float32)
    sem_gt[:3] = [0, table[0], table[-1]]
    per_point = [table.index(int(s)) if s != 0 and int(s) in table else -1 for s in sem_gt]
    got = ev.semantic_positions(sem_gt, table)
    assert got.dtype == np.int32 and np.array_equal(got, np.asarray(per_point, dtype=np.int32))
    assert (got == -1).any() and (got >= 0).any()
    dup = [4, 9, 4, 2]                                                     # list.index returns the first position
    assert ev.semantic_positions(np.array([4, 2, 9, 0, 3]), dup).tolist() == [0, 3, 1, -1, -1]
    assert ev.semantic_positions(np.array([], np.int64), dup).shape == (0,)
