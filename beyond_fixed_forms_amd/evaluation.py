"""The consumer right after the hot path: ScanNet instance evaluation, reference
evaluation/eval/scannetv2_inst_eval.py (EVAL below) with instance_eval_util.py:158-174 (`get_instances`), from the
prediction <-> ground-truth assignment (`assign_instances_for_scan`, EVAL:265-365) to AP / AP50 / AP25 and recall
(`evaluate_matches` EVAL:56-238, `compute_averages` EVAL:241-263, the result file EVAL:549-562).

The reference counts, pair by pair, `np.count_nonzero(np.logical_and(gts == instance_id, pred_mask))` over N points
(O(P x G x N) byte operations per scene); here the predicted masks and the ground-truth instances are bit rows on
the device and ONE popcount Gram (bff_cross_popcount) delivers every intersection, the void intersections and the
vertex counts; the host then assembles the reference's nested dicts in the reference's order.  What depends on the
ground truth alone (`GroundTruthScan`: encoded ids, instance bit rows, void row, vertex counts) is built once per scene
and reused by every class evaluated on it.  The AP curves are O(matches) host arithmetic: the reference's NumPy float64
operations in the reference's order, so a score equals the reference's to the last bit of everything but BLAS's
summation order inside `np.dot`.  `Evaluator` chains the two for a list of scans.
"""
from __future__ import annotations

import dataclasses
import os
from copy import deepcopy

import numpy as np
import torch

from . import _lib

MIN_REGION_SIZE = {"stpls3d": 10}        # scannetv2_inst_eval.py:42-45 (everything else: 100)
SEM_OFFSET = {"scannetv2": 2, "scannet200": 2, "replica": 1, "stpls3d": 1, "scannetpp": 105}     # :270-281


def pred_gt_overlaps(pred_rows: torch.Tensor, gts: torch.Tensor, instance_ids, void_mask=None):
    """pred_rows: int64 bit rows [P][nw] (device) of the predicted masks (FinalResult.rows / Stage2Result.rows, or
    _lib.pack_rows of a dense bool matrix); gts: int64 [N] encoded ground-truth ids per point
    (`gts_sem * encode_value + gts_ins`, :286-291); instance_ids: the `instance_id` of the GT instances to match.

    Returns numpy arrays
      intersection [P][G]   = count_nonzero(logical_and(gts == instance_id, pred_mask))          (:334)
      pred_count   [P]      = count_nonzero(pred_mask)                                           (:318)
      gt_count     [G]      = number of points of each GT instance (its `vert_count`)
      void_inter   [P]      = count_nonzero(logical_and(bool_void, pred_mask)) if void_mask is given (:328)
    """
    dev = pred_rows.device
    gts = gts.to(dev).to(torch.int64).contiguous()
    vals = torch.as_tensor(np.asarray(instance_ids, dtype=np.int64)).to(dev)
    gt_rows = _lib.ids_to_rows(gts, vals)
    out = [_lib.cross_popcount(pred_rows, gt_rows), _lib.popcount_rows(pred_rows), _lib.popcount_rows(gt_rows)]
    if void_mask is not None:
        void_rows = _lib.pack_rows(torch.as_tensor(void_mask).to(dev).reshape(1, -1).to(torch.bool).contiguous())
        out.append(_lib.cross_popcount(pred_rows, void_rows))
    res = _lib.fetch(*out)
    return res[0], res[1], res[2], (res[3][:, 0] if void_mask is not None else None)


def encode_gt(gts_sem, gts_ins, dataset_name="scannet200"):
    """:270-291: shift the semantic ids of the dataset, clamp negatives, `sem * encode_value + (ins + 1)`, 0 where the
    instance id is ignored.  Returns (gts int array [N], encode_value)."""
    encode = 10000 if dataset_name == "scannetpp" else 1000                       # :23-27
    sem = np.array(gts_sem) - SEM_OFFSET.get(dataset_name, 0) + 1
    sem[sem < 0] = 0
    ins = np.array(gts_ins) + 1
    gts = sem * encode + ins
    gts[ins < 0] = 0
    return gts, encode


@dataclasses.dataclass
class GroundTruthScan:
    """Everything `assign_instances_for_scan` derives from one scan's ground truth alone (EVAL:270-292, 315), resident
    on the device: built once per scene by `prepare_ground_truth`, reused by every class and every prediction list
    evaluated on that scene (the reference rebuilds it per (class, scene))."""
    n_points: int
    dataset_name: str
    n_labels: int                  # len(class_labels) it was built for: the valid ids are 1..n_labels
    encode: int
    gts: np.ndarray                # [N] encoded id per point, `sem * encode + ins + 1`, 0 where ignored (EVAL:288-289)
    instance_ids: np.ndarray       # int64 [G] ascending, 0 left out (get_instances)
    label_ids: np.ndarray          # int64 [G] `instance_id // encode`
    vert_count: np.ndarray         # int64 [G] points of each instance
    rows: torch.Tensor             # int64 [G][nw] device bit rows, rows[g] = (gts == instance_ids[g])
    void_row: torch.Tensor         # int64 [1][nw] device bit row of the points whose class is not a valid one (EVAL:315)


def prepare_ground_truth(gts_sem, gts_ins, class_labels, dataset_name="scannet200", device="cuda") -> GroundTruthScan:
    """Per-point semantic and instance ids of one scan -> its GroundTruthScan on `device`."""
    _lib.load()
    dev = torch.device(device)
    n_labels = len(class_labels)
    gts, encode = encode_gt(gts_sem, gts_ins, dataset_name)
    n = gts.shape[0]
    inst_ids = np.unique(gts)
    inst_ids = inst_ids[inst_ids != 0].astype(np.int64)
    gts_dev = torch.from_numpy(np.ascontiguousarray(gts, dtype=np.int64)).to(dev)
    bool_void = np.logical_not(np.isin(gts // encode, np.arange(n_labels) + 1))   # :315 (np.in1d there)
    void_row = _lib.pack_rows(torch.from_numpy(bool_void).to(dev).reshape(1, -1).contiguous())
    if len(inst_ids):
        rows = _lib.ids_to_rows(gts_dev, torch.from_numpy(inst_ids).to(dev))
        vert_count = _lib.popcount_rows(rows).cpu().numpy().astype(np.int64)
    else:
        rows = torch.zeros((0, (n + 63) // 64), dtype=torch.int64, device=dev)
        vert_count = np.zeros(0, np.int64)
    return GroundTruthScan(n, dataset_name, n_labels, encode, gts, inst_ids, inst_ids // encode, vert_count, rows, void_row)


def assign_instances_for_scan(preds, gts_sem, gts_ins, class_labels, use_label=True, dataset_name="scannet200",
                              device="cuda", pred_rows=None, ground_truth=None):
    """ScanNetEval.assign_instances_for_scan (:265-365) -> (gt2pred, pred2gt), the same nested dicts.

    preds: list of {"scan_id", "label_id", "conf", "pred_mask"}; pred_mask is an (N,) array (anything != 0 is set),
    or ignored when `pred_rows` (int64 bit rows [len(preds)][nw] on the device, e.g. FinalResult.rows) is given.
    class_labels: the evaluator's valid_class_labels (ids 1..len).
    ground_truth: the scan's GroundTruthScan (prepare_ground_truth with the same class_labels and dataset_name); then
    gts_sem / gts_ins are not read (they may be None) and nothing of the ground truth is derived or uploaded again."""
    _lib.load()
    labels = list(class_labels)
    valid_ids = np.arange(len(labels)) + 1                                        # :30
    id2label = {int(i): lab for i, lab in zip(valid_ids, labels)}
    eval_labels = labels if use_label else ["class_agnostic"]                     # :55-58
    truth = ground_truth
    if truth is None:
        truth = prepare_ground_truth(gts_sem, gts_ins, labels, dataset_name, device)
    elif truth.n_labels != len(labels) or truth.dataset_name != dataset_name:
        raise ValueError("ground_truth was prepared for another label set or dataset")
    dev = truth.rows.device
    encode, n, inst_ids, gt_count = truth.encode, truth.n_points, truth.instance_ids, truth.vert_count
    min_region = MIN_REGION_SIZE.get(dataset_name, 100)

    # ---- predictions that reach the counting stage (label known)
    keep = []
    for k, pred in enumerate(preds):
        if use_label and pred["label_id"] not in id2label:                        # :311-312
            continue
        keep.append(k)
    if pred_rows is None:
        if keep:
            dense = torch.from_numpy(np.stack([np.not_equal(np.asarray(preds[k]["pred_mask"]), 0) for k in keep]))
            for k in keep:
                assert np.asarray(preds[k]["pred_mask"]).shape[0] == n            # :320
            rows = _lib.pack_rows(dense.to(dev).contiguous())
        else:
            rows = torch.zeros((0, (n + 63) // 64), dtype=torch.int64, device=dev)
    else:
        assert pred_rows.shape[1] == (n + 63) // 64                               # :320 for rows
        rows = _lib.gather_rows(pred_rows, torch.tensor(keep, dtype=torch.int32, device=dev)) if keep else pred_rows[:0]
    # ---- ONE Gram of the predictions against the resident ground-truth rows, the void row and their own counts
    if len(keep) and len(inst_ids):
        inter, pred_count, void_inter = _lib.fetch(_lib.cross_popcount(rows, truth.rows), _lib.popcount_rows(rows),
                                                   _lib.cross_popcount(rows, truth.void_row))
        void_inter = void_inter[:, 0]
    else:
        if len(keep):
            pred_count, void_inter = _lib.fetch(_lib.popcount_rows(rows), _lib.cross_popcount(rows, truth.void_row))
            void_inter = void_inter[:, 0]
        else:
            pred_count = void_inter = np.zeros(0, np.int32)
        inter = np.zeros((len(keep), len(inst_ids)), np.int32)

    gt_instances = {lab: [] for lab in labels}
    col_of = {}                                                                    # (label, position) -> Gram column
    for c, iid in enumerate(inst_ids):
        label_id = int(iid // encode)
        if label_id in id2label:
            lab = id2label[label_id]
            col_of[(lab, len(gt_instances[lab]))] = c
            gt_instances[lab].append({"instance_id": int(iid), "label_id": label_id, "vert_count": int(gt_count[c]),
                                      "med_dist": -1, "dist_conf": 0.0, "box": np.zeros((6))})
    if use_label:                                                                  # :294-298
        gt2pred = deepcopy(gt_instances)
        for lab in gt2pred:
            for gt in gt2pred[lab]:
                gt["matched_pred"] = []
        cols = {lab: [col_of[(lab, k)] for k in range(len(v))] for lab, v in gt2pred.items()}
    else:                                                                          # :300-308
        agnostic, acols = [], []
        for lab, instances in gt_instances.items():
            agnostic += deepcopy(instances)
            acols += [col_of[(lab, k)] for k in range(len(instances))]
        for gt in agnostic:
            gt["matched_pred"] = []
        gt2pred = {eval_labels[0]: agnostic}
        cols = {eval_labels[0]: acols}

    # ---- predictions that are large enough to count (:323-324), numbered in input order (:358-360)
    pred2gt = {lab: [] for lab in eval_labels}
    pred_count = np.asarray(pred_count, dtype=np.int64)
    big = np.flatnonzero(pred_count >= min_region)
    records, by_label = [], {lab: [] for lab in eval_labels}
    for number, r in enumerate(big.tolist()):
        pred = preds[keep[r]]
        lab = id2label[pred["label_id"]] if use_label else eval_labels[0]
        rec = {"filename": "{}_{}".format(pred["scan_id"], number), "pred_id": number,
               "label_id": pred["label_id"] if use_label else None, "vert_count": int(pred_count[r]),
               "confidence": pred["conf"], "void_intersection": int(void_inter[r])}
        records.append(rec)
        by_label[lab].append((r, len(records) - 1))
    # ---- matches = the non-zero entries of the Gram block (predictions of a label) x (ground truth of that label);
    # np.nonzero walks it row-major, i.e. prediction by prediction and within one by ground-truth position, the order
    # in which the reference's nested loops meet them (:331-357).  IoU = I / (|gt| + |pred| - I) in float64 (:340)
    matched = [[] for _ in records]
    for lab, members in by_label.items():
        gt_list = gt2pred[lab]
        if not members or not gt_list:
            continue
        r_idx = np.array([m[0] for m in members])
        block = np.asarray(inter, dtype=np.int64)[np.ix_(r_idx, np.asarray(cols[lab], dtype=np.int64))]
        pi, gi = np.nonzero(block > 0)
        hit = block[pi, gi]
        gt_verts = np.array([g["vert_count"] for g in gt_list], dtype=np.int64)
        iou = hit.astype(np.float64) / (gt_verts[gi] + pred_count[r_idx][pi] - hit).astype(np.float64)
        for p_, g_, i_, u_ in zip(pi.tolist(), gi.tolist(), hit.tolist(), iou.tolist()):
            rec_no = members[p_][1]
            gt = gt_list[g_]
            # the ground-truth side keeps a snapshot of the prediction as it is before its own matches are attached,
            # the prediction side a shallow snapshot of the ground-truth entry (its match list stays the shared one)
            gt["matched_pred"].append(dict(records[rec_no], intersection=i_, iou=u_))
            matched[rec_no].append(dict(gt, intersection=i_, iou=u_))
    for rec, m in zip(records, matched):
        rec["matched_gt"] = m
    for lab, members in by_label.items():
        pred2gt[lab] = [records[k] for _, k in members]
    return gt2pred, pred2gt


# --------------------------------------------------------------------------- AP / recall from the matches
def iou_thresholds():
    """EVAL:38, the reference's expression: the same doubles (0.6000000000000001 among them); 0.25 is the last."""
    return np.append(np.arange(0.5, 0.95, 0.05), 0.25)


def _average_precision(y_true, y_score, hard_false_negatives):
    """EVAL:176-225: the precision / recall curve over the distinct scores and its area -> (ap, rc, curve length).
    The same NumPy calls in the same order; the per-threshold loop of :201-209 is written on whole arrays, element by
    element the same float64 operations."""
    order = np.argsort(y_score)
    score, true = y_score[order], y_true[order]
    below = np.cumsum(true)                                # true examples up to and including each position
    _, first = np.unique(score, return_index=True)         # where each distinct score starts
    k = len(first) + 1
    n_all, n_true = len(score), below[-1]
    precision, recall = np.zeros(k), np.zeros(k)
    below = np.append(below, 0)                            # what index -1 reads for the lowest score
    lost = below[first - 1]                                # true examples scored under the threshold
    tp = n_true - lost
    fp = n_all - first - tp
    fn = lost + hard_false_negatives
    precision[:-1] = tp / (tp + fp)
    recall[:-1] = tp / (tp + fn)
    rc = recall[0]                                         # the recall of the lowest threshold
    precision[-1], recall[-1] = 1.0, 0.0                   # the artificial end of the curve
    padded = np.append(np.append(recall[0], recall), 0.0)
    widths = np.convolve(padded, [-0.5, 0, 0.5], "valid")
    return np.dot(precision, widths), rc, k


def evaluate_matches(matches, eval_class_labels, dataset_name="scannet200", curve_lengths=None):
    """ScanNetEval.evaluate_matches (EVAL:56-238) -> (ap, rc), float64 [1][len(eval_class_labels)][10]: per label and
    IoU threshold (0.5 ... 0.9, then 0.25) the average precision and the recall, NaN where a label has no ground truth.

    matches: {key: {"gt": gt2pred, "pred": pred2gt}}, what assign_instances_for_scan (ours or the reference's) returns
    per scan.  A label that has neither a ground-truth instance nor a prediction in any scan is decided once (NaN)
    and never walked.  curve_lengths: a list that receives the length of every curve integrated (for error bounds)."""
    labels = list(eval_class_labels)
    ious = iou_thresholds()
    encode = 10000 if dataset_name == "scannetpp" else 1000
    min_region_size = MIN_REGION_SIZE.get(dataset_name, 100)
    distance_thresh, distance_conf = float("inf"), -float("inf")                   # EVAL:46-47
    ap = np.zeros((1, len(labels), len(ious)), float)
    rc = np.zeros((1, len(labels), len(ious)), float)
    scans = list(matches.values())
    live = [li for li, lab in enumerate(labels) if any(s["gt"][lab] or s["pred"][lab] for s in scans)]
    dead = np.ones(len(labels), bool)
    dead[live] = False
    ap[0, dead, :] = rc[0, dead, :] = float("nan")                                 # EVAL:233-235 at every threshold
    filenames = [p["filename"] for li in live for s in scans for p in s["pred"][labels[li]] if "filename" in p]
    for oi, iou_th in enumerate(ious):
        pred_visited = dict.fromkeys(filenames, False)                             # EVAL:72-78: per threshold, by filename
        for li in live:
            label_name = labels[li]
            y_true, y_score = [], []
            hard_false_negatives = 0
            has_gt = has_pred = False
            for s in scans:
                pred_instances = s["pred"][label_name]
                gt_instances = [gt for gt in s["gt"][label_name]                   # EVAL:90-97
                                if gt["instance_id"] >= encode and gt["vert_count"] >= min_region_size
                                and gt["med_dist"] <= distance_thresh and gt["dist_conf"] >= distance_conf]
                has_gt = has_gt or bool(gt_instances)
                has_pred = has_pred or bool(pred_instances)
                cur_score = [-float("inf")] * len(gt_instances)
                cur_match = [False] * len(gt_instances)
                extra = []                                                         # scores of the appended false positives
                for gti, gt in enumerate(gt_instances):                            # EVAL:107-135
                    found_match = False
                    for pred in gt["matched_pred"]:
                        if pred_visited[pred["filename"]]:                         # greedy
                            continue
                        if pred["iou"] > iou_th:
                            confidence = pred["confidence"]
                            if cur_match[gti]:      # a second one on this GT: the lower score is a false positive
                                extra.append(min(cur_score[gti], confidence))
                                cur_score[gti] = max(cur_score[gti], confidence)
                            else:
                                found_match = True
                                cur_match[gti] = True
                                cur_score[gti] = confidence
                                pred_visited[pred["filename"]] = True
                    if not found_match:
                        hard_false_negatives += 1
                cur_score = [c for c, m in zip(cur_score, cur_match) if m]         # EVAL:137-138
                cur_true = [1.0] * len(cur_score) + [0.0] * len(extra)
                cur_score += extra
                for pred in pred_instances:                                        # EVAL:141-166
                    if any(gt["iou"] > iou_th for gt in pred["matched_gt"]):
                        continue
                    num_ignore = pred["void_intersection"]
                    for gt in pred["matched_gt"]:
                        if gt["instance_id"] < encode:                             # group
                            num_ignore += gt["intersection"]
                        if (gt["vert_count"] < min_region_size or gt["med_dist"] > distance_thresh
                                or gt["dist_conf"] < distance_conf):               # small ground-truth instance
                            num_ignore += gt["intersection"]
                    if float(num_ignore) / pred["vert_count"] <= iou_th:
                        cur_true.append(0.0)
                        cur_score.append(pred["confidence"])
                y_true += cur_true
                y_score += cur_score
            if has_gt and has_pred:
                if len(y_true) == 0:                 # EVAL:181-184 leaves the zeros of the result arrays in place
                    ap_current = rc_current = 0.0
                else:
                    ap_current, rc_current, k = _average_precision(np.asarray(y_true, dtype=np.float64),
                                                                   np.asarray(y_score, dtype=np.float64),
                                                                   hard_false_negatives)
                    if curve_lengths is not None:
                        curve_lengths.append(k)
            elif has_gt:
                ap_current = rc_current = 0.0
            else:
                ap_current = rc_current = float("nan")
            ap[0, li, oi] = ap_current
            rc[0, li, oi] = rc_current
    return ap, rc


def compute_averages(ap, rc, eval_class_labels):
    """ScanNetEval.compute_averages (EVAL:241-263): the means over the labels that have a value, and per label."""
    ious = iou_thresholds()
    # the reference's index expressions, kept as they are: a tuple from np.where as the third index makes the selection
    # [1][T][L], and the order in which nanmean adds depends on that layout
    d = 0
    at50 = np.where(np.isclose(ious, 0.5))
    at25 = np.where(np.isclose(ious, 0.25))
    rest = np.where(np.logical_not(np.isclose(ious, 0.25)))
    avg = {"all_ap": np.nanmean(ap[d, :, rest]), "all_ap_50%": np.nanmean(ap[d, :, at50]),
           "all_ap_25%": np.nanmean(ap[d, :, at25]), "all_rc": np.nanmean(rc[d, :, rest]),
           "all_rc_50%": np.nanmean(rc[d, :, at50]), "all_rc_25%": np.nanmean(rc[d, :, at25]), "classes": {}}
    for li, label_name in enumerate(eval_class_labels):
        avg["classes"][label_name] = {"ap": np.average(ap[d, li, rest]), "ap50%": np.average(ap[d, li, at50]),
                                      "ap25%": np.average(ap[d, li, at25]), "rc": np.average(rc[d, li, rest]),
                                      "rc50%": np.average(rc[d, li, at50]), "rc25%": np.average(rc[d, li, at25])}
    return avg


_CLASS_KEYS = ("ap", "ap50%", "ap25%", "rc", "rc50%", "rc25%")
_ALL_KEYS = ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%")


def write_result_file(avgs, eval_class_labels, filename):
    """ScanNetEval.write_result_file (EVAL:549-562), its header of five names over seven values included."""
    with open(filename, "w") as f:
        f.write(",".join(["class", "class id", "ap", "ap50", "ap25"]) + "\n")
        for class_name in eval_class_labels:
            f.write(",".join(str(x) for x in [class_name] + [avgs["classes"][class_name][k] for k in _CLASS_KEYS]) + "\n")
        f.write("all_ap, all_ap50, all_ap25, all_rc, all_rc50, all_rc25\n")
        f.write(",".join(str(avgs[k]) for k in _ALL_KEYS) + "\n")


def format_results(avgs, eval_class_labels) -> str:
    """The table ScanNetEval.print_results prints (EVAL:494-546), as one string."""
    line_len = 64
    head = "{:<15}".format("what") + ":" + "".join("{:>8}".format(h) for h in ("AP", "AP_50%", "AP_25%", "AR", "RC_50%", "RC_25%"))
    out = ["", "#" * line_len, head, "#" * line_len]
    for label_name in eval_class_labels:
        out.append("{:<15}".format(label_name) + ":" + "".join("{:>8.3f}".format(avgs["classes"][label_name][k])
                                                               for k in _CLASS_KEYS))
    out += ["-" * line_len, "{:<15}".format("average") + ":" + "".join("{:>8.3f}".format(avgs[k]) for k in _ALL_KEYS),
            "#" * line_len, ""]
    return "\n".join(out) + "\n"


class Evaluator:
    """ScanNetEval.evaluate (EVAL:564-605) scan by scan: `add_scan` assigns one scan on the device, `evaluate` turns the
    scans added so far into the averages dict."""

    def __init__(self, class_labels, use_label=True, dataset_name="scannet200", device="cuda"):
        self.class_labels = list(class_labels)
        self.use_label, self.dataset_name, self.device = use_label, dataset_name, device
        self.eval_class_labels = self.class_labels if use_label else ["class_agnostic"]
        self.matches = {}

    def prepare_ground_truth(self, gts_sem, gts_ins) -> GroundTruthScan:
        return prepare_ground_truth(gts_sem, gts_ins, self.class_labels, self.dataset_name, self.device)

    def add_scan(self, preds, gts_sem=None, gts_ins=None, *, ground_truth=None, pred_rows=None):
        """One more scan: preds as for assign_instances_for_scan; the ground truth either as per-point ids or as the
        scan's GroundTruthScan; pred_rows: the masks as device bit rows (FinalResult.rows / Stage2Result.rows)."""
        gt2pred, pred2gt = assign_instances_for_scan(preds, gts_sem, gts_ins, self.class_labels, self.use_label,
                                                     self.dataset_name, self.device, pred_rows, ground_truth)
        self.matches[f"gt_{len(self.matches)}"] = {"gt": gt2pred, "pred": pred2gt}     # EVAL:586-591

    def ap_rc(self):
        return evaluate_matches(self.matches, self.eval_class_labels, self.dataset_name)

    def evaluate(self):
        ap, rc = self.ap_rc()
        return compute_averages(ap, rc, self.eval_class_labels)


# --------------------------------------------------------------------------- the per-class evaluation script's pieces
def semantic_positions(sem_gt, semantic_ids):
    """eval_scannet200.py:92 for all points at once: the dataset's raw semantic id -> its position in `semantic_ids`
    (the first one, as list.index), -1 for id 0 and for ids that are not listed.  -> int32 [N]."""
    sem = np.asarray(sem_gt).astype(np.int64).reshape(-1)                           # int(s) per point
    ids = np.asarray(semantic_ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable")                                          # equal ids: the first position wins
    at = np.searchsorted(ids[order], sem, side="left")
    at = np.minimum(at, max(len(ids) - 1, 0))
    pos = order[at] if len(ids) else np.zeros_like(sem)
    found = (ids[pos] == sem) & (sem != 0) if len(ids) else np.zeros(sem.shape, bool)
    return np.where(found, pos, -1).astype(np.int32)


def update_results_file(path, class_name, values, class_labels):
    """eval_scannet200.py:34-62, 139-148: replace the line of `path` that starts with "<class_name>," by the class's six
    values; a file that does not exist starts as the header and one `name,-,-,-` line per class.  Other lines stay."""
    if os.path.exists(path):
        with open(path, "r") as f:
            lines = f.readlines()
    else:
        lines = ["class,class id,ap,ap50,ap25,rc,rc50,rc25\n"] + [f"{c},-,-,-\n" for c in class_labels]
    new = ",".join([class_name] + [str(v) for v in values] + ["\n"])
    lines = [new if line.startswith(f"{class_name},") else line for line in lines]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.writelines(lines)


def final_file_predictions(result, scene_id, class_labels, n_points, device="cuda"):
    """One saved final file {"ins", "final_class", "conf"} -> (preds without masks, device bit rows), as
    eval_scannet200.py:106-133 reads it: "ins" dense rows (points equal to 1 are set) or RLE dicts, `final_class`
    label strings or a tensor of class positions, label_id = position + 1, and every confidence 1.0 (:130)."""
    category = result["final_class"]
    if torch.is_tensor(category):
        positions = [float(c) for c in category.reshape(-1).tolist()]
    else:
        index = {lab: i for i, lab in reversed(list(enumerate(class_labels)))}     # list.index: the first position
        positions = [float(index[c.lower()]) for c in category]
    preds = [{"scan_id": scene_id, "label_id": p + 1, "conf": 1.0} for p in positions]
    nw = (n_points + 63) // 64
    if not preds:
        return preds, torch.zeros((0, nw), dtype=torch.int64, device=device)
    ins = result["ins"]
    if isinstance(ins, (list, tuple)) and isinstance(ins[0], dict):
        from .scene import runs_from_rles
        if any(int(r["length"]) != n_points for r in ins):
            raise ValueError(f"{scene_id}: RLE masks of another length than the ground truth")
        rs, re, offs = runs_from_rles(ins, "final")
        t = lambda a: torch.from_numpy(a).to(device)
        return preds, _lib.rle_to_rows(t(rs), t(re), t(offs), n_points)
    ins = torch.as_tensor(ins).to(device)
    if ins.shape != (len(preds), n_points):
        raise ValueError(f"{scene_id}: masks of shape {tuple(ins.shape)} for {len(preds)} classes and {n_points} points")
    return preds, _lib.pack_rows((ins == 1).contiguous())
