"""Generate tests/golden/eval_ap.npz from the REAL reference evaluator.  TEST INFRASTRUCTURE ONLY.

Run where the reference tree is present:   python scripts/make_golden_eval_ap.py

The reference's own ScanNetEval.assign_instances_for_scan, evaluate_matches, compute_averages, write_result_file and
print_results (evaluation/eval/scannetv2_inst_eval.py, imported by oracle.make_golden_eval.load_reference_evaluator) run
on seeded synthetic scans; only their inputs and results are stored.  The ground truth of a scan is oracle's
`make_case`; the predictions are made here, each labelled after the instance it covers (with labels drawn
independently, as make_case draws them, 190 of 198 labels come out NaN and 4 distinct AP values are left).  Every branch
of evaluate_matches the fixture is meant to pin is asserted below on the reference's output, so the fixture cannot go
vacuous unnoticed.  The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden_eval import load_reference_evaluator, make_case  # noqa: E402

ENCODE, MIN_REGION = 1000, 100
UNPREDICTED = 198                 # a label that has ground truth and never a prediction: AP 0
NO_GT_LABEL = 50                  # a label that has predictions and never ground truth: NaN


def instances_of(sem, ins):
    """The evaluator's view of make_case's ground truth: {encoded id: (label id, point indices)}, label 0 = clamped."""
    s = sem.astype(np.int64) - 1
    s[s < 0] = 0
    g = s * ENCODE + ins.astype(np.int64) + 1
    g[ins + 1 < 0] = 0
    return g, {int(i): (int(i) // ENCODE, np.flatnonzero(g == i)) for i in np.unique(g) if i != 0}


def mask_of(n, *index_sets):
    m = np.zeros(n, np.uint8)
    for idx in index_sets:
        m[idx] = 1
    return m


def labelled_scan(seed, n, scan_id, specials):
    """Ground truth of make_case(seed, n) and predictions with IoUs spread over 0.25 .. 1 against instances of their
    own label, confidences on a grid of tenths (ties); `specials` adds one prediction per branch named in main()."""
    sem, ins, _ = make_case(seed, n, 0, True)
    rng = np.random.default_rng(1000 + seed)
    g, inst = instances_of(sem, ins)
    valid = {i: v for i, v in inst.items() if 1 <= v[0] <= 198}
    big = {i: v for i, v in valid.items() if len(v[1]) >= MIN_REGION}
    preds = []

    def add(mask, label, conf=None):
        preds.append({"scan_id": scan_id, "label_id": float(label), "pred_mask": mask,
                      "conf": float(np.round(rng.random(), 1)) if conf is None else conf})

    def elsewhere(label, count):
        """Points of large instances of other valid labels: neither void nor ground truth of `label`."""
        pool = np.concatenate([v[1] for v in big.values() if v[0] != label])
        return rng.choice(pool, count, replace=False)

    for i, (label, idx) in big.items():
        if label == UNPREDICTED or rng.random() < 0.2:
            continue
        part = idx[rng.random(len(idx)) < rng.uniform(0.3, 1.0)]
        noise = elsewhere(label, int(rng.uniform(0.0, 0.6) * len(idx)))
        add(mask_of(n, part, noise), label)
    if specials:
        by_label = {}
        for i, (label, idx) in big.items():
            if label != UNPREDICTED:
                by_label.setdefault(label, []).append(idx)
        # two predictions over threshold on one ground-truth instance
        label, idx = next(v for v in big.values() if v[0] != UNPREDICTED)
        add(mask_of(n, idx), label)
        add(mask_of(n, idx[: int(0.95 * len(idx))]), label)
        # one prediction covering two instances of one label, of sizes within 1 : 2 (both IoUs > 0.25)
        a, b = next((x, y) for lst in by_label.values() for x in lst for y in lst
                    if x is not y and len(x) <= len(y) <= 2 * len(x))
        add(mask_of(n, a, b), next(l for l, lst in by_label.items() if any(x is a for x in lst)))
        some = next(iter(by_label))
        # unmatched, mostly on an ignored instance (instance id -2: its points are encoded 0)
        ignored = np.flatnonzero(ins == -2)
        add(mask_of(n, ignored[:300], elsewhere(some, 40)), some)
        # unmatched, mostly on a class that is not a valid one
        void = np.flatnonzero(sem == 250)
        add(mask_of(n, void[:250], elsewhere(some, 30)), some)
        # unmatched at 0.5 (IoU just below it), more than half on a ground-truth instance below the minimum region size
        label, idx = next(v for v in valid.values() if 70 <= len(v[1]) < MIN_REGION and v[0] in by_label)
        add(mask_of(n, idx[:-5], elsewhere(label, len(idx) - 8)), label)
        # unmatched and staying a false positive: only points of other labels' instances
        add(mask_of(n, elsewhere(some, 400)), some)
        # predictions of a label without ground truth, and of a label the evaluator does not know
        add(mask_of(n, elsewhere(NO_GT_LABEL, 300)), NO_GT_LABEL)
        add(mask_of(n, elsewhere(some, 300)), 400)
    return sem, ins, preds


def hand_scan(confs):
    """One ground-truth instance of 200 points (label 1), everything else of a clamped class; two predictions of
    IoU 1 and 0.975 with it."""
    n = 400
    sem = np.zeros(n, np.int32)
    ins = np.zeros(n, np.int32)
    sem[:200], ins[:200] = 2, 5
    masks = [mask_of(n, np.arange(200)), mask_of(n, np.arange(195))]
    return sem, ins, [{"scan_id": "hand_00", "label_id": 1.0, "conf": c, "pred_mask": m} for c, m in zip(confs, masks)]


@contextlib.contextmanager
def recorded_curve_lengths(out):
    """evaluate_matches integrates each curve with one np.dot(precision, stepWidths): note the lengths."""
    real = np.dot

    def dot(a, b):
        out.append(len(a))
        return real(a, b)
    np.dot = dot
    try:
        yield
    finally:
        np.dot = real


def run_reference(ScanNetEval, labels, scans, use_label, all_conf_one):
    ev = ScanNetEval(labels, use_label=use_label, dataset_name="scannet200")
    matches = {}
    for i, (sem, ins, preds) in enumerate(scans):
        preds = [dict(p, conf=1.0) for p in preds] if all_conf_one else preds
        gt2pred, pred2gt = ev.assign_instances_for_scan(preds, sem.copy(), ins.copy())
        matches[f"gt_{i}"] = {"gt": gt2pred, "pred": pred2gt}
    lengths = []
    with recorded_curve_lengths(lengths):
        ap, rc = ev.evaluate_matches(matches)
    avgs = ev.compute_averages(ap, rc)
    return ev, matches, ap, rc, avgs, max(lengths, default=1)


ALL_KEYS = ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%")


def check_labelled(matches, ap, rc, labels):
    """The branches of evaluate_matches this case has to reach, asserted on what the reference returned."""
    preds = [p for m in matches.values() for lst in m["pred"].values() for p in lst]
    gts = [g for m in matches.values() for lst in m["gt"].values() for g in lst]
    has_gt = lambda lab: any(g["vert_count"] >= MIN_REGION for m in matches.values() for g in m["gt"][lab])
    assert len(matches) >= 3 and any(not any(m["pred"].values()) for m in matches.values())
    li = UNPREDICTED - 1
    assert has_gt(labels[li]) and np.all(ap[0, li] == 0) and np.all(rc[0, li] == 0)
    li = NO_GT_LABEL - 1
    assert any(m["pred"][labels[li]] for m in matches.values()) and np.all(np.isnan(ap[0, li]))
    finite = ap[0][~np.isnan(ap[0]).any(axis=1)]
    inner = np.unique(finite[(finite > 0) & (finite < 1)])
    assert finite.shape[0] >= 8 and inner.size >= 12, (finite.shape, inner.size)
    ious = np.asarray([g["iou"] for p in preds for g in p["matched_gt"]])
    assert all(((ious > lo) & (ious <= lo + 0.15)).any() for lo in (0.25, 0.4, 0.55, 0.7, 0.85))
    assert any(sum(p["iou"] > 0.9 for p in g["matched_pred"]) >= 2 for g in gts)
    assert any(sum(g["iou"] > 0.25 and g["vert_count"] >= MIN_REGION for g in p["matched_gt"]) >= 2 for p in preds)
    unmatched = [p for p in preds if has_gt(labels[int(p["label_id"]) - 1]) and not any(g["iou"] > 0.5 for g in p["matched_gt"])]
    small = lambda p: sum(g["intersection"] for g in p["matched_gt"] if g["vert_count"] < MIN_REGION)
    assert sum(p["void_intersection"] / p["vert_count"] > 0.5 for p in unmatched) >= 2          # ignored instance, void class
    assert any(p["void_intersection"] / p["vert_count"] <= 0.5 < (p["void_intersection"] + small(p)) / p["vert_count"]
               for p in unmatched)
    assert any((p["void_intersection"] + small(p)) / p["vert_count"] <= 0.25 and not any(g["iou"] > 0.25 for g in p["matched_gt"])
               for p in unmatched)
    confs = [p["confidence"] for p in preds]
    assert len(set(confs)) < len(confs)
    names = [p["filename"] for p in preds]
    assert len(set(names)) < len(names)                   # two scans under one scan id share pred_visited entries


def write_npz(path, arrays):
    """np.savez_compressed with the zip's timestamps fixed, so that the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ScanNetEval, labels = load_reference_evaluator()
    out = {"class_labels": np.asarray(labels, dtype=str)}
    same_id = "scene0011_00"
    cases = {
        "labelled": (True, [labelled_scan(11, 12_000, same_id, True), labelled_scan(12, 7_001, "scene0012_00", False),
                            make_case(13, 3_000, 0, True), labelled_scan(14, 5_003, same_id, False)]),
        "agnostic": (False, [make_case(21, 6_007, 18, False), make_case(22, 4_000, 12, False)]),
        "hand": (True, [hand_scan((0.9, 0.4))]),
    }
    for name, (use_label, scans) in cases.items():
        out[f"{name}.use_label"] = np.array(use_label)
        out[f"{name}.n_scans"] = np.array(len(scans))
        for i, (sem, ins, preds) in enumerate(scans):
            n = sem.shape[0]
            out[f"{name}.{i}.sem"], out[f"{name}.{i}.ins"] = sem, ins
            out[f"{name}.{i}.pred_label"] = np.asarray([p["label_id"] for p in preds], dtype=np.float64)
            out[f"{name}.{i}.pred_conf"] = np.asarray([p["conf"] for p in preds], dtype=np.float64)
            out[f"{name}.{i}.pred_scan"] = np.asarray([p["scan_id"] for p in preds], dtype=str)
            out[f"{name}.{i}.pred_masks"] = np.packbits(np.stack([p["pred_mask"] != 0 for p in preds]), axis=-1, bitorder="little") \
                if preds else np.zeros((0, (n + 7) // 8), np.uint8)
        k_max = 1
        for tag, one in (("", False), (".conf1", True)):
            ev, matches, ap, rc, avgs, k = run_reference(ScanNetEval, labels, scans, use_label, one)
            k_max = max(k_max, k)
            out[f"{name}{tag}.ap"], out[f"{name}{tag}.rc"] = ap, rc
            out[f"{name}{tag}.all"] = np.asarray([avgs[key] for key in ALL_KEYS], dtype=np.float64)
            if name == "labelled" and not one:
                check_labelled(matches, ap, rc, labels)
            if name == "hand":
                # derived by hand: confidences 0.9 / 0.4 -> precision [0.5, 1, 1], recall [1, 1, 0], steps [0, 0.5, 0.5]:
                # AP 1.0; both 1.0 -> precision [0.5, 1], recall [1, 0], steps [0.5, 0.5]: AP 0.75; recall 1 in both
                assert np.all(ap[0, 0] == (0.75 if one else 1.0)) and np.all(rc[0, 0] == 1.0), (ap[0, 0], rc[0, 0])
            if not one:
                with tempfile.TemporaryDirectory() as tmp:
                    ev.write_result_file(avgs, os.path.join(tmp, "result.txt"))
                    with open(os.path.join(tmp, "result.txt")) as f:
                        out[f"{name}.result_txt"] = np.array(f.read())
                printed = io.StringIO()
                with contextlib.redirect_stdout(printed):
                    ev.print_results(avgs)
                out[f"{name}.print_txt"] = np.array(printed.getvalue())
            n_nan = int(np.isnan(ap[0]).any(axis=1).sum())
            print(f"  {name}{tag}: {len(scans)} scans, {sum(len(s[2]) for s in scans)} predictions, {n_nan} NaN labels, "
                  f"{np.unique(ap[~np.isnan(ap)]).size} distinct AP values, longest curve {k}, all_ap {avgs['all_ap']:.4f}")
        out[f"{name}.k_max"] = np.array(k_max)
    out["cases"] = np.asarray(list(cases), dtype=str)
    path = os.path.join(ROOT, "tests", "golden", "eval_ap.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
