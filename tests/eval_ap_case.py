"""tests/golden/eval_ap.npz (written by scripts/make_golden_eval_ap.py from the reference's own evaluator) -> cases, and
the error bounds the tests hold the scores to.  Shared by the host and the GPU evaluation tests."""
from __future__ import annotations

import functools
import os

import numpy as np

import golden_io as gio

ALL_KEYS = ("all_ap", "all_ap_50%", "all_ap_25%", "all_rc", "all_rc_50%", "all_rc_25%")
CASES = ("labelled", "agnostic", "hand")
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(gio.GOLDEN_DIR, "eval_ap.npz"))


def class_labels():
    return [str(s) for s in fixture()["class_labels"]]


def scans(name, conf_one=False):
    """-> (use_label, [(sem, ins, preds)]) of one case; conf_one: the variant with every confidence 1.0."""
    z = fixture()
    out = []
    for i in range(int(z[f"{name}.n_scans"])):
        sem, ins = z[f"{name}.{i}.sem"], z[f"{name}.{i}.ins"]
        masks = np.unpackbits(z[f"{name}.{i}.pred_masks"], axis=-1, count=sem.shape[0], bitorder="little")
        preds = [{"scan_id": str(s), "label_id": float(l), "conf": 1.0 if conf_one else float(c), "pred_mask": m}
                 for s, l, c, m in zip(z[f"{name}.{i}.pred_scan"], z[f"{name}.{i}.pred_label"], z[f"{name}.{i}.pred_conf"], masks)]
        out.append((sem, ins, preds))
    return bool(z[f"{name}.use_label"]), out


def expected(name, conf_one=False):
    """-> (ap, rc, the six all_* values) the reference computed."""
    z, tag = fixture(), ".conf1" if conf_one else ""
    return z[f"{name}{tag}.ap"], z[f"{name}{tag}.rc"], z[f"{name}{tag}.all"]


def assert_scores(name, conf_one, ap, rc, avgs):
    """NaN positions and recall are exact (recall is one float64 division of integers).  An AP is np.dot of k
    non-negative terms, each at most its step width, the widths summing to at most 1: whatever order BLAS adds them in,
    the sums differ by at most k * 2^-52, k_max the longest curve of the case.  A mean over L labels adds L * 2^-52."""
    e_ap, e_rc, e_all = expected(name, conf_one)
    tol = int(fixture()[f"{name}.k_max"]) * EPS
    assert ap.shape == e_ap.shape and ap.dtype == np.float64 and rc.dtype == np.float64
    assert np.array_equal(np.isnan(ap), np.isnan(e_ap))
    assert np.array_equal(rc, e_rc, equal_nan=True)
    ok = ~np.isnan(e_ap)
    assert np.all(np.abs(ap[ok] - e_ap[ok]) <= tol), np.abs(ap[ok] - e_ap[ok]).max()
    tol_mean = tol + ap.shape[1] * EPS
    for key, e in zip(ALL_KEYS, e_all):
        assert abs(avgs[key] - e) <= tol_mean, (key, avgs[key], e)
