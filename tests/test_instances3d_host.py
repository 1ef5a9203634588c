"""What the optional 3-D stages share (beyond_fixed_forms_amd/instances3d.py), as far as it runs without a GPU: the order
of the kept components against a literal sort over tuples, and the result the stages hand back."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from beyond_fixed_forms_amd import instances3d as i3


def order_ref(offs, elem, pts, mode):
    """(parent row, points descending, anchor) by Python's sorted; "largest": the first of every parent."""
    par = [max(k for k in range(len(offs) - 1) if offs[k] <= e) for e in elem]
    order = sorted(range(len(elem)), key=lambda i: (par[i], -pts[i], elem[i]))
    if mode == "largest":
        order = [i for n, i in enumerate(order) if n == 0 or par[i] != par[order[n - 1]]]
    return order, par


KEPT = {
    # rows of 4, 0, 5 and 3 elements; the kept list in the order a run might leave it in
    "ties in points go to the smaller anchor": ([0, 4, 4, 9, 12], [11, 2, 9, 0, 3, 5], [7, 7, 3, 7, 9, 7]),
    "parents interleaved": ([0, 4, 4, 9, 12], [10, 1, 6, 0, 11, 4, 8, 3], [1, 5, 2, 5, 8, 9, 2, 6]),
    "a row's last and the next row's first element": ([0, 4, 4, 9, 12], [4, 3, 8, 9], [1, 2, 3, 4]),
    "empty": ([0, 4, 4, 9, 12], [], []),
    "single": ([0, 4, 4, 9, 12], [5], [40]),
}


@pytest.mark.parametrize("mode", ["split", "largest"])
@pytest.mark.parametrize("case", list(KEPT))
def test_kept_order_is_the_literal_sort(case, mode):
    offs, elem, pts = (np.array(a, dtype=np.int64) for a in KEPT[case])
    order, par = i3.kept_order(offs, elem, pts, mode)
    exp_order, exp_par = order_ref(offs.tolist(), elem.tolist(), pts.tolist(), mode)
    assert order.tolist() == exp_order and par.tolist() == exp_par
    if mode == "largest":
        assert len(order) == len(set(exp_par))


def test_kept_order_hand_case():
    offs = np.array([0, 4, 4, 9, 12])
    elem, pts = np.array([11, 2, 9, 0, 3, 5]), np.array([7, 7, 3, 7, 9, 7])
    order, par = i3.kept_order(offs, elem, pts, "split")
    assert par.tolist() == [3, 0, 3, 0, 0, 2]
    assert elem[order].tolist() == [3, 0, 2, 5, 11, 9]                      # row 0: 9 points, then 7 and 7 by anchor
    assert elem[i3.kept_order(offs, elem, pts, "largest")[0]].tolist() == [3, 5, 11]


@dataclasses.dataclass
class Result:
    rows: object
    conf: object
    final_class: list
    n_points: int = 100
    conf_host: object = None
    prefetch: object = None


PARENT = torch.tensor([2, 0, 2], dtype=torch.int64)


@pytest.mark.parametrize("conf", [[0.5, 0.25, 0.125], (0.5, 0.25, 0.125), torch.tensor([0.5, 0.25, 0.125], dtype=torch.float16),
                                  np.array([0.5, 0.25, 0.125], dtype=np.float32)], ids=["list", "tuple", "tensor", "ndarray"])
def test_replace_rows_keeps_the_kind_and_dtype_of_conf(conf):
    res = Result("old", conf, ["a", "b", "c"], conf_host=conf, prefetch=object())
    new = i3.replace_rows(res, "new", PARENT)
    assert new is not res and type(new) is Result and new.rows == "new" and res.rows == "old"
    assert new.final_class == ["c", "a", "c"] and new.parent is PARENT
    for got in (new.conf, new.conf_host):
        assert type(got) is type(conf) and getattr(got, "dtype", None) == getattr(conf, "dtype", None)
        assert [float(x) for x in got] == [0.125, 0.5, 0.125]
    assert new.prefetch is None and res.prefetch is not None                # the inputs of the replaced rows: dropped
    assert new.n_points == 100                                              # no new length was given


def test_replace_rows_without_rows_parent_or_length():
    res = Result(None, [0.5], ["a"])
    assert i3.replace_rows(res, None, PARENT) is res                        # nothing to replace: the object itself
    new = i3.replace_rows(res, "new", n_points=700)                         # the lift: rows and length, no parent
    assert (new.rows, new.n_points, new.conf, new.final_class) == ("new", 700, [0.5], ["a"]) and not hasattr(new, "parent")
    assert new.conf_host is None and res.n_points == 100
    saved = SimpleNamespace(rows="old", conf=[0.5], final_class=["a"])      # a saved file's namespace has no n_points
    new = i3.replace_rows(saved, "new", n_points=700)
    assert new.rows == "new" and not hasattr(new, "n_points") and not hasattr(new, "prefetch")
