"""pipeline.pipelined, the schedule every pipelined caller relies on: with recording halves, the order of the fronts and
backs, the number of items in flight, the distance between back(i) and front(i + depth) -- what makes the reuse of
workspace i % depth safe -- the meaning of depth None / <= 0, and where an exception in a back half leaves the fronts."""
import pytest

from beyond_fixed_forms_amd import pipeline

NS = [0, 1, 3, 4, 5, 13]
DEPTHS = [None, 0, 1, 2, 4, 7]


def effective(depth):
    return pipeline.PIPELINE_DEPTH if depth is None else max(1, depth)


def record(n, depth, fail_at=None):
    """Run pipelined(n, front, back, depth) with halves that log ("front", i), ("back", i) on entry and ("done", i) when
    back(i) returns; back(fail_at) raises.  -> (log, results, the exception or None)."""
    log = []

    def front(i):
        log.append(("front", i))
        return ("handle", i)

    def back(i, h):
        log.append(("back", i))
        assert h == ("handle", i)                 # the handle of front(i), not a neighbour's
        if i == fail_at:
            raise KeyError(i)
        log.append(("done", i))
        return 10 * i

    out, err = [], None
    try:
        for r in pipeline.pipelined(n, front, back, depth):
            out.append(r)
    except KeyError as e:
        err = e
    return log, out, err


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", NS)
def test_schedule(n, depth):
    d = effective(depth)
    log, out, err = record(n, depth)
    assert err is None and out == [10 * i for i in range(n)]
    assert [i for what, i in log if what == "front"] == list(range(n))          # fronts in index order, each once
    assert [i for what, i in log if what == "back"] == list(range(n))           # backs too
    issued = done = 0
    most = 0
    for what, i in log:
        if what == "front":
            # front(i) starts only after back(i - depth) has returned: workspace i % depth is free again
            assert i - d < 0 or done > i - d, (n, depth, i)
            issued += 1
        elif what == "back":
            assert issued > i                                                   # never a back before its own front
        else:
            done += 1
        most = max(most, issued - done)
        assert issued - done <= d
    assert most == min(n, d)                                                    # ... and the depth is really used


def test_depth_defaults():
    """None means PIPELINE_DEPTH, anything <= 0 means one item at a time."""
    n = pipeline.PIPELINE_DEPTH + 3
    assert record(n, None)[0] == record(n, pipeline.PIPELINE_DEPTH)[0]
    assert record(n, 0)[0] == record(n, 1)[0] == record(n, -3)[0]
    one = record(3, 1)[0]
    assert one == [(w, i) for i in range(3) for w in ("front", "back", "done")]
    if pipeline.PIPELINE_DEPTH > 1:
        assert record(n, None)[0] != record(n, 1)[0]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 13])
def test_exception_in_a_back_half(n, depth):
    """back(j) raises: the exception reaches the caller after exactly the fronts 0 .. j + depth - 1 (those of them
    that exist), the results before j were delivered, and nothing runs afterwards."""
    d = effective(depth)
    for j in sorted({0, n // 2, n - 1}):
        log, out, err = record(n, depth, fail_at=j)
        assert isinstance(err, KeyError) and err.args == (j,)
        assert out == [10 * i for i in range(j)]
        assert [i for what, i in log if what == "front"] == list(range(min(n, j + d)))
        assert [i for what, i in log if what == "back"] == list(range(j + 1))
        assert log[-1] == ("back", j)
