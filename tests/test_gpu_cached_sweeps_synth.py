"""The cached sweeps and the pixel-sorted companion on visibility tables written in NumPy (tests/vis_table_synth.py), at the
sizes the geometric cases never reach: widths and pixel counts that divide nothing, rows of more than 256 chunks, a row of
exactly 64 KB of LDS and the refusal one point later, hundreds of pairs on one pixel, a sort key of all 32 bits.

Per case: bff_visibility_sorted equals visibility_sorted_ref.companion; bff_project_views_runs and bff_project_views_cached
equal vis_table_synth.table_sweep -- rows, chunk flags, both counters -- and each other, bit for bit; the guard row and
the counters' tails stay untouched.  The regime conditions of every case are asserted again here."""
import ctypes
import faulthandler
import sys

import numpy as np
import pytest
import torch

import test_gpu_visibility_table as vt
import vis_table_synth as vs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITEM_LIMIT_S = 120
FILL, SENTINEL, TAIL = 7, -12345, 64


def to_dev(a):
    a = np.ascontiguousarray(a)
    return vt.to_dev(a.view(np.int32) if a.dtype == np.uint32 else a)


CASE_SETS = [(name, wb) for name, c in vs.CASES.items() for wb in sorted(c["sets"])]


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(ITEM_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def lib():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return _lib


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Device:
    """One case on the device: the table, its companion, the frames, and per mask set the run tables and the directory."""

    def __init__(self, lib, case):
        self.case = case
        self.vis = tuple(to_dev(a) for a in case.table)
        self.sorted = lib.visibility_sorted(self.vis, case.pairs, case.n, case.h, case.w)
        self.depth_index, self.frame_mask = to_dev(case.depth_index), to_dev(case.frame_mask)
        self.flags = to_dev(case.frame_flags)
        self.sets = {}
        for wb in case.covers:
            rs, re, offs, voffs = (to_dev(a) for a in case.runs[wb])
            tab, directory = lib.mask_row_directory(rs, re, offs, int(case.runs[wb][3][-1]), case.h, case.w)
            rowbase, nmask = (to_dev(a) for a in case.layout(wb))
            self.sets[wb] = dict(rs=rs, re=re, offs=offs, voffs=voffs, tab=tab, directory=directory, rowbase=rowbase,
                                 nmask=nmask)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def on_device(lib):
    """name -> the case on the device, uploaded once per module and dropped with it."""
    resident = {}

    def get(name):
        if name not in resident:
            resident[name] = Device(lib, vs.get(name))
        return resident[name]
    yield get
    resident.clear()


def buffers(case, wb, rows_fill=0):
    """Rows and chunk flags with one guard row, counters of FILL with a SENTINEL tail."""
    n_rows = case.expected(wb)[0].shape[0]
    rows = torch.full((n_rows + 1, case.nw), rows_fill, dtype=torch.int64, device=DEV)
    cmask = torch.full((n_rows + 1, case.mw), rows_fill, dtype=torch.int64, device=DEV)
    counters = []
    for _ in range(2):
        buf = torch.full((case.n + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
        buf[:case.n] = FILL
        counters.append(buf)
    return n_rows, rows, cmask, counters[0], counters[1]


def sweep(lib, d, wb, form):
    case, s = d.case, d.sets[wb]
    n_rows, rows, cmask, mc, vc = buffers(case, wb)
    frames = (d.frame_mask, s["rowbase"], s["nmask"], d.flags)
    if form == "runs":
        lib.project_views_runs(case.n, d.depth_index, case.h, case.w, d.vis, d.sorted, s["rs"], s["re"], s["offs"], s["voffs"],
                               wb, *frames, rows[:n_rows], mc[:case.n], vc[:case.n], cmask[:n_rows])
    else:
        lib.project_views_cached(case.n, d.depth_index, case.h, case.w, d.vis, s["tab"], s["directory"], s["rs"], s["re"],
                                 s["voffs"], wb, *frames, rows[:n_rows], mc[:case.n], vc[:case.n], chunk_mask=cmask[:n_rows])
    torch.cuda.synchronize()
    return u64(rows), u64(cmask), mc.cpu().numpy(), vc.cpu().numpy()


def assert_sweep(case, wb, got, form):
    e_rows, e_cmask, e_masked, e_viewed = case.expected(wb)
    rows, cmask, mc, vc = got
    n, n_rows = case.n, e_rows.shape[0]
    bad = np.flatnonzero((rows[:n_rows] != e_rows).any(axis=1))
    assert bad.size == 0, f"{form}: rows {bad[:8].tolist()} differ, first at word {np.flatnonzero(rows[bad[0]] != e_rows[bad[0]])[:4].tolist()}"
    assert np.array_equal(cmask[:n_rows], e_cmask), f"{form}: chunk flags"
    assert not rows[n_rows:].any() and not cmask[n_rows:].any(), f"{form}: the guard row was written"
    assert np.array_equal(mc[:n], e_masked + FILL), f"{form}: masked_count"
    assert np.array_equal(vc[:n], e_viewed + FILL), f"{form}: viewed_count"
    assert (mc[n:] == SENTINEL).all() and (vc[n:] == SENTINEL).all(), f"{form}: a counter's tail was written"


@pytest.mark.parametrize("name", list(vs.CASES))
def test_companion_of_a_synthetic_table(lib, on_device, name):
    case = vs.get(name)
    vs.assert_regime(case)
    d = on_device(name)
    espix, espt, erow = case.companion()
    spix, spt, rowstart = (u32(t) for t in d.sorted)
    assert spix.shape == espix.shape and rowstart.shape == erow.shape
    assert np.array_equal(spix, espix), "pixels"
    assert np.array_equal(spt, espt), "points: equal pixels keep their ascending point order"
    assert np.array_equal(rowstart, erow), "row starts"
    assert lib.visibility_sorted_bytes(case.n_slots, case.h, case.pairs) == (espix.nbytes, espt.nbytes, erow.nbytes)


@pytest.mark.parametrize("name,wb", CASE_SETS, ids=[f"{n}-{wb}" for n, wb in CASE_SETS])
def test_cached_sweeps_of_a_synthetic_table(lib, on_device, name, wb):
    case = vs.get(name)
    vs.assert_regime(case)
    d = on_device(name)
    points = sweep(lib, d, wb, "points")
    assert_sweep(case, wb, points, "point-major")
    if name == "over":
        assert not lib.sweep_runs_ok(case.n) and lib.sweep_runs_ok(case.n - 1)
        n_rows, rows, cmask, mc, vc = buffers(case, wb, rows_fill=0x5a5a)
        s = d.sets[wb]
        with pytest.raises(RuntimeError, match="exceeds 64 KB of LDS"):
            lib.project_views_runs(case.n, d.depth_index, case.h, case.w, d.vis, d.sorted, s["rs"], s["re"], s["offs"],
                                   s["voffs"], wb, d.frame_mask, s["rowbase"], s["nmask"], d.flags, rows[:n_rows],
                                   mc[:case.n], vc[:case.n], cmask[:n_rows])
        torch.cuda.synchronize()
        assert (rows == 0x5a5a).all() and (cmask == 0x5a5a).all(), "the refused call wrote rows or flags"
        assert (mc[:case.n] == FILL).all() and (vc[:case.n] == FILL).all(), "the refused call counted"
        assert (mc[case.n:] == SENTINEL).all() and (vc[case.n:] == SENTINEL).all()
        return
    assert lib.sweep_runs_ok(case.n)
    runs = sweep(lib, d, wb, "runs")
    assert_sweep(case, wb, runs, "run-major")
    for a, b, what in zip(points, runs, ("rows", "chunk_mask", "masked", "viewed")):
        assert np.array_equal(a, b), f"{what}: the two forms differ"


def test_one_slot_more_than_the_sort_key_holds(lib):
    """key32 with S + 1 slots: slots x pixels pass 2^32, the companion is refused and nothing is written."""
    case = vs.get("key32")
    n_slots = case.n_slots + 1
    assert n_slots * case.h * case.w > 1 << 32
    mask, off, pix = case.table
    grow = lambda a: np.concatenate([a, np.full_like(a[:1], 0 if a is mask else case.pairs)])
    vis = tuple(to_dev(a) for a in (grow(mask), grow(off), pix))
    with pytest.raises(RuntimeError, match="exceed the 32-bit sort key"):
        lib.visibility_sorted(vis, case.pairs, case.n, case.h, case.w)
    # the entry point itself, on buffers of ours and with more scratch than the case below the bound asks for
    spix = torch.full((case.pairs,), SENTINEL, dtype=torch.int32, device=DEV)
    spt, rowstart = spix.clone(), torch.full((n_slots, case.h + 1), SENTINEL, dtype=torch.int32, device=DEV)
    temp = torch.full((1 << 22,), 0x5a, dtype=torch.uint8, device=DEV)
    need = ctypes.c_size_t(temp.numel())
    ptr = lib._ptr
    with pytest.raises(RuntimeError, match="exceed the 32-bit sort key"):
        lib.call("bff_visibility_sorted", ptr(vis[0]), ptr(vis[1]), ptr(vis[2]), case.pairs, case.n, n_slots, case.h, case.w,
                 ptr(spix), ptr(spt), ptr(rowstart), ptr(temp), ctypes.byref(need))
    torch.cuda.synchronize()
    assert (spix == SENTINEL).all() and (spt == SENTINEL).all() and (rowstart == SENTINEL).all() and (temp == 0x5a).all()
    assert need.value == temp.numel()
