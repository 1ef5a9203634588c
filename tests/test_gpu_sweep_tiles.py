"""The sweep's multi-frame tiles against the per-frame reference of tests/sweep_case.py, bit for bit.

One block of project_views_kernel visits a tile of up to 8 frames: the 8-frames-at-once culling ballot, the per-wave LDS
transposition slice reused from frame to frame, the per-slot mask tables of the look-up mode, the ragged last tile and the
counters summed across a tile only matter when that tile holds more than one frame.  The case has 33 blocks of points,
so the prefixes of its 1001 frames reach every tile size 1 ... 8 (asserted through bff_sweep_frames_per_block: if the
heuristic is retuned this module fails instead of quietly testing one frame per block).  Every mask source, every depth
form, with and without the culling table, for both word widths; plus bff_count_viewed on the same data."""
import faulthandler
import sys

import numpy as np
import pytest
import torch

import sweep_case as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = sc.N_POINTS
FILL, SENTINEL, TAIL = 7, -12345, 64
ITEM_LIMIT_S = 120                # a test item that is still running by then has hung: the process ends with a traceback

MASKS = ("words", "segmap", "labels", "lookup")
DEPTHS = ("f32", "u16rows", "u16tiles", "f32tiles")
FULL = [(wb, p, m, d, t) for wb in (32, 64) for p in (1001, 249) for m in MASKS for d in DEPTHS for t in (False, True)]
REST = [(wb, p, m, d, t) for wb in (32, 64) for p in sc.PREFIXES if p not in (1001, 249)
        for m, d, t in (("words", "f32", False), ("lookup", "f32tiles", True))]


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(ITEM_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


def to_dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


class Device:
    """Everything of the case that lives on the GPU, uploaded / decoded once per module."""

    def __init__(self, lib):
        self.lib = lib
        c = self.case = sc.get()
        soa = np.full((3, N + 3), np.nan)                            # n_pad need not be a multiple of anything
        soa[:, :N] = c.xyz.T
        self.xyz = to_dev(soa)
        self.inv_pose = to_dev(c.inv_pose.reshape(sc.N_FRAMES, 16))
        self.depth_index = to_dev(c.depth_index)
        self.flags = to_dev(c.frame_flags)
        raw = to_dev(c.depth_raw)
        self.depth = {"f32": (to_dev(c.depth_f32.reshape(sc.N_FRAMES, sc.HW)), None),
                      "u16rows": (raw, None),
                      "u16tiles": (lib.tile_depth(raw, metres=False), (sc.HS, sc.WS)),
                      "f32tiles": (lib.tile_depth(raw, metres=True), (sc.HS, sc.WS))}
        self.bounds = lib.point_tile_bounds(self.xyz, N)
        assert self.bounds.shape == ((N + 255) // 256, 6)
        self.sets = {wb: self.mask_set(c.sets[wb]) for wb in (32, 64)}
        self.viewed_at = {p: to_dev(v) for p, v in c.viewed_at.items()}
        torch.cuda.synchronize()

    def mask_set(self, s):
        lib, wb = self.lib, s.word_bits
        rs, re, offs, voffs = (to_dev(a, np.int32) for a in s.run_tables())
        nv, wdt = len(s.views), torch.int32 if wb == 32 else torch.int64
        words = torch.empty((nv, sc.HW), dtype=wdt, device=DEV)
        lib.rle_to_maskbits(rs, re, offs, voffs, nv, sc.HW, wb, words)
        sparse = torch.full_like(words, -1)                          # segments without a mask pixel keep the garbage
        seg = torch.empty((nv, lib.segmap_words(sc.HW)), dtype=torch.int32, device=DEV)
        lib.rle_to_maskbits(rs, re, offs, voffs, nv, sc.HW, wb, sparse, seg)
        lab = torch.full((nv, lib.label_plane_stride(sc.HW)), 0xEE, dtype=torch.uint8, device=DEV)
        ovf = torch.full_like(words, -1)
        seg2 = torch.empty((nv, 2 * lib.segmap_words(sc.HW)), dtype=torch.int32, device=DEV)
        lib.rle_to_labels(rs, re, offs, voffs, nv, sc.HW, wb, lab, ovf, seg2)
        tab, directory = lib.mask_row_directory(rs, re, offs, int(voffs[-1]), sc.H, sc.W)
        mw = s.chunk_mask.shape[1]
        assert mw == lib.load().bff_chunk_mask_words(sc.NW)
        return dict(s=s, wb=wb, runs=(rs, re, voffs), words=words, sparse=sparse, seg=seg, lab=lab, ovf=ovf, seg2=seg2, tab=tab,
                    directory=directory, frame_mask=to_dev(s.frame_mask), rowbase=to_dev(s.frame_rowbase),
                    nmask=to_dev(s.frame_nmask), exp_rows=to_dev(s.rows), exp_cmask=to_dev(s.chunk_mask),
                    masked_at={p: to_dev(v) for p, v in s.masked_at.items()},
                    rows=torch.empty((s.n_rows + 1, sc.NW), dtype=torch.int64, device=DEV),          # + one guard row
                    cmask=torch.empty((s.n_rows + 1, mw), dtype=torch.int64, device=DEV))

    def counters(self):
        buf = torch.full((N + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
        buf[:N] = FILL
        return buf

    def sweep(self, wb, p, masks, depth, table):
        """One sweep over the first p frames -> (rows, chunk_mask, masked, viewed) buffers, guards and tails included."""
        d, lib = self.sets[wb], self.lib
        n_rows = int(d["s"].rows_upto[p])
        rows, cmask = d["rows"].zero_(), d["cmask"].zero_()
        mc, vc = self.counters(), self.counters()
        dimg, dsize = self.depth[depth]
        head = (self.xyz, N, self.inv_pose[:p], sc.K, dimg, self.depth_index[:p], sc.H, sc.W, sc.THRESH)
        frames = (d["frame_mask"][:p], d["rowbase"][:p], d["nmask"][:p], self.flags[:p])
        out = (rows[:n_rows], mc[:N], vc[:N])
        kw = dict(chunk_mask=cmask[:n_rows], tile_bounds=self.bounds if table else None, depth_size=dsize)
        if masks == "lookup":
            rs, re, voffs = d["runs"]
            lib.project_views_lookup(*head, d["tab"], d["directory"], rs, re, voffs, wb, *frames, *out, **kw)
        elif masks == "words":
            lib.project_views(*head, d["words"], wb, *frames, *out, **kw)
        elif masks == "segmap":
            lib.project_views(*head, d["sparse"], wb, *frames, *out, segmap=d["seg"], **kw)
        else:
            lib.project_views(*head, d["ovf"], wb, *frames, *out, segmap=d["seg2"], labels=d["lab"], **kw)
        return rows, cmask, mc, vc

    def check(self, wb, p, got):
        """Every buffer of one sweep against the reference, exactly."""
        d = self.sets[wb]
        s = d["s"]
        n_rows = int(s.rows_upto[p])
        rows, cmask, mc, vc = got
        if not torch.equal(rows[:n_rows], d["exp_rows"][:n_rows]):
            bad = torch.nonzero((rows[:n_rows] != d["exp_rows"][:n_rows]).any(dim=1)).flatten().cpu().numpy()
            frames = np.unique(np.searchsorted(s.rows_upto, bad, side="right") - 1)
            raise AssertionError(f"rows: {bad.size} of {n_rows} rows differ, in {frames.size} frames, first frames {frames[:12].tolist()}")
        assert not rows[n_rows:].any(), "rows written past n_rows"
        assert torch.equal(cmask[:n_rows], d["exp_cmask"][:n_rows]), "chunk_mask"
        assert not cmask[n_rows:].any(), "chunk_mask written past n_rows"
        for name, buf, exp in (("masked_count", mc, d["masked_at"][p]), ("viewed_count", vc, self.viewed_at[p])):
            if not torch.equal(buf[:N], exp + FILL):
                bad = int((buf[:N] != exp + FILL).sum())
                raise AssertionError(f"{name}: {bad} of {N} points differ from fill + reference")
            assert (buf[N:] == SENTINEL).all(), f"{name} written past n_points"


@pytest.fixture(scope="module")
def dev():
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return Device(_lib)


def test_library_picks_every_tile_size(dev):
    got = [dev.lib.load().bff_sweep_frames_per_block(N, p) for p in sc.PREFIXES]
    assert got == list(sc.EXPECTED_FPB) == [sc.frames_per_block_formula(N, p) for p in sc.PREFIXES]


@pytest.mark.parametrize("wb,p,masks,depth,table", FULL + REST,
                         ids=[f"w{wb}-P{p}-{m}-{d}-{'table' if t else 'notable'}" for wb, p, m, d, t in FULL + REST])
def test_sweep_equals_per_frame_reference(dev, wb, p, masks, depth, table):
    assert dev.lib.load().bff_sweep_frames_per_block(N, p) == sc.EXPECTED_FPB[sc.PREFIXES.index(p)]
    dev.check(wb, p, dev.sweep(wb, p, masks, depth, table))


@pytest.mark.parametrize("wb,p,masks,depth,table", [(32, 1001, "lookup", "f32tiles", True), (64, 1001, "labels", "u16tiles", True),
                                                   (64, 249, "lookup", "u16rows", False), (32, 1000, "words", "f32", True)])
def test_two_runs_give_the_same_bytes(dev, wb, p, masks, depth, table):
    first = [t.clone() for t in dev.sweep(wb, p, masks, depth, table)]
    second = dev.sweep(wb, p, masks, depth, table)
    for a, b, what in zip(first, second, ("rows", "chunk_mask", "masked_count", "viewed_count")):
        assert torch.equal(a, b), what
    dev.check(wb, p, second)


@pytest.mark.parametrize("table", [False, True], ids=["notable", "table"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_count_viewed_equals_reference(dev, depth, table):
    """bff_count_viewed over the flagged frames of the whole list, for the library's frame tile and given ones."""
    sel = torch.nonzero(dev.flags & 1).flatten()
    pose, dindex = dev.inv_pose[sel].contiguous(), dev.depth_index[sel].contiguous()
    dimg, dsize = dev.depth[depth]
    exp = dev.viewed_at[sc.N_FRAMES] + FILL
    for fpb in (0, 1, 3, 8, 32):
        vc = dev.counters()
        dev.lib.count_viewed(dev.xyz, N, pose, sc.K, dimg, dindex, sc.H, sc.W, sc.THRESH, vc[:N],
                             tile_bounds=dev.bounds if table else None, depth_size=dsize, frames_per_block=fpb)
        assert torch.equal(vc[:N], exp), f"frames_per_block {fpb}: {int((vc[:N] != exp).sum())} points differ"
        assert (vc[N:] == SENTINEL).all(), f"frames_per_block {fpb}: written past n_points"
