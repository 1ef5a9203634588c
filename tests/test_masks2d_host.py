"""Host side of the dense-mask encoder (beyond_fixed_forms_amd/masks2d.py): the run-table <-> RLE conversion against
the oracle's rle_encode_batch, and the frame bookkeeping on entries that only have a len().  No GPU."""
import numpy as np
import pytest
import torch

from oracle import rle_ref


def edge_rows(n, seed):
    """The row set of test_rows_to_rle_matches_reference_encoder: empty, full, p < 0.5, sparse with both ends set, dense
    with holes, blocks of 37, even pixels, odd pixels."""
    rng = np.random.default_rng(seed)
    d = np.stack([rng.random(n) < p for p in (0.0, 1.0, 0.5, 0.02, 0.98)] +
                 [np.repeat(rng.random(n // 37 + 1) < 0.5, 37)[:n], np.arange(n) % 2 == 0, np.arange(n) % 2 == 1])
    d[3, 0] = d[3, -1] = True
    return d


def runs_of(d):
    """Dense bool rows -> (start, end, offs) by the definition: maximal runs of set pixels, [start, end)."""
    st, en, offs = [], [], [0]
    for row in d:
        p = np.concatenate([[False], row, [False]])
        edges = np.flatnonzero(p[1:] != p[:-1])
        st.append(edges[0::2]); en.append(edges[1::2])
        offs.append(offs[-1] + edges.size // 2)
    return np.concatenate(st).astype(np.int32), np.concatenate(en).astype(np.int32), np.asarray(offs, np.int32)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 10_001])
def test_runs_to_rles_matches_the_reference_encoder_and_inverts_runs_from_rles(n):
    from beyond_fixed_forms_amd.masks2d import runs_to_rles
    from beyond_fixed_forms_amd.scene import runs_from_rles
    d = edge_rows(n, n)
    st, en, offs = runs_of(d)
    got = runs_to_rles(st, en, offs, n)
    exp = rle_ref.rle_encode_batch_ref(torch.from_numpy(d))
    assert len(got) == len(exp) == d.shape[0]
    for g, e in zip(got, exp):
        assert g["length"] == e["length"] == n
        assert g["counts"].dtype == e["counts"].dtype == np.int64 and np.array_equal(g["counts"], e["counts"])
    back = runs_from_rles(got)
    for a, b in zip(back, (st, en, offs)):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    # and the other way round: runs_from_rles of the reference's output -> runs_to_rles gives it back
    again = runs_to_rles(*runs_from_rles(exp), n)
    assert all(np.array_equal(a["counts"], e["counts"]) for a, e in zip(again, exp))


def test_runs_to_rles_with_absolute_offsets_and_no_masks():
    """A frame's view of shared tables: offsets that do not start at 0 address the shared arrays; the arrays each mask
    gets are its own copies."""
    from beyond_fixed_forms_amd.masks2d import runs_to_rles
    d = edge_rows(130, 3)
    st, en, offs = runs_of(d)
    exp = rle_ref.rle_encode_batch_ref(torch.from_numpy(d))
    part = runs_to_rles(st, en, offs[3:7], 130)
    assert len(part) == 3 and all(np.array_equal(g["counts"], e["counts"]) for g, e in zip(part, exp[3:6]))
    part[0]["counts"][:] = -1
    assert np.array_equal(runs_to_rles(st, en, offs[3:7], 130)[0]["counts"], exp[3]["counts"])
    assert runs_to_rles(st[:0], en[:0], np.zeros(1, np.int32), 130) == []
    none = runs_to_rles(st[:0], en[:0], np.zeros(3, np.int32), 130)
    assert len(none) == 2 and all(r["counts"].size == 0 and r["counts"].dtype == np.int64 for r in none)


class OnlyLen:
    """Stands for a dense tensor / DeviceRuns as far as the frame bookkeeping goes: it has a length and nothing else."""

    def __init__(self, m):
        self.m = m

    def __len__(self):
        return self.m


def entry(fid, masks, m):
    return {"frame_id": f"{fid}.jpg", "segmented_frame_masks": masks, "confidences": torch.zeros(m, dtype=torch.float16),
            "labels": ["table"] * m}


def test_frame_table_and_word_bits_take_the_mask_count_from_len():
    from beyond_fixed_forms_amd.scene import class_word_bits, frame_table, masks_all_rle, slots_on_first_use
    rle = lambda m: [dict(length=12, counts=np.array([1, 2]))] * m
    for counts in ([3, 0, 32], [3, 33], [70, 5, 0]):
        stub = [entry(10 * i, OnlyLen(m), m) for i, m in enumerate(counts)]
        twin = [entry(10 * i, rle(m), m) for i, m in enumerate(counts)]
        assert class_word_bits(stub) == class_word_bits(twin) == (32 if max(counts) <= 32 else 64)
        wb = class_word_bits(stub)
        a = frame_table(stub, wb, slots_on_first_use()[0], viewed=["0", "10", "40"])
        b = frame_table(twin, wb, slots_on_first_use()[0], viewed=["0", "10", "40"])
        for x, y in zip(a.int_tables(), b.int_tables()):
            assert np.array_equal(x, y)
        assert (a.frame_ids, a.n_rows, a.n_mask_frames, a.labels) == (b.frame_ids, b.n_rows, b.n_mask_frames, b.labels)
        assert a.n_rows == sum(counts) and a.rles == [] and len(b.rles) == sum(counts)
        assert [len(e) for e in a.mask_entries] == counts and all(isinstance(e, OnlyLen) for e in a.mask_entries)
        assert masks_all_rle(b) and not masks_all_rle(a)
    # 70 masks with 64-bit words: two mask-views (64 + 6); an entry without masks makes no kernel frame
    ft = frame_table([entry(0, OnlyLen(70), 70), entry(10, OnlyLen(0), 0)], 64, slots_on_first_use()[0])
    assert ft.frame_nmask == [64, 6] and ft.frame_ids == ["0", "0"] and ft.view_mask_offs == [0, 64, 70]
    with pytest.raises(ValueError, match="differ in length"):
        frame_table([entry(0, OnlyLen(3), 2)], 32, slots_on_first_use()[0])


def test_run_tables_without_a_gpu():
    """RLE lists take the host path as before (also on a CPU device); dense masks have no CPU encoder and say so; a
    dense entry of another size is refused with the RLE path's message."""
    from beyond_fixed_forms_amd.scene import frame_table, run_tables, runs_from_rles, slots_on_first_use
    d = edge_rows(6 * 9, 1)
    rles = rle_ref.rle_encode_batch_ref(torch.from_numpy(d))
    cpu = torch.device("cpu")
    ft = frame_table([entry(0, rles[:5], 5), entry(10, [], 0), entry(20, rles[5:], 3)], 32, slots_on_first_use()[0])
    got = run_tables(ft, 6, 9, cpu)
    for g, e in zip(got, runs_from_rles(rles)):
        assert g.dtype == torch.int32 and np.array_equal(g.numpy(), e)
    with pytest.raises(ValueError, match=r"mask RLE length 54 != H\*W = 48"):
        run_tables(ft, 6, 8, cpu)
    dense = torch.from_numpy(d).view(8, 1, 6, 9)
    ftd = frame_table([entry(0, dense, 8)], 32, slots_on_first_use()[0])
    with pytest.raises(ValueError, match=r"mask RLE length 54 != H\*W = 48"):
        run_tables(ftd, 6, 8, cpu)
    with pytest.raises(ValueError, match="GPU"):
        run_tables(ftd, 6, 9, cpu)


def test_tile_size_constant_matches_the_library():
    from beyond_fixed_forms_amd import _lib, masks2d
    assert _lib.load().bff_masks2d_tile_pixels() == masks2d.TILE_PIXELS
    assert masks2d.TILE_PIXELS % 1024 == 0


def test_entry_points_reject_bad_arguments():
    from beyond_fixed_forms_amd import _lib
    lib = _lib.load()
    assert lib.bff_masks2d_count(None, -1, 10, None, None, None) == -1 and b"bad sizes" in lib.bff_last_error()
    assert lib.bff_masks2d_count(None, 1, 1 << 31, None, None, None) == -2 and b"2^31" in lib.bff_last_error()
    assert lib.bff_masks2d_count(None, 1, 10, None, None, None) == -1 and b"null" in lib.bff_last_error()
    assert lib.bff_masks2d_count(None, 0, 10, None, None, None) == 0
    assert lib.bff_masks2d_runs(None, 3, -1, None, None, None, None) == -1 and b"bad sizes" in lib.bff_last_error()
    assert lib.bff_masks2d_runs(None, 3, 10, None, None, None, None) == -1 and b"null" in lib.bff_last_error()
    assert lib.bff_masks2d_runs(None, 0, 10, None, None, None, None) == 0
    assert lib.bff_masks2d_runs(None, 3, 0, None, None, None, None) == 0
