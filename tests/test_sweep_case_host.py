"""The multi-frame-tile case of tests/sweep_case.py, checked on the host: the reference alone has to meet the conditions
without which the GPU comparison (tests/test_gpu_sweep_tiles.py) would pass vacuously -- something visible in every
frame, points behind the camera that pass the depth test, culling that both skips and keeps at every slot of a frame
tile, both forms of label-plane segment, frames without masks / without the flag at every slot, a wave that stores rows
for two frames of one tile."""
import re
import os

import numpy as np
import pytest

import sweep_case as sc


@pytest.fixture(scope="module")
def case():
    return sc.get()


def test_sizes_and_prefixes():
    assert sc.N_POINTS == 33 * 1024 - 324 and (sc.N_POINTS + 1023) // 1024 == 33 and sc.NW == 523 and sc.NW % 4 != 0
    assert sc.N_POINTS % 1024 % 256 != 0 and sc.N_POINTS % 1024 < 768         # a ragged wave and an empty one in the last block
    assert [sc.frames_per_block_formula(sc.N_POINTS, p) for p in sc.PREFIXES] == list(sc.EXPECTED_FPB) == [1, 2, 3, 4, 5, 6, 7, 8, 8]
    # every length up to 869 leaves a last tile of one frame, 1000 is a whole number of tiles, 1001 leaves one frame over
    assert [p % k for p, k in zip(sc.PREFIXES, sc.EXPECTED_FPB)] == [0, 1, 1, 1, 1, 1, 1, 0, 1]
    assert all(f % 8 != 0 and 0 <= f < sc.N_FRAMES for f in sc.NEAR) and len(sc.NEAR) == 6


def test_formula_is_the_one_in_the_header():
    header = open(os.path.join(sc.ROOT, "include", "bff_hip.h")).read()
    assert re.search(r"int32_t bff_sweep_frames_per_block\(int64_t n_points, int32_t n_frames\);", header)
    from beyond_fixed_forms_amd import _lib
    assert "bff_sweep_frames_per_block" in _lib.PLAIN and _lib.ABI_VERSION >= 15
    fpb = _lib.load().bff_sweep_frames_per_block                  # a host function: no GPU needed to ask
    assert [fpb(sc.N_POINTS, p) for p in sc.PREFIXES] == list(sc.EXPECTED_FPB)
    for n, f in ((1, 1), (1024, 4095), (1024, 4096), (1025, 2048), (1 << 21, 1), (1 << 21, 3), (1 << 21, 65535), (237360, 300),
                 (0, 5), (5, 0)):
        assert fpb(n, f) == sc.frames_per_block_formula(n, f), (n, f)


def test_every_frame_sees_something(case):
    ordinary = np.setdiff1d(np.arange(sc.N_FRAMES), sc.NEAR)
    n = case.n_visible[ordinary]
    print(f"visible points per ordinary frame: min {n.min()}, median {np.median(n):.0f}")
    assert n.min() >= 50 and np.median(n) >= 1000
    assert sorted(case.depth_index.tolist()) == list(range(sc.N_FRAMES))
    assert len({case.inv_pose[f].tobytes() for f in range(sc.N_FRAMES)}) == sc.N_FRAMES      # a pose of its own per frame
    assert len({case.depth_raw[case.depth_index[f]].tobytes() for f in ordinary}) == ordinary.size   # and a depth image


def test_near_frames_see_points_behind_the_camera(case):
    behind = case.n_behind[list(sc.NEAR)]
    print(f"visible points with c_2 < 0 in the near frames: {behind.tolist()}")
    assert (behind > 10).all()
    assert all((case.depth_raw[case.depth_index[f]] == sc.NEAR_MM).all() for f in sc.NEAR)


def test_culling_skips_and_keeps_at_every_slot(case):
    share = [float(case.tile_inb[k::8].mean()) for k in range(8)]
    print("share of (256-point tile, frame) pairs with an in-bounds point, per slot:", [round(s, 3) for s in share])
    assert all(0.2 <= s <= 0.5 for s in share)


@pytest.mark.parametrize("wb", [32, 64])
def test_mask_sets(case, wb):
    s = case.sets[wb]
    assert tuple(v.shape[0] for v in s.views) == sc.VIEW_SIZES[wb] and max(sc.VIEW_SIZES[wb]) == wb
    assert s.n_rows <= 6000 and s.rows.shape == (s.n_rows, sc.NW) and s.chunk_mask.shape == (s.n_rows, 2)
    f = np.arange(sc.N_FRAMES)
    assert np.array_equal(s.frame_mask < 0, f % 3 == 2) and np.array_equal((case.frame_flags & 1) == 0, f % 5 == 4)
    for k in range(8):                                             # every kind of frame at every slot of an 8-tile
        assert (s.frame_mask[k::8] < 0).any() and ((case.frame_flags[k::8] & 1) == 0).any()
        assert all((s.frame_mask[k::8] == v).any() for v in range(len(s.views)))
    assert len(set(s.frame_rowbase[s.frame_nmask > 0].tolist())) == int((s.frame_nmask > 0).sum())
    total = s.pairs_palette + s.pairs_words
    print(f"word_bits {wb}: {s.n_rows} rows, {total} visible-and-masked pairs, palette share {s.pairs_palette / total:.3f}, "
          f"word share {s.pairs_words / total:.3f}")
    assert s.pairs_palette >= 0.1 * total and s.pairs_words >= 0.1 * total
    # a 256-point tile (one wave) that receives bits in two frames of one 8-tile: the wave's LDS slice is reused
    per_tile = s.tile_bits[:1000].reshape(125, 8, -1).sum(axis=1)
    print(f"word_bits {wb}: (8-tile, point tile) pairs written in >= 2 frames: {int((per_tile >= 2).sum())}")
    assert (per_tile >= 2).any()
    # the counters grow along the prefixes and the rows hold exactly the masked count
    assert sorted(s.masked_at) == sorted(case.viewed_at) == sorted(sc.PREFIXES)
    bits = np.unpackbits(s.rows.view(np.uint8), axis=1, bitorder="little")[:, :sc.N_POINTS]
    assert np.array_equal(bits.sum(axis=0, dtype=np.int64), s.masked_at[sc.N_FRAMES])
    assert not np.unpackbits(s.rows.view(np.uint8), axis=1, bitorder="little")[:, sc.N_POINTS:].any()
    for a, b in zip(sc.PREFIXES, sc.PREFIXES[1:]):
        assert (s.masked_at[b] >= s.masked_at[a]).all() and (case.viewed_at[b] >= case.viewed_at[a]).all()
    assert case.viewed_at[sc.N_FRAMES].max() > 0 and s.masked_at[sc.PREFIXES[0]].max() > 0
