"""bff_diag_sweep_lines against NumPy: the 128-byte lines one sweep touches, bit for bit.

bench.py's roofline figure counts the bits of these bitmaps, so they are pinned here on the data of tests/sweep_case.py:
the first 125 frames (the first of PREFIXES), 33 468 points, 48 x 64 images, 131 x 125 blocks.  Per frame
  * the depth bitmap holds the lines of the pixels of every in-bounds point: 32 pixels per line for float32 (H, W)
    images; for sensor frames the lines of the pixel's four source texels at the tap table's texel offsets (8 x 8 tiles),
    64 texels per line for uint16 and 32 for float32;
  * the mask bitmap holds the lines of the pixels of every visible point in the frames that have a mask view, 128 / word
    bytes pixels per line; frames without a view stay empty.
In-bounds pixels and visibility come from the case's per-frame reference (oracle.geom_fma.view on the depth resized by
io.resize_bilinear_f32); no segment bitmap, so no label lines.

With all points the depth bitmaps of this case are full (5 357 in-bounds points per frame on 3 072 pixels: every line of
every frame is touched) and only the mask bitmaps tell lines apart, so every case is repeated over the first FEW points
alone -- one wave's tile, a compact patch of each frame it is seen in -- where the depth bitmaps are sparse too."""
import ctypes

import numpy as np
import pytest
import torch

import sweep_case as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, P = sc.N_POINTS, sc.PREFIXES[0]
LINE_WORDS = 8                    # >= ceil(ceil(H * W / 16) / 32) = 6; the words behind a bitmap's last line stay zero
TEXELS_PER_LINE = {"u16tiles": 64, "f32tiles": 32}
FEW = 256


def bitmaps(lines_of_frame):
    """uint32 [P + 1][LINE_WORDS]: bit l of row f set for every l in lines_of_frame[f]; one guard row."""
    bits = np.zeros((P + 1, LINE_WORDS * 32), bool)
    for f, lines in enumerate(lines_of_frame):
        bits[f, lines] = True
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32)


class Expected:
    """The case's reference for the first P frames, as line bitmaps."""

    def __init__(self):
        from beyond_fixed_forms_amd import io as bio
        from oracle import geom_fma
        c = self.case = sc.get()
        x0, x1, _, y0, y1, _ = (a.astype(np.int64) for a in bio.bilinear_taps(sc.HS, sc.WS, sc.H, sc.W))
        tw = (sc.WS + 7) // 8
        tiled = lambda y, x: ((y >> 3) * tw + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)
        self.inb_idx, self.pixels, self.texels = [], [], []
        for f in range(P):
            _, pix, vis = geom_fma.view(c.xyz, c.inv_pose[f], sc.K, c.depth_f32[c.depth_index[f]], sc.THRESH)
            u, v = pix[:, 0], pix[:, 1]
            inb = (u >= 0) & (u < sc.W) & (v >= 0) & (v < sc.H)
            assert np.array_equal(np.flatnonzero(vis), c.vis_idx[f]) and inb[c.vis_idx[f]].all()
            u, v = u[inb], v[inb]
            self.inb_idx.append(np.flatnonzero(inb))
            self.pixels.append(v * sc.W + u)
            self.texels.append(np.stack([tiled(y0[v], x0[u]), tiled(y0[v], x1[u]), tiled(y1[v], x0[u]), tiled(y1[v], x1[u])], axis=1))
        assert sum(p.size for p in self.pixels) > 100 * P and sum(p.size for p in c.vis_pix[:P]) > 100 * P

    def depth_lines(self, depth, n):
        """of the points [0, n)"""
        if depth == "f32":
            return bitmaps([p[i < n] >> 5 for i, p in zip(self.inb_idx, self.pixels)])
        return bitmaps([t[i < n].reshape(-1) // TEXELS_PER_LINE[depth] for i, t in zip(self.inb_idx, self.texels)])

    def mask_lines(self, word_bits, n):
        c, fm = self.case, self.case.sets[word_bits].frame_mask
        per_line = 128 // (word_bits // 8)
        return bitmaps([c.vis_pix[f][c.vis_idx[f] < n] // per_line if fm[f] >= 0 else [] for f in range(P)])


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


@pytest.fixture(scope="module")
def expected():
    return Expected()


@pytest.fixture(scope="module")
def dev(expected):
    from beyond_fixed_forms_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    c = expected.case
    soa = np.full((3, N + 3), np.nan)                                # n_pad need not be a multiple of anything
    soa[:, :N] = c.xyz.T
    raw = to_dev(c.depth_raw)
    return dict(lib=_lib, xyz=to_dev(soa), inv_pose=to_dev(c.inv_pose[:P].reshape(P, 16)), depth_index=to_dev(c.depth_index[:P]),
                depth={"f32": to_dev(c.depth_f32.reshape(sc.N_FRAMES, sc.HW)), "u16tiles": _lib.tile_depth(raw, metres=False),
                       "f32tiles": _lib.tile_depth(raw, metres=True)},
                frame_mask={wb: to_dev(c.sets[wb].frame_mask[:P]) for wb in (32, 64)})


@pytest.mark.parametrize("n", [N, FEW], ids=["all", "few"])
@pytest.mark.parametrize("word_bits", [32, 64])
@pytest.mark.parametrize("depth", ["f32", "u16tiles", "f32tiles"])
def test_marked_lines_equal_reference(dev, expected, depth, word_bits, n):
    lib, ptr = dev["lib"], dev["lib"]._ptr
    dl = torch.zeros((P + 1, LINE_WORDS), dtype=torch.int32, device=DEV)
    ml = torch.zeros_like(dl)
    k = (ctypes.c_double * 9)(*[float(x) for x in sc.K.reshape(-1)])
    head = (ptr(dev["xyz"]), n, dev["xyz"].shape[1], ptr(dev["inv_pose"]), ctypes.cast(k, ctypes.c_void_p), P)
    tail = (ptr(dev["depth_index"]), sc.H, sc.W, sc.THRESH, None, word_bits, ptr(dev["frame_mask"][word_bits]), ptr(dl), ptr(ml),
            LINE_WORDS, None)
    if depth == "f32":
        lib.call("bff_diag_sweep_lines", *head, ptr(dev["depth"][depth]), *tail)
    else:
        lib.call("bff_diag_sweep_lines_u16", *head, ptr(dev["depth"][depth]), sc.HS, sc.WS, 1 if depth == "u16tiles" else 2, *tail)
    got_d, got_m = (t.cpu().numpy().view(np.uint32) for t in (dl, ml))
    exp_d, exp_m = expected.depth_lines(depth, n), expected.mask_lines(word_bits, n)
    assert exp_d.any() and exp_m.any()
    for name, got, exp in (("depth", got_d, exp_d), ("mask", got_m, exp_m)):
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, f"{name} lines differ in {bad.size} of {P} frames, first {bad[:8].tolist()}"
