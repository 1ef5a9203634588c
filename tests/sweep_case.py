"""One data set and its per-frame reference for the sweep's multi-frame tiles (host only: NumPy + oracle/geom_fma).

A room-shaped cloud of 33 blocks of points and 1001 frames, each with its own pose, depth image, row base, mask view
and flags.  Every test case is a PREFIX of the frame list: with 33 blocks the sweep (bff_sweep_frames_per_block) takes
frame tiles of 1 ... 8 frames at the prefix lengths PREFIXES, so one reference, computed once frame by frame, serves
every tile size.  The reference knows nothing of tiles: oracle.geom_fma.view per frame, the mask bit of a visible point
read from the dense masks at its pixel.

Depth comes in one form here (uint16 sensor frames) and is resized with io.resize_bilinear_f32 to the float32 (H, W)
images the reference reads; the sweep's other depth forms are re-layouts of the same sensor frames, so one reference
serves them all.  Two mask sets over the same geometry: `word_bits` 32 and 64."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import merge_ref  # noqa: E402
from mask_rows_ref import runs_of  # noqa: E402

SEED = 20240607
N_POINTS = 32 * 1024 + 700                     # 33 blocks; the last block holds 700 points: a ragged wave, an empty wave
NW = (N_POINTS + 63) // 64                     # 523: no multiple of the 4 words a wave stores
H, W = 48, 64
HS, WS = 24, 32                                # sensor frames
HW = H * W
K = np.array([[57.6, 0.0, 31.5], [0.0, 57.6, 23.5], [0.0, 0.0, 1.0]])
ROOM = np.array([4.0, 5.0, 2.5])
C0 = ROOM / 2
N_BLOB = 1500
N_FRAMES = 1001
NEAR = (11, 13, 250, 620, 997, 999)            # camera at C0, sensor frame of 30 mm everywhere; none in slot 0 of an 8-tile
NEAR_MM = 30
THRESH = 0.08
TILE = 256                                     # points of one wave = one entry of the culling table
PREFIXES = (125, 249, 373, 497, 621, 745, 869, 1000, 1001)
EXPECTED_FPB = (1, 2, 3, 4, 5, 6, 7, 8, 8)
VIEW_SIZES = {32: (1, 3, 17, 32), 64: (3, 34, 64)}
PALETTE_PIECES = {32: 16, 64: 8}               # most pieces of a 128-pixel segment the label plane keeps as a palette


def frames_per_block_formula(n_points, n_frames):
    """The library's frame tile, restated: clamp(n_frames * ceil(n_points / 1024) / 4096, 1, 8)."""
    return int(min(8, max(1, n_frames * ((n_points + 1023) // 1024) // 4096)))


def make_cloud(rng):
    """Points on the six faces of the room, N_BLOB of them replaced by a blob at the centre; Morton order."""
    from beyond_fixed_forms_amd.scene import morton_order
    p = rng.random((N_POINTS, 3)) * ROOM
    face = rng.integers(0, 6, N_POINTS)
    axis, side = face // 2, face % 2
    p[np.arange(N_POINTS), axis] = side * ROOM[axis]
    blob = rng.choice(N_POINTS, N_BLOB, replace=False)
    p[blob] = C0 + rng.normal(0.0, 0.02, (N_BLOB, 3))
    return np.ascontiguousarray(p[morton_order(p)])


def make_poses(rng):
    """-> inv_pose f64 [F][4][4]: a camera per frame in the middle 40 % of the room (NEAR frames: at the centre), any
    yaw, pitch within 0.6 rad; x right, y down, z forward."""
    pos = C0 + (rng.random((N_FRAMES, 3)) - 0.5) * 0.4 * ROOM
    pos[list(NEAR)] = C0
    yaw = rng.uniform(-np.pi, np.pi, N_FRAMES)
    pitch = rng.uniform(-0.6, 0.6, N_FRAMES)
    inv = np.empty((N_FRAMES, 4, 4))
    for f in range(N_FRAMES):
        fwd = np.array([np.cos(pitch[f]) * np.cos(yaw[f]), np.cos(pitch[f]) * np.sin(yaw[f]), np.sin(pitch[f])])
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        pose = np.eye(4)
        pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, pos[f]
        inv[f] = np.linalg.inv(pose)
    return inv


def render_sensor_frame(pts_cam, pix):
    """uint16 [HS][WS]: per texel the minimum rint(z * 1000) over the in-bounds points in front of the camera whose pixel
    maps to the texel (row v * HS // H, column u * WS // W); 0 where there is none."""
    u, v, z = pix[:, 0], pix[:, 1], pts_cam[:, 2]
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > 0)
    tex = (v[ok] * HS // H) * WS + u[ok] * WS // W
    mm = np.minimum(np.rint(z[ok] * 1000.0), 65535).astype(np.int64)
    order = np.argsort(-mm, kind="stable")                     # the smallest value of a texel is written last
    out = np.zeros(HS * WS, np.int64)
    out[tex[order]] = mm[order]
    return out.astype(np.uint16).reshape(HS, WS)


def _blob(rng, shape=None, box=None):
    """A rectangle or an ellipse of at least 6 x 6 pixels somewhere in the image (or filling box = (r0, r1, c0, c1)):
    bool [HW]."""
    if box is None:
        r0, c0 = int(rng.integers(0, H - 6)), int(rng.integers(0, W - 6))
        r1, c1 = int(rng.integers(r0 + 6, H + 1)), int(rng.integers(c0 + 6, W + 1))
    else:
        r0, r1, c0, c1 = box
    m = np.zeros((H, W), bool)
    if (rng.random() < 0.5) if shape is None else shape == "box":
        m[r0:r1, c0:c1] = True
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        m = ((yy - (r0 + r1 - 1) / 2) / ((r1 - r0) / 2)) ** 2 + ((xx - (c0 + c1 - 1) / 2) / ((c1 - c0) / 2)) ** 2 <= 1.0
    return m.reshape(-1)


def _noise(rng, rows=slice(0, H)):
    """Per-pixel noise with p = 0.5 on the given image rows: bool [HW]."""
    m = np.zeros((H, W), bool)
    m[rows] = rng.random((H, W))[rows] < 0.5
    return m.reshape(-1)


def make_views(rng, word_bits):
    """Dense views (list of bool [m][HW]) of VIEW_SIZES[word_bits] masks.  Blobs give segments of few pieces (palette
    form), noise gives a new word at almost every pixel (word form)."""
    if word_bits == 32:
        v1 = np.stack([_blob(rng, "ellipse")])
        v1[0] |= _blob(rng, "box")
        v3 = np.stack([_noise(rng) for _ in range(3)])
        v17 = np.stack([_blob(rng) for _ in range(17)])
        v32 = np.stack([_blob(rng) for _ in range(26)] + [_noise(rng, slice(8 * k, 8 * k + 12)) for k in range(5)] +
                       [np.zeros(HW, bool)])                    # the last mask is empty
        return [v1, v3, v17, v32]
    # noise on the upper half only; below it a box and an ellipse on separate rows: <= 5 pieces per two-row segment
    v3 = np.stack([_blob(rng, "box", (26, 36, 5, 60)), _blob(rng, "ellipse", (36, 48, 4, 62)), _noise(rng, slice(0, H // 2))])
    v34 = np.stack([_blob(rng) for _ in range(30)] + [_noise(rng, slice(10 * k, 10 * k + 14)) for k in range(3)] +
                   [np.zeros(HW, bool)])
    v64 = np.stack([_noise(rng) for _ in range(40)] + [_blob(rng) for _ in range(24)])
    return [v3, v34, v64]


def frame_views(word_bits):
    """frame_mask int32 [F]: -1 for f % 3 == 2; the large views at about every 13th frame (periods coprime to 8)."""
    f = np.arange(N_FRAMES)
    if word_bits == 32:
        fm = np.where(f % 13 == 0, 3, np.where(f % 13 == 6, 2, np.where(f % 7 < 3, 1, 0)))
    else:
        fm = np.where(f % 27 == 0, 2, np.where(f % 13 == 6, 1, 0))
    return np.where(f % 3 == 2, -1, fm).astype(np.int32)


def segment_is_word_form(view, word_bits):
    """bool [HW / 128]: the 128-pixel segments of a dense view with more pieces (maximal runs of pixels with the same
    mask word) than a palette block holds."""
    word = np.zeros(HW, np.uint64)
    for b, m in enumerate(view):
        word |= m.astype(np.uint64) << np.uint64(b)
    seg = word.reshape(-1, 128)
    pieces = 1 + (seg[:, 1:] != seg[:, :-1]).sum(axis=1)
    return pieces > PALETTE_PIECES[word_bits]


@dataclasses.dataclass
class MaskSet:
    word_bits: int
    views: list                  # dense bool [m][HW] per view
    frame_mask: np.ndarray       # int32 [F]
    frame_nmask: np.ndarray      # int32 [F]
    frame_rowbase: np.ndarray    # int32 [F]
    rows_upto: np.ndarray        # int64 [F + 1]: rows of the frames before f
    rows: np.ndarray             # uint64 [n_rows][NW]: expected bit rows
    chunk_mask: np.ndarray       # uint64 [n_rows][mw]
    masked_at: dict              # prefix length -> int32 [N_POINTS]
    pairs_palette: int           # visible-and-masked (point, frame) pairs in palette-form segments
    pairs_words: int             # ... in word-form segments
    tile_bits: np.ndarray        # bool [F][tiles]: the 256-point tile receives a bit in the frame

    @property
    def n_rows(self):
        return int(self.rows.shape[0])

    def run_tables(self):
        """-> (run_start, run_end, mask_run_offs, view_mask_offs) int32 over all masks of all views."""
        rs, re, offs = runs_of(np.concatenate(self.views, axis=0))
        voffs = np.concatenate([[0], np.cumsum([v.shape[0] for v in self.views])]).astype(np.int32)
        return rs, re, offs, voffs


@dataclasses.dataclass
class SweepCase:
    xyz: np.ndarray              # f64 [N_POINTS][3]
    inv_pose: np.ndarray         # f64 [F][4][4]
    depth_raw: np.ndarray        # uint16 [F][HS][WS], image of frame f at depth_index[f]
    depth_f32: np.ndarray        # float32 [F][H][W], same order
    depth_index: np.ndarray      # int32 [F], a permutation
    frame_flags: np.ndarray      # int32 [F]: bit 0 = the frame counts for viewed_count; bit 1 is noise
    vis_idx: list                # per frame: indices of the visible points
    vis_pix: list                # per frame: their flattened pixels
    n_visible: np.ndarray        # int64 [F]
    n_behind: np.ndarray         # int64 [F]: visible points with c_2 < 0
    tile_inb: np.ndarray         # bool [F][tiles]: the 256-point tile holds a point whose pixel is in bounds
    viewed_at: dict              # prefix length -> int32 [N_POINTS]
    sets: dict                   # word_bits -> MaskSet


def _mask_set(word_bits, rng, vis_idx, vis_pix):
    views = make_views(rng, word_bits)
    assert tuple(v.shape[0] for v in views) == VIEW_SIZES[word_bits]
    fm = frame_views(word_bits)
    nmask = np.array([views[v].shape[0] if v >= 0 else 0 for v in fm], np.int32)
    rows_upto = np.concatenate([[0], np.cumsum(nmask, dtype=np.int64)])
    word_form = [segment_is_word_form(v, word_bits) for v in views]
    n_tiles = (N_POINTS + TILE - 1) // TILE
    rows = np.zeros((int(rows_upto[-1]), NW), np.uint64)
    masked = np.zeros(N_POINTS, np.int32)
    masked_at, tile_bits = {}, np.zeros((N_FRAMES, n_tiles), bool)
    pal = wrd = 0
    for f in range(N_FRAMES):
        if fm[f] >= 0:
            idx, pix = vis_idx[f], vis_pix[f]
            bits = views[fm[f]][:, pix]                          # [m][visible points]
            dense = np.zeros((nmask[f], NW * 64), bool)
            dense[:, idx] = bits
            rows[rows_upto[f]:rows_upto[f + 1]] = np.packbits(dense, axis=1, bitorder="little").view(np.uint64)
            masked[idx] += bits.sum(axis=0, dtype=np.int32)
            hit = bits.any(axis=0)
            in_words = word_form[fm[f]][pix[hit] >> 7]
            wrd += int(in_words.sum())
            pal += int((~in_words).sum())
            tile_bits[f, np.unique(idx[hit] // TILE)] = True
        if f + 1 in PREFIXES:
            masked_at[f + 1] = masked.copy()
    cmask = np.concatenate([
        merge_ref.row_stats_ref(np.unpackbits(rows[r:r + 512].view(np.uint8), axis=1, bitorder="little")[:, :N_POINTS], NW)["chunk_mask"]
        for r in range(0, rows.shape[0], 512)])
    return MaskSet(word_bits, views, fm, nmask, rows_upto[:-1].astype(np.int32), rows_upto, rows, cmask, masked_at, pal, wrd,
                   tile_bits)


def build(seed=SEED):
    from beyond_fixed_forms_amd import io as bio
    from oracle import geom_fma
    rng = np.random.default_rng(seed)
    xyz = make_cloud(rng)
    inv_pose = make_poses(rng)
    f = np.arange(N_FRAMES)
    flags = (np.where(f % 5 == 4, 0, 1) | 2 * rng.integers(0, 2, N_FRAMES)).astype(np.int32)
    depth_index = rng.permutation(N_FRAMES).astype(np.int32)
    depth_raw = np.zeros((N_FRAMES, HS, WS), np.uint16)
    depth_f32 = np.zeros((N_FRAMES, H, W), np.float32)
    n_tiles = (N_POINTS + TILE - 1) // TILE
    pad = n_tiles * TILE - N_POINTS
    vis_idx, vis_pix = [], []
    n_visible, n_behind = np.zeros(N_FRAMES, np.int64), np.zeros(N_FRAMES, np.int64)
    tile_inb = np.zeros((N_FRAMES, n_tiles), bool)
    viewed, viewed_at = np.zeros(N_POINTS, np.int32), {}
    no_depth = np.zeros((H, W), np.float32)
    for i in range(N_FRAMES):
        pts, pix, _ = geom_fma.view(xyz, inv_pose[i], K, no_depth, THRESH)
        raw = np.full((HS, WS), NEAR_MM, np.uint16) if i in NEAR else render_sensor_frame(pts, pix)
        img = bio.resize_bilinear_f32(raw.astype(np.float32) / np.float32(1000), W, H)
        depth_raw[depth_index[i]], depth_f32[depth_index[i]] = raw, img
        pts, pix, vis = geom_fma.view(xyz, inv_pose[i], K, img, THRESH)
        idx = np.flatnonzero(vis)
        vis_idx.append(idx)
        vis_pix.append(pix[idx, 1] * W + pix[idx, 0])
        n_visible[i] = idx.size
        n_behind[i] = int((pts[idx, 2] < 0).sum())
        inb = (pix[:, 0] >= 0) & (pix[:, 0] < W) & (pix[:, 1] >= 0) & (pix[:, 1] < H)
        tile_inb[i] = np.concatenate([inb, np.zeros(pad, bool)]).reshape(n_tiles, TILE).any(axis=1)
        if flags[i] & 1:
            viewed += vis
        if i + 1 in PREFIXES:
            viewed_at[i + 1] = viewed.copy()
    sets = {wb: _mask_set(wb, np.random.default_rng([seed, wb]), vis_idx, vis_pix) for wb in (32, 64)}
    return SweepCase(xyz, inv_pose, depth_raw, depth_f32, depth_index, flags, vis_idx, vis_pix, n_visible, n_behind, tile_inb,
                     viewed_at, sets)


_case = None


def get():
    """The case, built once per process."""
    global _case
    if _case is None:
        _case = build()
    return _case
