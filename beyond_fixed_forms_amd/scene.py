"""Host-side preparation of one scene: reference disk formats -> HBM-resident kernel inputs.

Mirrors the loading part of the reference scene loop (tools/projection_2d_to_3d.py:376-400,
:422-436, :526-535): intrinsics `[:3,:3]`, cloud `[:, :3]` with a homogeneous 1, per-frame
`np.linalg.inv(pose)` (kept on the host in float64, exactly as the reference computes it), depth
images, and the RLE `mask_2d` list -- which is turned into flat run tables instead of being decoded
to dense (M,1,H,W) tensors.  An entry's masks may also arrive dense (the 2-D stage's own tensors) or as
masks2d.DeviceRuns (already encoded on the device); run_tables is the one place that tells them apart.

prepare_scene (one mask list) and prepare_geometry + prepare_class (several lists against one resident
scene) are put together from the same pieces: cloud_host_layout, host_depth_to_device /
raw_depth_on_device, frame_table, concat_confidences, label_ids, and device_scene, the one place a
DeviceScene is assembled from a SceneGeometry and one list's tables.  ingest.py builds the same
records from the same frame table through pinned staging and native code.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import numpy as np
import torch

DEPTH_THRESH = 0.08      # hard-coded at the reference call sites projection_2d_to_3d.py:438,565


def runs_from_rles(rles, what="mask"):
    """list of {"length","counts"} -> (start int32[R], end int32[R], offs int32[n+1]) with the decode
    semantics of rle_decode_batch (rle_encode_decode.py:45-57): 1-based (start, len) pairs cast to
    int32, `mask[lo:hi] = 1` per run (python slicing clips hi at `length`).  Runs are returned
    0-based, clipped, non-empty, sorted and disjoint per mask (overlapping or unsorted inputs are
    merged, which leaves the decoded mask unchanged)."""
    n = len(rles)
    sizes = np.fromiter((np.asarray(r["counts"]).size for r in rles), dtype=np.int64, count=n)
    if np.any(sizes % 2):
        raise ValueError(f"{what} RLE with an odd number of counts")
    flat = (np.concatenate([np.asarray(r["counts"]).reshape(-1) for r in rles]) if n and sizes.sum()
            else np.zeros(0, np.int64)).astype(np.int32)
    length = np.fromiter((int(r["length"]) for r in rles), dtype=np.int64, count=n)
    start = flat[0::2].astype(np.int64) - 1
    end = start + flat[1::2].astype(np.int64)
    owner = np.repeat(np.arange(n), sizes // 2)
    if np.any(start < 0):
        raise ValueError(f"{what} RLE with start < 1 (negative python slice in the reference decoder)")
    end = np.minimum(end, length[owner])
    ok = end > start
    start, end, owner = start[ok], end[ok], owner[ok]
    same = owner[1:] == owner[:-1]
    if np.any(same & (start[1:] < end[:-1])):          # rare: normalise per mask
        s2, e2, o2 = [], [], []
        for g in np.unique(owner):
            sel = owner == g
            order = np.argsort(start[sel], kind="stable")
            s, e = start[sel][order], end[sel][order]
            cs, ce = [s[0]], [e[0]]
            for a, b in zip(s[1:], e[1:]):
                if a <= ce[-1]:
                    ce[-1] = max(ce[-1], b)
                else:
                    cs.append(a); ce.append(b)
            s2 += cs; e2 += ce; o2 += [g] * len(cs)
        start, end, owner = np.array(s2, np.int64), np.array(e2, np.int64), np.array(o2, np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=offs[1:])
    return start.astype(np.int32), end.astype(np.int32), offs.astype(np.int32)


def morton_order(xyz: np.ndarray) -> np.ndarray:
    """Permutation that sorts points along a 3-D Morton (Z-order) curve, 10 bits per axis over the
    bounding box.  Purely a layout choice: every result of the path is invariant to the point order
    (per-point tests and set cardinalities), and outputs are returned in the original order.  Sorted
    points make instance bit rows block-sparse (the Gram skips empty chunks) and the per-frame depth /
    mask gathers of neighbouring lanes land on neighbouring pixels."""
    p = np.nan_to_num(xyz.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = p.min(axis=0), p.max(axis=0)
    q = ((p - lo) / np.maximum(hi - lo, 1e-300) * 1023.0).astype(np.uint64)
    q = np.minimum(q, 1023)

    def spread(v):
        v = (v | (v << 16)) & np.uint64(0x030000FF)
        v = (v | (v << 8)) & np.uint64(0x0300F00F)
        v = (v | (v << 4)) & np.uint64(0x030C30C3)
        v = (v | (v << 2)) & np.uint64(0x09249249)
        return v
    code = spread(q[:, 0]) | (spread(q[:, 1]) << np.uint64(1)) | (spread(q[:, 2]) << np.uint64(2))
    return np.argsort(code, kind="stable")


@dataclasses.dataclass
class DeviceScene:
    """Everything one scene needs, resident in HBM (see DESIGN.md 'Data layout')."""
    scene_id: str
    n_points: int
    nw: int
    height: int
    width: int
    cam_intr: np.ndarray                 # (3,3) float64, host (becomes kernel arguments)
    xyz: torch.Tensor                    # f64 [3][n_pad]
    depth: Optional[torch.Tensor]        # f32 [n_depth][H*W] metres, or None when depth_raw is resident instead
    # per kernel frame (mask frames in mask_2d order, then viewed-only frames)
    inv_pose: torch.Tensor               # f64 [F][16]
    depth_index: torch.Tensor            # i32 [F]
    frame_mask: torch.Tensor             # i32 [F]  index into maskbits or -1
    frame_rowbase: torch.Tensor          # i32 [F]
    frame_nmask: torch.Tensor            # i32 [F]
    frame_flags: torch.Tensor            # i32 [F]  bit0: counts towards viewed_count
    n_frames: int
    n_mask_frames: int                   # the first n_mask_frames entries carry masks
    n_viewed: int                        # number of frames of the detection-ratio sweep
    word_bits: int
    n_rows: int                          # Ins = total number of 2-D masks
    run_start: torch.Tensor
    run_end: torch.Tensor
    mask_run_offs: torch.Tensor
    view_mask_offs: torch.Tensor
    conf: torch.Tensor                   # (Ins,) float16/float32 device
    labels: List[str]                    # Ins label strings (host)
    label_id: torch.Tensor               # i32 [Ins]
    n_label_ids: int = 1                 # number of distinct label strings
    stage1: Optional[dict] = None
    unsort: Optional[torch.Tensor] = None   # i32 [N]: position of original point o in the sorted cloud (None = unsorted)
    tile_bounds: Optional[torch.Tensor] = None   # f64 [tiles][6]: boxes of the sweep's point tiles (frustum culling)
    perm: Optional[torch.Tensor] = None     # i32 [N]: original index of sorted position s (inverse of `unsort`)
    depth_raw: Optional[torch.Tensor] = None   # depth at the sensor's resolution: int16 [n_depth][hs][ws] (the uint16
                                               # millimetres of the PNGs) or -- depth_size given -- [n_depth][tiled texels]
                                               # in 8 x 8 tiles, int16 or float32 metres; the sweep evaluates the bilinear
                                               # resize (and / 1000 for int16) per point (P:432-436)
    depth_size: Optional[tuple] = None         # (hs, ws) of the tiled frames
    # one class of a multi-class run (prepare_class): the detection ratio's denominator, counted once for the scene by
    # SceneGeometry (int32 [N], sorted point order); the sweep then visits the class's mask frames only
    viewed_in: Optional[torch.Tensor] = None
    geometry: Optional["SceneGeometry"] = None   # the resident scene whose cloud, poses and depth this one shares

    @property
    def sweep_depth(self):
        """What the projection sweep gathers from: the raw frames when resident, else the float32 (H, W) images."""
        return self.depth_raw if self.depth_raw is not None else self.depth


def tile_raw_depth():
    """Layout of resident sensor-resolution depth: "f32" (default) 8 x 8-texel tiles of float32 metres (`/ 1000` done once
    per texel on the way in); BFF_DEPTH_TILES=u16: tiles of the uint16 millimetres; BFF_DEPTH_TILES=0: None, the frames
    row-major as stored.  All three give bit-identical results."""
    import os
    v = os.environ.get("BFF_DEPTH_TILES", "f32")
    return None if v == "0" else ("u16" if v == "u16" else "f32")


RAW_DEPTH_MAX_POINTS = 500_000


def keep_raw_depth(n_points: int = 0, height: int = 0, width: int = 0) -> bool:
    """Raw 16-bit depth stays resident at the sensor's resolution and is resized per point inside the sweep -- for
    clouds up to RAW_DEPTH_MAX_POINTS points; larger ones take the separate scale + resize pass into float32 (H, W)
    images (bit-identical; the pass costs 8 x the bytes, but the sweep of a 10^6-point cloud is bound by its geometry and
    runs at a higher occupancy without the resize: config 4, 1.54 vs 1.84 ms; config 2: 0.31 vs 0.28 ms).
    BFF_DEPTH_RESIZE_PASS=1 / 0 forces the pass / the in-sweep resize.  Images whose tap table (12 B per row and column)
    would not fit 48 KB of LDS always take the pass."""
    import os
    if height + width > 4096:
        return False
    v = os.environ.get("BFF_DEPTH_RESIZE_PASS")
    if v in ("0", "1"):
        return v == "0"
    return n_points <= RAW_DEPTH_MAX_POINTS


def viewed_frame_ids(color_files, downsample_ratio):
    """Reference projection_2d_to_3d.py:528-535,545."""
    files = [f for f in color_files if f.endswith(".jpg")]
    files.sort(key=lambda x: int(x.split(".")[0]))
    return [f[:-4] for f in files[::downsample_ratio]]


def with_viewed_counts(cfg) -> bool:
    """The detection-ratio filter (P:524-578) is the one that needs viewed counts."""
    return (not cfg.if_occurance_threshold) and bool(cfg.if_detected_ratio_threshold)


# ---------------------------------------------------------------------------------------------------------------------
# The pieces every preparation function is made of.  The cloud, the poses, the depth frames and the detection ratio's
# viewed counts depend on the scene alone (P:538-567 never looks at a mask): they make a SceneGeometry.  A mask_2d list
# adds a frame table, run tables, confidences and labels: together a DeviceScene.  prepare_scene builds both for one
# list; prepare_geometry + prepare_class share one geometry among several lists (pipeline.project_classes_stream,
# projection.project_scene_classes), each class bit-identical to prepare_scene on that class's own scene.  ingest.py
# builds the same records through pinned staging and native code.

def padded_points(n):
    return max(1024, ((n + 1023) // 1024) * 1024)


def cloud_host_layout(points, sort_points=True):
    """(N, >= 3) cloud -> (f64 [3][n_pad] SoA in Morton order, perm, unsort, n, n_pad); perm / unsort are None when the
    cloud is left as it is.  Sorted position s holds original point perm[s]; unsort is the inverse."""
    pts = np.asarray(points)[:, :3].astype(np.float64, copy=False)                  # :387
    n = pts.shape[0]
    n_pad = padded_points(n)
    soa = np.zeros((3, n_pad), dtype=np.float64)
    unsort = perm = None
    if sort_points and n > 1:
        perm = morton_order(pts)
        soa[:, :n] = pts[perm].T
        unsort = np.empty(n, dtype=np.int32)
        unsort[perm] = np.arange(n, dtype=np.int32)
    else:
        soa[:, :n] = pts.T
    return soa, perm, unsort, n, n_pad


def class_word_bits(mask_2d):
    """32-bit mask words unless some frame of the list holds more than 32 masks (chosen per scene / per class)."""
    max_m = max((len(fr["segmented_frame_masks"]) for fr in mask_2d), default=0)
    return 32 if max_m <= 32 else 64


def slots_on_first_use():
    """Depth slots of a single-class scene: `slot(fid)` gives a frame the next free slot when it is first asked for
    (mask frames that hold at least one mask in list order, then the viewed frames not yet seen).
    -> (slot, the frame ids in slot order, filled as slot is called)."""
    slot_of, ids = {}, []

    def slot(fid):
        s = slot_of.get(fid)
        if s is None:
            s = slot_of[fid] = len(ids)
            ids.append(fid)
        return s
    return slot, ids


@dataclasses.dataclass
class FrameTable:
    """The kernel frames of one mask_2d list (frame_table) and the per-mask rows that go with them."""
    frame_ids: List[str]                 # per kernel frame: whose pose it takes
    depth_index: List[int]               # the tables of DeviceScene, as lists
    frame_mask: List[int]
    frame_rowbase: List[int]
    frame_nmask: List[int]
    frame_flags: List[int]
    view_mask_offs: List[int]
    rles: list                           # every 2-D mask that came as an RLE dict, in row order
    conf_list: list                      # one confidence tensor per mask_2d entry
    labels: List[str]
    n_rows: int
    n_mask_frames: int
    mask_entries: list = dataclasses.field(default_factory=list)   # each entry's `segmented_frame_masks` as given: a list
                                                                   # of RLE dicts, a dense tensor or a masks2d.DeviceRuns

    def int_tables(self):
        return [np.asarray(a, dtype=np.int32) for a in (self.depth_index, self.frame_mask, self.frame_rowbase,
                                                        self.frame_nmask, self.frame_flags, self.view_mask_offs)]


def frame_table(mask_2d, word_bits, slot, viewed=None) -> FrameTable:
    """Every 2-D mask frame in list order, in chunks of <= word_bits masks (P:413-421; an entry without masks makes no
    kernel frame), `slot(fid)` naming the depth slot of each.  With `viewed` (the ordered frame ids of the
    detection-ratio sweep, P:538-567) the first chunk of a mask frame that is viewed carries flag bit 0 and the viewed
    frames left over follow as frames without masks; without, all flags are 0 and the viewed counts come from elsewhere
    (SceneGeometry.viewed)."""
    viewed_left = dict.fromkeys(viewed or ())        # ordered set of frames still to be counted
    frame_ids, d_idx, f_mask, f_rowbase, f_nmask, f_flags = [], [], [], [], [], []
    all_rles, view_mask_offs, conf_list, labels, entries = [], [0], [], [], []
    row = 0
    for fr in mask_2d:
        fid = fr["frame_id"][:-4]
        rles = fr["segmented_frame_masks"]
        m = len(rles)
        if not (len(fr["confidences"]) == m and len(fr["labels"]) == m):
            raise ValueError(f"frame {fid}: masks / confidences / labels differ in length")
        for c0 in range(0, m, word_bits):
            mc = min(word_bits, m - c0)
            frame_ids.append(fid); d_idx.append(slot(fid))
            f_mask.append(len(view_mask_offs) - 1); f_rowbase.append(row); f_nmask.append(mc)
            counted = c0 == 0 and fid in viewed_left
            if counted:
                del viewed_left[fid]
            f_flags.append(1 if counted else 0)
            view_mask_offs.append(view_mask_offs[-1] + mc)
            row += mc
        if isinstance(rles, (list, tuple)):
            all_rles += rles
        entries.append(rles)
        conf_list.append(fr["confidences"])
        labels += fr["labels"]
    n_mask_frames = len(frame_ids)
    for fid in viewed_left:
        frame_ids.append(fid); d_idx.append(slot(fid))
        f_mask.append(-1); f_rowbase.append(0); f_nmask.append(0); f_flags.append(1)
    return FrameTable(frame_ids, d_idx, f_mask, f_rowbase, f_nmask, f_flags, view_mask_offs, all_rles, conf_list, labels,
                      row, n_mask_frames, entries)


def confidence_dtype(conf_list):
    dts = {c.dtype for c in conf_list}
    if len(dts) != 1:
        raise TypeError(f"mixed confidence dtypes {dts}")
    return dts.pop()


def concat_confidences(conf_list, on_host=True):
    """One (Ins,) tensor of the frames' confidences, on the host or (on_host=False) wherever they are."""
    if not conf_list:
        return torch.zeros(0, dtype=torch.float16)
    confidence_dtype(conf_list)
    return torch.cat([c.reshape(-1).cpu() if on_host else c.reshape(-1) for c in conf_list])


def label_ids(labels):
    """-> (int32 id per label, number of distinct strings): ids in order of first appearance."""
    ids = {s: k for k, s in enumerate(dict.fromkeys(labels))}
    if len(ids) <= 1:
        return np.zeros(len(labels), dtype=np.int32), len(ids)
    return np.fromiter(map(ids.__getitem__, labels), dtype=np.int32, count=len(labels)), len(ids)


_taps = {}


def resize_taps(hs, ws, h, w, dev):
    """io.bilinear_taps of (hs, ws) -> (h, w) as device tensors, built once per size combination and device."""
    key = (hs, ws, h, w, str(dev))
    t = _taps.get(key)
    if t is None:
        from .io import bilinear_taps
        t = _taps[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in bilinear_taps(hs, ws, h, w))
    return t


def raw_depth_on_device(raw_dev, n_points, h, w, raw_depth_resident=None):
    """int16 [F][hs][ws] on the device (the PNGs' uint16 millimetres) -> (depth, depth_raw, depth_size) as DeviceScene
    holds them: resident at the sensor's resolution (keep_raw_depth, or as raw_depth_resident says), tiled unless
    BFF_DEPTH_TILES=0, or scaled + resized to float32 (H, W) images here (P:432-436)."""
    from . import _lib
    hs, ws = int(raw_dev.shape[1]), int(raw_dev.shape[2])
    if keep_raw_depth(n_points, h, w) if raw_depth_resident is None else raw_depth_resident:
        tiles = tile_raw_depth()
        if tiles:
            return None, _lib.tile_depth(raw_dev, metres=tiles == "f32"), (hs, ws)
        return None, raw_dev, None
    taps = resize_taps(hs, ws, h, w, raw_dev.device) if (hs, ws) != (h, w) else None
    return _lib.depth_from_u16(raw_dev, h, w, taps), None, None


def host_depth_to_device(scene, ids, n_points, h, w, dev, raw_depth_resident=None):
    """The depth frames `ids` of a scene, one slot each in that order -> (depth, depth_raw, depth_size): raw uint16
    frames (scene.depths_raw) uploaded as they are and handed to raw_depth_on_device, else float32 (H, W) metres."""
    raw = getattr(scene, "depths_raw", None)
    if not ids:
        return torch.zeros((0, h * w), dtype=torch.float32, device=dev), None, None
    frames = []
    for f in ids:
        if raw is not None:
            d = np.asarray(raw[f])
            if d.dtype != np.uint16 or d.ndim != 2:
                raise ValueError(f"raw depth {f}: expected a 2-D uint16 array")
            frames.append(d.view(np.int16))
        else:
            d = np.asarray(scene.depths[f], dtype=np.float32)
            if d.shape != (h, w):
                raise ValueError(f"depth {f}: shape {d.shape} != ({h},{w})")
            frames.append(d.reshape(-1))
    if any(d.shape != frames[0].shape for d in frames):
        raise ValueError("raw depth frames of different sizes")
    # frame by frame (no 1.5 GB np.stack: the copies go straight from the caller's arrays)
    out = torch.empty((len(frames),) + frames[0].shape, dtype=torch.float32 if raw is None else torch.int16, device=dev)
    for i, d in enumerate(frames):
        out[i].copy_(torch.from_numpy(np.ascontiguousarray(d)))
    return (out, None, None) if raw is None else raw_depth_on_device(out, n_points, h, w, raw_depth_resident)


def _stride_key(cfg, key) -> int:
    v = cfg.get(key, 0)
    if v is None or v is False:
        return 0
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError(f"{key}: a non-negative integer stride expected, got {v!r}")
    return int(v)


def depth_from_cloud_stride(cfg) -> int:
    """The optional config key `depth_from_cloud`: 0 (or absent) = the scene brings its depth frames; an integer stride
    s >= 1 = they are rendered from the cloud at (ceil(height_2d / s), ceil(width_2d / s))."""
    return _stride_key(cfg, "depth_from_cloud")


def depth_from_mesh_stride(cfg) -> int:
    """The optional config key `depth_from_mesh`: as depth_from_cloud, the frames rasterised from the scene's triangle
    mesh (SceneInputs.faces / mesh_vertices; on disk scene_mesh_dir/<scene_id>.npz)."""
    return _stride_key(cfg, "depth_from_mesh")


def rendered_depth_stride(cfg) -> int:
    """The stride of whichever of depth_from_cloud / depth_from_mesh is on (0 = neither: the scene brings its depth
    frames); both at once is an error."""
    cloud, mesh = depth_from_cloud_stride(cfg), depth_from_mesh_stride(cfg)
    if cloud and mesh:
        raise ValueError("depth_from_cloud and depth_from_mesh are both set: a scene's depth is rendered from one of them")
    return cloud or mesh


MESH_NEAR_CLIP_LIMIT = 65.535      # metres: the largest depth a uint16 millimetre frame holds


def mesh_near_clip(cfg) -> float:
    """The optional config key `mesh_near_clip`, in metres: 0 (absent, None) = a triangle of the mesh that reaches behind
    the camera plane is dropped whole; a value in (0, 65.535) = it is clipped at that depth instead
    (bff_render_mesh_depth_clip_u16).  It belongs to depth_from_mesh: a positive value without that key is an error."""
    v = cfg.get("mesh_near_clip", 0.0)
    if v is None:
        return 0.0
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
            not (0 <= v < MESH_NEAR_CLIP_LIMIT):                                        # NaN fails the comparison
        raise ValueError(f"mesh_near_clip: 0 (off) or a depth in metres below {MESH_NEAR_CLIP_LIMIT} expected, got {v!r}")
    if v > 0 and not depth_from_mesh_stride(cfg):
        raise ValueError("mesh_near_clip is set but depth_from_mesh is not: only the mesh renderer clips")
    return float(v)


def cloud_splat_radius(cfg) -> float:
    """The optional config key `cloud_splat_radius`, in metres: 0 (absent, None) = a point of the cloud writes one texel
    of its rendered frame; a positive value = it covers the texels within a camera-facing square of that half-width
    (bff_render_splat_depth_u16).  It belongs to depth_from_cloud: a positive value without that key is an error."""
    v = cfg.get("cloud_splat_radius", 0.0)
    if v is None:
        return 0.0
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
            not (0 <= v < np.inf):                                                      # NaN fails the comparison
        raise ValueError(f"cloud_splat_radius: 0 (off) or a finite radius in metres expected, got {v!r}")
    if v > 0 and not depth_from_cloud_stride(cfg):
        raise ValueError("cloud_splat_radius is set but depth_from_cloud is not: only the point renderer splats")
    return float(v)


def rendered_depth_size(h, w, stride):
    return -(-h // stride), -(-w // stride)


def checked_faces(faces, n_vertices) -> np.ndarray:
    """The triangles of a mesh as contiguous int32 (T, 3), checked on the host before anything is uploaded: an integer
    array of that shape whose indices lie in [0, n_vertices).  The kernel never sees a bad index."""
    if faces is None:
        raise ValueError("depth_from_mesh: the scene has no faces")
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"mesh faces: shape (T, 3) expected, got {f.shape}")
    if f.dtype == np.bool_ or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"mesh faces: an integer array expected, got {f.dtype}")
    if f.shape[0] >= 1 << 31:
        raise ValueError(f"mesh faces: {f.shape[0]} triangles, at most 2^31 - 1")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= n_vertices):
        raise ValueError(f"mesh faces: indices {int(f.min())} .. {int(f.max())} outside [0, {n_vertices})")
    return np.ascontiguousarray(f, dtype=np.int32)


def checked_mesh(scene, n_points):
    """-> (faces int32 (T, 3), the mesh's own vertices as f64 SoA [3][nv_pad] or None, number of vertices).  Without
    `mesh_vertices` the faces index the rows of the cloud (ScanNet: the cloud is the mesh's vertex array); with them the
    mesh is independent of the cloud (ScanNet++)."""
    verts = getattr(scene, "mesh_vertices", None)
    if verts is None:
        return checked_faces(getattr(scene, "faces", None), n_points), None, n_points
    v = np.asarray(verts)
    if v.ndim != 2 or v.shape[1] != 3 or not np.issubdtype(v.dtype, np.floating):
        raise ValueError(f"mesh vertices: a float array of shape (V, 3) expected, got {v.dtype} {v.shape}")
    faces = checked_faces(getattr(scene, "faces", None), v.shape[0])
    soa = np.zeros((3, padded_points(v.shape[0])), dtype=np.float64)
    soa[:, :v.shape[0]] = v.T
    return faces, soa, v.shape[0]


def mesh_for_render(faces, xyz, n_points, unsort=None, vertices=None, n_vertices=0):
    """A checked mesh on the device as bff_render_mesh_depth_u16 takes it -> (vertices f64 [3][nv_pad], their number,
    faces int32 [T][3]).  faces: int32 [T][3] on xyz's device.  Without `vertices` (the mesh's own, SoA on the device) the
    faces index the cloud: they are remapped into the sorted point order through `unsort` (None: the cloud was left as
    it is), and the sorted cloud `xyz` is the vertex array -- no second copy of it.  The triangles are launched sorted by
    their smallest vertex position, so that the vertices a wave gathers are neighbours: the one device sort per scene."""
    if vertices is None:
        vertices, n_vertices = xyz, n_points
        if unsort is not None and faces.numel():
            faces = unsort[faces.long()]
    if faces.shape[0] > 1:
        faces = faces[torch.sort(faces.min(dim=1).values).indices]
    return vertices, int(n_vertices), faces.to(torch.int32).contiguous()


def rendered_depth_on_device(xyz, n_points, inv_pose_host, cam_intr, h, w, stride, tile_bounds=None,
                             raw_depth_resident=None, inv_pose_dev=None, mesh=None, near_clip=0.0, splat_radius=0.0):
    """host_depth_to_device for a scene without depth frames: one frame per row of inv_pose_host (the slots' inverse
    poses, f64 [slots][16]) rendered from the sorted cloud `xyz` on its device (bff_render_depth_u16, one call for all
    slots, on the current stream) at 1 / stride of the working resolution, handed to raw_depth_on_device like the PNGs'
    uint16 frames -> (depth, depth_raw, depth_size).  inv_pose_dev: the same poses already on the device (ingest.py
    sends them through its pinned staging).  mesh (mesh_for_render's triple): the frames are rasterised from these
    triangles instead (bff_render_mesh_depth_u16), clipped at near_clip metres when that is positive (mesh_near_clip).
    splat_radius: positive = the cloud's points cover a footprint of that radius in metres (cloud_splat_radius,
    bff_render_splat_depth_u16)."""
    from . import _lib
    dev = xyz.device
    if dev.type != "cuda":
        raise ValueError("depth_from_cloud / depth_from_mesh need a GPU device (there is no CPU renderer)")
    if not len(inv_pose_host):
        return torch.zeros((0, h * w), dtype=torch.float32, device=dev), None, None
    dh, dw = rendered_depth_size(h, w, stride)
    inv = inv_pose_dev if inv_pose_dev is not None else \
        torch.as_tensor(np.ascontiguousarray(inv_pose_host, dtype=np.float64).reshape(-1, 16)).to(dev)
    k33 = np.asarray(cam_intr, dtype=np.float64)[:3, :3]
    if mesh is not None:
        raw = _lib.render_mesh_depth(mesh[0], mesh[1], mesh[2], inv, k33, h, w, dh, dw, near_clip=near_clip)
    else:
        splat = dict(splat_radius=splat_radius) if splat_radius else {}          # key off: the call as it always was
        raw = _lib.render_depth(xyz, n_points, inv, k33, h, w, dh, dw, tile_bounds, **splat)
    return raw_depth_on_device(raw, n_points, h, w, raw_depth_resident)


@dataclasses.dataclass
class SceneGeometry:
    """The part of a resident scene that no mask touches: sorted cloud, one inverse pose and one depth slot per frame
    id, and -- shared by the classes of a multi-class run -- the viewed counts.  Slot order: prepare_geometry takes
    frame_union (the classes' mask frames, in class then list order, then the viewed frames); prepare_scene the order
    its one frame table first asks for them (slots_on_first_use)."""
    scene_id: str
    n_points: int
    nw: int
    height: int
    width: int
    cam_intr: np.ndarray                 # (3,3) float64, host
    xyz: torch.Tensor                    # f64 [3][n_pad], sorted
    frame_ids: List[str]                 # slot k <-> frame id
    inv_pose_host: np.ndarray            # f64 [slots][16], np.linalg.inv of each pose (P:425)
    depth: Optional[torch.Tensor]        # as DeviceScene.depth / depth_raw / depth_size, one frame per slot
    depth_raw: Optional[torch.Tensor] = None
    depth_size: Optional[tuple] = None
    tile_bounds: Optional[torch.Tensor] = None
    unsort: Optional[torch.Tensor] = None
    perm: Optional[torch.Tensor] = None
    n_viewed: int = 0                    # frames of the detection-ratio sweep
    viewed: Optional[torch.Tensor] = None   # i32 [N] viewed counts in the sorted point order (None: no ratio filter)
    stage1: Optional[dict] = None

    def __post_init__(self):
        self.slot = {f: k for k, f in enumerate(self.frame_ids)}

    @property
    def sweep_depth(self):
        return self.depth_raw if self.depth_raw is not None else self.depth


def new_geometry(scene, h, w, n, ids, inv, n_viewed, xyz, depth3, bounds, unsort, perm) -> SceneGeometry:
    """depth3: (depth, depth_raw, depth_size); the scene gives its id, its intrinsics `[:3,:3]` (:376) and stage 1."""
    return SceneGeometry(scene_id=scene.scene_id, n_points=n, nw=(n + 63) // 64, height=h, width=w,
                         cam_intr=np.asarray(scene.cam_intr, dtype=np.float64)[:3, :3].copy(), xyz=xyz, frame_ids=ids,
                         inv_pose_host=inv, depth=depth3[0], depth_raw=depth3[1], depth_size=depth3[2], tile_bounds=bounds,
                         unsort=unsort, perm=perm, n_viewed=n_viewed, stage1=getattr(scene, "stage1", None))


def device_scene(geom: SceneGeometry, ft: FrameTable, word_bits, tables, inv_pose, runs, conf, n_label_ids,
                 shared) -> DeviceScene:
    """A geometry + one list's tables on the device: `tables` = FrameTable.int_tables() and the label ids, `runs` =
    (run_start, run_end, mask_run_offs).  shared: one class of a multi-class run, which keeps the geometry and takes
    its viewed counts; a single-class scene keeps neither and counts `viewed` inside its own sweep."""
    depth_index, frame_mask, frame_rowbase, frame_nmask, frame_flags, view_mask_offs, label_id = tables
    return DeviceScene(
        scene_id=geom.scene_id, n_points=geom.n_points, nw=geom.nw, height=geom.height, width=geom.width,
        cam_intr=geom.cam_intr, xyz=geom.xyz, tile_bounds=geom.tile_bounds, depth=geom.depth, inv_pose=inv_pose,
        depth_index=depth_index, frame_mask=frame_mask, frame_rowbase=frame_rowbase, frame_nmask=frame_nmask,
        frame_flags=frame_flags, n_frames=len(ft.frame_ids), n_mask_frames=ft.n_mask_frames, n_viewed=geom.n_viewed,
        word_bits=word_bits, n_rows=ft.n_rows, run_start=runs[0], run_end=runs[1], mask_run_offs=runs[2],
        view_mask_offs=view_mask_offs, conf=conf, labels=ft.labels, label_id=label_id, n_label_ids=max(1, n_label_ids),
        stage1=geom.stage1, unsort=geom.unsort, perm=geom.perm, depth_raw=geom.depth_raw, depth_size=geom.depth_size,
        viewed_in=geom.viewed if shared else None, geometry=geom if shared else None)


def class_inv_poses(geom, ft):
    """f64 [F][16]: the inverse pose of each kernel frame, out of its depth slot's."""
    return geom.inv_pose_host[np.asarray(ft.depth_index, dtype=np.int64)].reshape(len(ft.frame_ids), 16)


def _geometry(scene, cfg, ids, n_viewed, dev, sort_points, raw_depth_resident) -> SceneGeometry:
    h, w = int(cfg.height_2d), int(cfg.width_2d)
    soa, perm, unsort, n, _ = cloud_host_layout(scene.points, sort_points)
    inv = np.stack([np.linalg.inv(np.asarray(scene.poses[f], dtype=np.float64)).reshape(16) for f in ids]) if ids \
        else np.zeros((0, 16))                                                      # :425
    stride = rendered_depth_stride(cfg)
    near_clip = mesh_near_clip(cfg)
    splat_radius = cloud_splat_radius(cfg)
    mesh = checked_mesh(scene, n) if depth_from_mesh_stride(cfg) else None        # raises before anything is uploaded
    if not stride:
        depth3 = host_depth_to_device(scene, ids, n, h, w, dev, raw_depth_resident)
    xyz = torch.as_tensor(soa).to(dev)
    bounds = None
    if dev.type == "cuda" and n:
        from . import _lib
        bounds = _lib.point_tile_bounds(xyz, n)          # built once per scene, next to the spatial sort it relies on
    t32 = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    unsort = t32(unsort)
    if stride:                                           # no depth frames: the cloud or the mesh says what each camera sees
        if mesh is not None and dev.type == "cuda":
            faces, verts, nv = mesh
            mesh = mesh_for_render(torch.as_tensor(faces).to(dev), xyz, n, unsort,
                                   None if verts is None else torch.as_tensor(verts).to(dev), nv)
        depth3 = rendered_depth_on_device(xyz, n, inv, scene.cam_intr, h, w, stride, bounds, raw_depth_resident, mesh=mesh,
                                          near_clip=near_clip, splat_radius=splat_radius)
    return new_geometry(scene, h, w, n, ids, inv, n_viewed, xyz, depth3, bounds, unsort, t32(perm))


def geometry_for_depth_frames(scene, cfg, frame_ids, device="cuda") -> SceneGeometry:
    """A SceneGeometry of the frames `frame_ids` ("1230" or "1230.jpg", one slot each in that order): the sorted cloud, the
    inverse poses and the DEPTH frames -- the scene's own (scene.depths / depths_raw), or rendered as depth_from_cloud /
    depth_from_mesh say -- and no viewed counts.  What reads a scene from its instances' side needs (views.scene_views)."""
    ids = [str(f)[:-4] if str(f).endswith(".jpg") else str(f) for f in frame_ids]
    return _geometry(scene, cfg, ids, 0, torch.device(device), True, None)


def masks_all_rle(ft: FrameTable) -> bool:
    """Does every entry of the list hold its masks as RLE dicts (the mask_2d file's form)?"""
    return all(isinstance(e, (list, tuple)) for e in ft.mask_entries)


def _concat_device_runs(parts, dev):
    """DeviceRuns in row order -> (run_start, run_end, mask_run_offs) on `dev`, without a host copy of any run.
    Consecutive views of one encode_masks call are taken together; when every stretch is a whole call's tables (what
    run_tables and masks2d.to_device_runs make) the runs are concatenated as they are and the offsets shifted by the
    tables' sizes.  Anything else (a subset of a call's frames) is gathered on the device, which costs one read-back of
    the total (8 bytes)."""
    i32 = torch.int32
    segs = []                                   # [owner, first mask, end mask]
    for d in parts:
        if len(d) == 0:
            continue
        own = d.owner if d.owner is not None else d
        if segs and segs[-1][0] is own and segs[-1][2] == d.first_mask:
            segs[-1][2] += len(d)
        else:
            segs.append([own, d.first_mask, d.first_mask + len(d)])
    if not segs:
        z = torch.zeros(0, dtype=i32, device=dev)
        return [z, z.clone(), torch.zeros(1, dtype=i32, device=dev)]
    on = lambda t: t if t.device == dev else t.to(dev)
    if all(a == 0 and b == own.n_masks for own, a, b in segs):
        if len(segs) == 1:
            own = segs[0][0]
            return [on(own.run_start), on(own.run_end), on(own.mask_run_offs)]
        base, offs = 0, [torch.zeros(1, dtype=i32, device=dev)]
        for own, _, _ in segs:
            offs.append(on(own.mask_run_offs)[1:] + base)
            base += int(own.run_start.shape[0])
        if base >= 1 << 31:
            raise ValueError(f"{base} runs of 2-D masks in one scene, at most 2^31 - 1")
        return [torch.cat([on(own.run_start) for own, _, _ in segs]), torch.cat([on(own.run_end) for own, _, _ in segs]),
                torch.cat(offs).to(i32)]
    lo, ln, tab, base = [], [], [], 0
    for own, a, b in segs:
        o = on(own.mask_run_offs).to(torch.int64)
        lo.append(o[a:b] + base)
        ln.append(o[a + 1:b + 1] - o[a:b])
        tab.append(own)
        base += int(own.run_start.shape[0])
    lo, ln = torch.cat(lo), torch.cat(ln)
    cum = torch.cumsum(ln, 0)
    total = int(cum[-1].item())
    if total >= 1 << 31:
        raise ValueError(f"{total} runs of 2-D masks in one scene, at most 2^31 - 1")
    src = torch.repeat_interleave(lo - (cum - ln), ln, output_size=total) + torch.arange(total, device=dev)
    offs = torch.zeros(lo.shape[0] + 1, dtype=i32, device=dev)
    offs[1:] = cum
    return [torch.cat([on(t.run_start) for t in tab])[src], torch.cat([on(t.run_end) for t in tab])[src], offs]


def run_tables(ft: FrameTable, height, width, dev):
    """(run_start, run_end, mask_run_offs) of a frame table on `dev`, whatever form its entries' masks came in -- the
    one place that decides:
      all RLE dicts              runs_from_rles on the host, then uploaded (the mask_2d file's path, unchanged);
      dense and / or DeviceRuns  the dense entries are encoded on the device (one masks2d.encode_masks call per scene)
                                 and the tables concatenated there: no run visits the host;
      a mixed list               the device entries are read back (DeviceRuns.to_rles) and the RLE path is taken."""
    from . import masks2d
    n_pixels = height * width
    for r in ft.rles:
        if int(r["length"]) != n_pixels:
            raise ValueError(f"mask RLE length {r['length']} != H*W = {n_pixels}")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(dev)
    if masks_all_rle(ft):
        return [t(a) for a in runs_from_rles(ft.rles, "2-D mask")]
    entries = list(ft.mask_entries)
    dense = [i for i, e in enumerate(entries) if masks2d.is_dense(e)]
    for i in dense:
        masks2d._dense_shape_check(entries[i], height, width)
    for e in entries:
        if isinstance(e, masks2d.DeviceRuns) and len(e) and e.n_pixels != n_pixels:
            raise ValueError(f"mask RLE length {e.n_pixels} != H*W = {n_pixels}")
        if not (isinstance(e, (list, tuple, masks2d.DeviceRuns)) or masks2d.is_dense(e)):
            raise TypeError(f"segmented_frame_masks: RLE dicts, a dense tensor or DeviceRuns expected, got {type(e).__name__}")
    if dev.type != "cuda":
        raise ValueError("dense masks / DeviceRuns need a GPU device (there is no CPU encoder)")
    if dense:
        for i, d in zip(dense, masks2d.encode_masks([entries[i] for i in dense], dev)):
            entries[i] = d
    if not any(isinstance(e, (list, tuple)) and len(e) for e in entries):
        return _concat_device_runs([e for e in entries if isinstance(e, masks2d.DeviceRuns)], dev)
    rles, fetched = [], {}                      # every encode_masks call's tables are read back once
    for e in entries:
        if isinstance(e, masks2d.DeviceRuns):
            own = e.owner if e.owner is not None else e
            if id(own) not in fetched:
                fetched[id(own)] = own.to_rles()
            rles += fetched[id(own)][e.first_mask:e.first_mask + len(e)]
        else:
            rles += list(e)
    return [t(a) for a in runs_from_rles(rles, "2-D mask")]


def _class_tables(geom, ft, word_bits, dev, shared) -> DeviceScene:
    runs = run_tables(ft, geom.height, geom.width, dev)
    conf = concat_confidences(ft.conf_list)
    label_id, n_ids = label_ids(ft.labels)
    t = lambda a, dtype=torch.int32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)
    return device_scene(geom, ft, word_bits, [t(a) for a in ft.int_tables() + [label_id]],
                        t(class_inv_poses(geom, ft), torch.float64), runs, conf.to(dev), n_ids, shared)


def prepare_scene(scene, cfg, device="cuda", with_viewed=True, sort_points=True, raw_depth_resident=None) -> DeviceScene:
    """Upload one scene.  `scene` is duck-typed like beyond_fixed_forms_amd.synthetic.SceneInputs
    (the reference's on-disk objects held in memory)."""
    dev = torch.device(device)
    viewed = viewed_frame_ids(scene.color_files, cfg.downsample_ratio) if with_viewed else []
    word_bits = class_word_bits(scene.mask_2d)
    slot, ids = slots_on_first_use()
    ft = frame_table(scene.mask_2d, word_bits, slot, viewed)
    geom = _geometry(scene, cfg, ids, len(viewed), dev, sort_points, raw_depth_resident)
    return _class_tables(geom, ft, word_bits, dev, shared=False)


@dataclasses.dataclass
class SceneClasses:
    """One scene's inputs for several query classes: `scene` is SceneInputs-like (its own mask_2d is not used), `masks`
    maps each class to its mask_2d list (io.load_scene_classes)."""
    scene: object
    masks: Dict[str, list]


def frame_union(mask_2ds, viewed_ids=()):
    """Frame ids of several mask_2d lists (in list order, list after list), then the viewed frames: each id once."""
    ids = [fr["frame_id"][:-4] for m in mask_2ds for fr in m]
    return list(dict.fromkeys(ids + list(viewed_ids)))


def count_geometry_viewed(geom: SceneGeometry, viewed_ids, depth_thresh=DEPTH_THRESH):
    """geom.viewed = visibility counts over `viewed_ids` (bff_count_viewed, on the current stream)."""
    from . import _lib
    dev = geom.xyz.device
    geom.n_viewed = len(viewed_ids)
    viewed = torch.zeros(max(geom.n_points, 1), dtype=torch.int32, device=dev)[:geom.n_points]
    if viewed_ids and geom.n_points:
        idx = np.array([geom.slot[f] for f in viewed_ids], dtype=np.int64)
        inv = torch.as_tensor(np.ascontiguousarray(geom.inv_pose_host[idx])).to(dev, non_blocking=False)
        d_idx = torch.as_tensor(idx.astype(np.int32)).to(dev)
        _lib.count_viewed(geom.xyz, geom.n_points, inv, geom.cam_intr, geom.sweep_depth, d_idx, geom.height, geom.width,
                          depth_thresh, viewed, tile_bounds=geom.tile_bounds, depth_size=geom.depth_size)
    geom.viewed = viewed


def prepare_geometry(scene, cfg, mask_2ds, device="cuda", with_viewed=True, sort_points=True,
                     raw_depth_resident=None) -> SceneGeometry:
    """The class-independent part of prepare_scene for the classes whose mask lists are `mask_2ds`: cloud (sorted),
    inverse poses and depth of every frame any of them or the detection-ratio sweep looks at, and -- with_viewed, on a
    GPU -- the viewed counts (bff_count_viewed)."""
    dev = torch.device(device)
    viewed = viewed_frame_ids(scene.color_files, cfg.downsample_ratio) if with_viewed else []
    geom = _geometry(scene, cfg, frame_union(mask_2ds, viewed), len(viewed), dev, sort_points, raw_depth_resident)
    if with_viewed and dev.type == "cuda":
        count_geometry_viewed(geom, viewed)
    return geom


def prepare_class(geom: SceneGeometry, mask_2d, cfg, device=None) -> DeviceScene:
    """One class of a scene against its resident geometry: the class's RLE run tables, confidences and labels, and a
    frame table of its mask frames in list order whose depth_index points into the geometry's depth slots.  Frame,
    mask, label and confidence tables equal prepare_scene's for the class's own scene (with_viewed=False)."""
    dev = geom.xyz.device if device is None else torch.device(device)
    word_bits = class_word_bits(mask_2d)
    return _class_tables(geom, frame_table(mask_2d, word_bits, geom.slot.__getitem__), word_bits, dev, shared=True)
