"""Overlapped scene ingestion: reference host objects -> HBM-resident kernel inputs
without the host thread of the device path paying for it.

`prepare_scene_fast` does what scene.prepare_scene does (P:376-400, 422-436, 526-535) with the byte work moved off
the interpreter: the RLE dicts become run tables in libbff_host.so (native threads, GIL released, written straight
into pinned staging), depth frames are packed into pinned staging the same way and uploaded as ONE asynchronous
copy (raw 16-bit frames are scaled + resized on the device, P:432-436), poses are inverted in one batched LAPACK
call (np.linalg.inv over the stack = the same gesv per matrix as P:425), and the cloud is sorted and laid out on the
device (bff_cloud_layout).  Everything is enqueued on the caller's stream, so a loader thread with its own stream
overlaps the uploads of scene i+1 with the kernels of scene i (`Ingestor`).  Inputs the fast path does not cover
(unsorted / overlapping runs, mixed frame sizes, CPU devices) fall back to scene.prepare_scene: same results.

The bookkeeping is scene.py's (frame_table, label_ids, raw_depth_on_device, device_scene); this module adds the
transport: _run_tables, _gather_confidences and _upload_tables for one mask list (_class_to_device), _depth_to_device
and _cloud_to_device for the scene (_geometry_to_device).  prepare_scene_fast is the two halves on one Staging between
one wait and one fence; prepare_geometry_fast and prepare_class_fast are one half each, with a wait and a fence of
their own.
"""
from __future__ import annotations

import ctypes
import inspect
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from ctypes import c_int, c_longlong, c_void_p, py_object

import numpy as np
import torch

from . import _lib
from .scene import (DeviceScene, SceneGeometry, checked_mesh, class_inv_poses, class_word_bits, cloud_splat_radius,
                    concat_confidences, confidence_dtype, count_geometry_viewed, depth_from_mesh_stride, device_scene,
                    frame_table, frame_union, label_ids, masks_all_rle, mesh_for_render, mesh_near_clip, new_geometry,
                    padded_points, prepare_class, prepare_geometry, prepare_scene, raw_depth_on_device,
                    rendered_depth_on_device, rendered_depth_stride, run_tables, slots_on_first_use, viewed_frame_ids,
                    with_viewed_counts)

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "lib", "libbff_host.so")
_host = None


def host_lib():
    """libbff_host.so (CPython C API: loaded with PyDLL, the functions release the GIL themselves)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise _lib.BffLibraryError(f"{HOST_LIB_PATH} not found: build it with `make -C "
                                       f"{os.path.join(_HERE, 'csrc_host')}` (or __graft_entry__.build())")
        lib = ctypes.PyDLL(HOST_LIB_PATH)
        lib.bff_host_pack_rles.argtypes = [py_object, c_void_p, c_void_p, c_longlong, c_void_p, c_longlong, c_int]
        lib.bff_host_pack_rles.restype = c_longlong
        lib.bff_host_pack_frames.argtypes = [py_object, c_void_p, c_longlong, c_int]
        lib.bff_host_pack_frames.restype = c_longlong
        lib.bff_host_png_size.argtypes = [ctypes.c_char_p, c_void_p]
        lib.bff_host_png_size.restype = c_int
        lib.bff_host_decode_depth_pngs.argtypes = [py_object, c_void_p, c_int, c_int, c_void_p, c_int]
        lib.bff_host_decode_depth_pngs.restype = c_longlong
        lib.bff_host_abi.restype = c_int
        lib.bff_host_gather_bytes.argtypes = [c_void_p, c_void_p, c_longlong, c_void_p]
        lib.bff_host_gather_bytes.restype = c_longlong
        if lib.bff_host_abi() != 3:
            raise _lib.BffLibraryError(f"{HOST_LIB_PATH}: unexpected ABI; rebuild")
        _host = lib
    return _host


class Staging:
    """Pinned host buffers of one loader (grown on demand, reused scene after scene).  A buffer may be rewritten only
    after the copies that read it have finished: `fence()` records an event, `wait()` blocks on the last one."""

    def __init__(self):
        self.buf = {}
        self.event = None

    def get(self, name, nbytes):
        t = self.buf.get(name)
        if t is None or t.numel() < nbytes:
            t = self.buf[name] = torch.empty(max(int(nbytes), 64), dtype=torch.uint8, pin_memory=True)
        return t

    def wait(self):
        if self.event is not None:
            self.event.synchronize()

    def fence(self):
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()


_TRACE = os.environ.get("BFF_INGEST_TRACE") == "1"
trace_log = []                 # (phase, seconds) appended by loader threads when BFF_INGEST_TRACE=1 (list.append is atomic)


class _Lap:
    """Phase clock of one prepare_scene_fast call (diagnostic, off unless BFF_INGEST_TRACE=1)."""

    def __init__(self):
        self.t = time.perf_counter() if _TRACE else 0.0

    def __call__(self, phase):
        if _TRACE:
            now = time.perf_counter()
            trace_log.append((phase, now - self.t))
            self.t = now


def pack_rles(rles, expect_length, staging: Staging, tag, n_threads=4):
    """RLE dicts -> (run_start, run_end, offs) int32 pinned views, or None when the native fast path declines
    (unsorted / overlapping runs etc.: the caller uses scene.runs_from_rles)."""
    n = len(rles)
    offs = staging.get(tag + ".offs", 4 * (n + 1)).view(torch.int32)
    cap = max(staging.buf[tag + ".start"].numel() // 4 if tag + ".start" in staging.buf else 0, 1 << 16)
    while True:                                   # the native builder reports -2 when the tables are too small: grow
        rs = staging.get(tag + ".start", 4 * cap).view(torch.int32)
        re = staging.get(tag + ".end", 4 * cap).view(torch.int32)
        got = host_lib().bff_host_pack_rles(rles, rs.data_ptr(), re.data_ptr(), cap, offs.data_ptr(), int(expect_length), n_threads)
        if got != -2:
            break
        cap *= 2
    if got == -4:
        raise ValueError("2-D mask RLE with start < 1 (negative python slice in the reference decoder)")
    if got == -3:
        raise ValueError("RLE with an odd number of counts")
    if got == -6:
        raise ValueError(f"mask RLE length != H*W = {expect_length}")
    if got < 0:
        return None
    return rs[:got], re[:got], offs[:n + 1]


def _run_tables(ft, h, w, staging, dev, n_threads):
    """A frame table's masks -> (run_start, run_end, mask_run_offs) on the device.  RLE dicts: built by native threads
    straight into pinned staging; None when pack_rles declines (the caller takes the exact slow path).  Dense masks /
    DeviceRuns (scene.run_tables): encoded and concatenated on the device -- no native builder, no staging for runs."""
    if not masks_all_rle(ft):
        return run_tables(ft, h, w, dev)
    rles = ft.rles
    if rles:
        packed = pack_rles(rles, h * w, staging, "m2d", n_threads)
        if packed is None:
            return None
    else:
        z = torch.zeros(0, dtype=torch.int32)
        packed = (z, z, torch.zeros(1, dtype=torch.int32))
    return [torch.as_tensor(t).to(dev, non_blocking=True) for t in packed]


def _gather_confidences(conf_list, staging, dev):
    """The frames' confidences as one device tensor.  Host tensors (the mask_2d file's) are gathered into the pinned
    staging by ONE native call: torch.cat / reshape / numpy() per frame are ATen calls, each of which hands the GIL over
    and back; with the loader threads and the compute thread contending that cost 30-60 us per call, 8-18 ms per scene
    (BFF_INGEST_TRACE).  Tensors already on a GPU stay there (no round trip through the host, which would wait for this
    stream's uploads)."""
    if not (conf_list and all(c.device.type == "cpu" and c.is_contiguous() for c in conf_list)):
        return concat_confidences(conf_list, on_host=False).to(dev)
    dtype = confidence_dtype(conf_list)
    meta = np.empty((2, len(conf_list)), dtype=np.int64)
    meta[0] = [c.data_ptr() for c in conf_list]
    meta[1] = [c.numel() * conf_list[0].element_size() for c in conf_list]
    total = int(meta[1].sum())
    cstage = staging.get("conf", total)
    if host_lib().bff_host_gather_bytes(meta[0].ctypes.data, meta[1].ctypes.data, len(conf_list), cstage.data_ptr()) != total:
        raise ValueError("confidence tensors could not be gathered")
    return cstage[:total].view(dtype).to(dev, non_blocking=True)


def _upload_tables(tables, inv, staging, dev):
    """int32 host tables + the float64 inverse poses [F][16] through ONE pinned block and one copy
    -> (the tables as device views, inv_pose)."""
    sizes = [t.size for t in tables]
    n_int = 4 * sum(sizes)
    at = (n_int + 7) // 8 * 8
    tstage = staging.get("tables", at + 8 * inv.size + 64).numpy()
    np.concatenate(tables, out=tstage[:n_int].view(np.int32))
    tstage[at:at + 8 * inv.size].view(np.float64)[:] = inv.reshape(-1)
    tdev = staging.buf["tables"][:at + 8 * inv.size].to(dev, non_blocking=True)
    tint = tdev[:n_int].view(torch.int32)
    cuts = np.cumsum([0] + sizes)
    return [tint[cuts[k]:cuts[k + 1]] for k in range(len(tables))], \
        tdev[at:at + 8 * inv.size].view(torch.float64).view(inv.shape[0], 16)


def _geometry_to_device(scene, cfg, ids, n_viewed, dev, staging, n_threads, lap=lambda phase: None):
    """scene._geometry through pinned staging (no wait, no fence: the callers' business): poses inverted in one batched
    call (np.linalg.inv over a stack = the per-matrix LAPACK call of P:425), the frames `ids` in one copy, the cloud
    laid out on the device.  None when the depth frames are of mixed sizes / dtypes (exact slow path)."""
    h, w = int(cfg.height_2d), int(cfg.width_2d)
    pts = np.asarray(scene.points)
    if pts.dtype != np.float64 or pts.ndim != 2 or pts.shape[1] < 3 or not pts.flags.c_contiguous:
        pts = np.ascontiguousarray(pts[:, :3], dtype=np.float64)
    inv = np.linalg.inv(np.stack([np.asarray(scene.poses[f], dtype=np.float64) for f in ids])).reshape(len(ids), 16) \
        if ids else np.zeros((0, 16))
    lap("pose inverses")
    stride = rendered_depth_stride(cfg)
    near_clip = mesh_near_clip(cfg)                  # raises before any upload, like the two-keys error above
    splat_radius = cloud_splat_radius(cfg)           # likewise
    if stride:                                       # no depth frames: rendered from the cloud, so the cloud goes first
        mesh = checked_mesh(scene, pts.shape[0]) if depth_from_mesh_stride(cfg) else None    # raises before any upload
        xyz, unsort, perm, bounds = _cloud_to_device(pts, dev, staging)
        lap("cloud (copy to pinned, enqueue, layout)")
        if mesh is not None:
            mesh = _mesh_to_device(mesh, xyz, pts.shape[0], unsort, dev, staging)
        depth3 = _depth_to_device(scene, ids, pts.shape[0], h, w, dev, staging, n_threads,
                                  cloud=(xyz, inv, scene.cam_intr, stride, bounds, mesh, near_clip, splat_radius))
        lap("depth (rendered from the cloud / the mesh)")
        return new_geometry(scene, h, w, pts.shape[0], ids, inv, n_viewed, xyz, depth3, bounds, unsort, perm)
    depth3 = _depth_to_device(scene, ids, pts.shape[0], h, w, dev, staging, n_threads)
    if depth3 is None:
        return None
    lap("depth (pack / enqueue / tile)")
    xyz, unsort, perm, bounds = _cloud_to_device(pts, dev, staging)
    lap("cloud (copy to pinned, enqueue, layout)")
    return new_geometry(scene, h, w, pts.shape[0], ids, inv, n_viewed, xyz, depth3, bounds, unsort, perm)


def _class_to_device(geom, ft, word_bits, runs, staging, shared, lap=lambda phase: None) -> DeviceScene:
    """scene._class_tables through pinned staging (no wait, no fence): `runs` from _run_tables, the confidences in one
    native gather, the frame table + label ids + inverse poses as one block."""
    dev = geom.xyz.device
    conf = _gather_confidences(ft.conf_list, staging, dev)
    lap("small tables: confidences")
    label_id, n_ids = label_ids(ft.labels)
    lap("small tables: label ids")
    tables, inv_pose = _upload_tables(ft.int_tables() + [label_id], class_inv_poses(geom, ft), staging, dev)
    lap("small tables: pack + enqueue")
    return device_scene(geom, ft, word_bits, tables, inv_pose, runs, conf, n_ids, shared)


def prepare_scene_fast(scene, cfg, device="cuda", with_viewed=True, staging: Staging = None, n_threads=4) -> DeviceScene:
    """scene.prepare_scene with the byte work native / on the device; everything is enqueued on the current stream."""
    dev = torch.device(device)
    slow = lambda: prepare_scene(scene, cfg, device=device, with_viewed=with_viewed)
    if dev.type != "cuda":
        return slow()
    staging = staging or Staging()
    lap = _Lap()
    staging.wait()                                   # the previous scene's copies out of these buffers are done
    lap("wait for the staging buffers")
    viewed = _viewed_ids_cached(scene, cfg.downsample_ratio) if with_viewed else []
    word_bits = class_word_bits(scene.mask_2d)
    slot, ids = slots_on_first_use()
    ft = frame_table(scene.mask_2d, word_bits, slot, viewed)
    lap("frame table (python)")
    runs = _run_tables(ft, int(cfg.height_2d), int(cfg.width_2d), staging, dev, n_threads)
    lap("run tables (native) + upload")
    if runs is None:
        return slow()                                # rare inputs: exact slow path
    geom = _geometry_to_device(scene, cfg, ids, len(viewed), dev, staging, n_threads, lap)
    if geom is None:
        return slow()                                # mixed sizes / dtypes
    ds = _class_to_device(geom, ft, word_bits, runs, staging, False, lap)
    staging.fence()                                  # the pinned buffers may be rewritten once these copies are done
    lap("fence")
    return ds


def _depth_to_device(scene, depth_ids, n, h, w, dev, staging, n_threads, cloud=None):
    """The frames `depth_ids` of a scene on the device, in that order (scene.host_depth_to_device's layout rules): packed
    into pinned staging by native threads and uploaded as ONE asynchronous copy.  -> (depth, depth_raw, depth_size), or
    None when the frames are of mixed sizes / dtypes (the caller takes the exact slow path).
    cloud = (xyz, the frames' inverse poses on the host, K, stride, tile bounds, mesh, mesh_near_clip, cloud_splat_radius):
    the scene has no depth frames (config key depth_from_cloud or depth_from_mesh); they are rendered from the cloud already laid out on the device, or from
    the mesh on the device (_mesh_to_device; None: from the cloud), on the current stream
    (scene.rendered_depth_on_device) -- no depth staging is taken and nothing crosses the bus but the poses."""
    if cloud is not None:
        xyz, inv, cam_intr, stride, bounds, mesh, near_clip, splat_radius = cloud
        inv_dev = None
        if inv.size:
            pstage = staging.get("render.poses", inv.nbytes)
            pstage.numpy()[:inv.nbytes].view(np.float64)[:] = inv.reshape(-1)
            inv_dev = pstage[:inv.nbytes].view(torch.float64).view(-1, 16).to(dev, non_blocking=True)
        return rendered_depth_on_device(xyz, n, inv, cam_intr, h, w, stride, bounds, inv_pose_dev=inv_dev, mesh=mesh,
                                        near_clip=near_clip, splat_radius=splat_radius)
    raw_depth = getattr(scene, "depths_raw", None)
    src = raw_depth if raw_depth is not None else scene.depths
    frames = [src[f] for f in depth_ids]
    if not frames:
        return torch.zeros((0, h * w), dtype=torch.float32, device=dev), None, None
    f0 = frames[0]
    want_dtype = np.uint16 if raw_depth is not None else np.float32
    if any(getattr(f, "dtype", None) != want_dtype or f.shape != f0.shape or not f.flags.c_contiguous for f in frames) or \
            (raw_depth is None and f0.shape != (h, w)):
        return None
    each = f0.nbytes
    # the frames may already lie, in upload order, in page-locked memory: a decoder that wrote them there
    # (io.load_scene(staging=...) -> this loader's "depth" buffer) or the caller's own pinned block
    staged = getattr(scene, "depth_staged", None) if raw_depth is not None else None
    flat = None
    if staged is not None and list(staged[1]) == depth_ids:
        held = staged[0].buf.get("depth") if isinstance(staged[0], Staging) else staged[0]
        if torch.is_tensor(held) and held.is_pinned() and held.numel() * held.element_size() >= each * len(frames):
            flat = held.view(-1).view(torch.uint8)[:each * len(frames)]
    if flat is None:
        # never pack into memory the sources live in: frames that io.load_scene(staging=...) decoded into this
        # loader's "depth" buffer in another order than the upload's (a mask_2d entry without masks gets a later
        # slot or none) are packed into a second pinned buffer; bff_host_pack_frames declines aliasing on its own
        key = "depth.packed" if _frames_inside(frames, staging.buf.get("depth")) else "depth"
        stage = staging.get(key, each * len(frames))
        if host_lib().bff_host_pack_frames(frames, stage.data_ptr(), each, n_threads) != len(frames):
            return None
        flat = stage[:each * len(frames)]
    if raw_depth is None:
        return flat.view(torch.float32).view(len(frames), h * w).to(dev, non_blocking=True), None, None
    raw_dev = flat.view(torch.int16).view((len(frames),) + f0.shape).to(dev, non_blocking=True)
    return raw_depth_on_device(raw_dev, n, h, w)


def _mesh_to_device(mesh, xyz, n, unsort, dev, staging):
    """scene.checked_mesh's host triple -> scene.mesh_for_render's device triple: the faces (and the mesh's own vertices,
    where it has them) travel through pinned staging like the other small tables, enqueued on the current stream."""
    faces, verts, nv = mesh

    def up(name, a, dtype):
        stage = staging.get(name, a.nbytes)
        np.copyto(stage.numpy()[:a.nbytes].view(a.dtype).reshape(a.shape), a)
        return stage[:a.nbytes].view(dtype).view(a.shape).to(dev, non_blocking=True)
    faces_dev = up("render.faces", faces, torch.int32) if faces.size else torch.zeros((0, 3), dtype=torch.int32, device=dev)
    return mesh_for_render(faces_dev, xyz, n, unsort, None if verts is None else up("render.vertices", verts, torch.float64), nv)


def _frames_inside(frames, held):
    """Does any of the host arrays `frames` lie (partly) inside the buffer `held` (a staging tensor or None)?"""
    if held is None:
        return False
    lo = held.data_ptr()
    hi = lo + held.numel() * held.element_size()
    for f in frames:
        a = f.__array_interface__["data"][0]
        if a < hi and a + f.nbytes > lo:
            return True
    return False


def _cloud_to_device(pts, dev, staging):
    """float64 [n][stride] cloud -> (xyz [3][n_pad] sorted along the Morton curve, unsort, perm, tile bounds) as
    scene.cloud_host_layout lays them out, everything enqueued on the current stream (bff_cloud_layout)."""
    n, stride = pts.shape
    n_pad = padded_points(n)
    pstage = staging.get("points", pts.nbytes)
    np.copyto(pstage.numpy()[:pts.nbytes].view(np.float64).reshape(n, stride), pts)
    pts_dev = pstage[:pts.nbytes].view(torch.float64).view(n, stride).to(dev, non_blocking=True)
    xyz = torch.empty((3, n_pad), dtype=torch.float64, device=dev)
    if not n:
        return xyz.zero_(), None, None, None
    sort = n > 1
    unsort = torch.empty(n, dtype=torch.int32, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    codes = torch.empty(2 * n, dtype=torch.int32, device=dev)
    box = torch.empty(6, dtype=torch.float64, device=dev)
    need = ctypes.c_size_t(0)
    _lib.call("bff_cloud_layout", None, n, stride, n_pad, 1, None, None, None, None, None, None, ctypes.byref(need))
    temp = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=dev)
    nbytes = ctypes.c_size_t(temp.numel())
    _lib.call("bff_cloud_layout", _lib._ptr(pts_dev), n, stride, n_pad, 1 if sort else 0, _lib._ptr(xyz), _lib._ptr(unsort),
              _lib._ptr(perm), _lib._ptr(codes), _lib._ptr(box), _lib._ptr(temp), ctypes.byref(nbytes))
    return xyz, unsort if sort else None, perm if sort else None, _lib.point_tile_bounds(xyz, n)


def prepare_geometry_fast(scene, cfg, mask_2ds, device="cuda", with_viewed=True, staging: Staging = None,
                          n_threads=4) -> SceneGeometry:
    """scene.prepare_geometry with prepare_scene_fast's byte work: depth frames (the union of the classes' mask frames,
    then the viewed frames) through pinned staging in one copy, poses inverted in one batched call, the cloud laid out
    on the device, and the viewed counts (bff_count_viewed) -- all enqueued on the current stream."""
    dev = torch.device(device)
    if dev.type == "cuda":
        staging = staging or Staging()
        staging.wait()
        viewed = _viewed_ids_cached(scene, cfg.downsample_ratio) if with_viewed else []
        geom = _geometry_to_device(scene, cfg, frame_union(mask_2ds, viewed), len(viewed), dev, staging, n_threads)
        if geom is not None:
            if with_viewed:
                count_geometry_viewed(geom, viewed)
            staging.fence()
            return geom
    return prepare_geometry(scene, cfg, mask_2ds, device=device, with_viewed=with_viewed)


def prepare_class_fast(geom: SceneGeometry, mask_2d, cfg, staging: Staging = None, n_threads=4) -> DeviceScene:
    """scene.prepare_class with the run tables built natively into pinned staging and the small tables (frame table,
    label ids, inverse poses) uploaded as one block; only the class's own data crosses the bus."""
    dev = geom.xyz.device
    if dev.type == "cuda":
        staging = staging or Staging()
        staging.wait()
        word_bits = class_word_bits(mask_2d)
        ft = frame_table(mask_2d, word_bits, geom.slot.__getitem__)
        runs = _run_tables(ft, geom.height, geom.width, staging, dev, n_threads)
        if runs is not None:
            ds = _class_to_device(geom, ft, word_bits, runs, staging, True)
            staging.fence()
            return ds
    return prepare_class(geom, mask_2d, cfg)                        # a CPU device, rare inputs: exact slow path


def _viewed_ids_cached(scene, ratio):
    """scene.viewed_frame_ids (a sort of the ~3000 colour file names by their number) once per scene object."""
    cache = scene.__dict__.setdefault("_viewed_ids", {})
    key = (int(ratio), len(scene.color_files))
    v = cache.get(key)
    if v is None:
        v = cache[key] = viewed_frame_ids(scene.color_files, ratio)
    return v


def prepare_stage1_fast(stage1: dict, device, staging: Staging, n_threads=2):
    """refinement.prepare_stage1 through the native run-table builder."""
    from .labels import idx_to_label
    from .refinement import DeviceStage1, prepare_stage1
    rles = stage1["ins"]
    n_points = int(rles[0]["length"])
    packed = pack_rles(rles, 0, staging, "s1", n_threads)
    if packed is None or any(int(r["length"]) != n_points for r in rles):
        return prepare_stage1(stage1, device)
    rs, re, offs = (t.to(device, non_blocking=True) for t in packed)
    return DeviceStage1(n_points, rs, re, offs, [idx_to_label(int(i)) for i in stage1["final_class"]])


def _takes_staging(loader) -> bool:
    """Does the loader accept a `staging` keyword?  Decided from its signature (functools.partial objects are looked
    through), never by calling it and catching TypeError: a TypeError raised inside the loader is the caller's to see."""
    try:
        params = inspect.signature(loader).parameters
    except (TypeError, ValueError):                   # no introspectable signature: called without
        return False
    p = params.get("staging")
    if p is not None:
        return p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)
    return any(q.kind == q.VAR_KEYWORD for q in params.values())


class Ingestor:
    """Loader threads, each with its own HIP stream and pinned staging: `submit(scene)` returns a future of
    (DeviceScene, DeviceStage1 | None, ready event).  The consumer makes its compute stream wait for the event
    (`stream.wait_event`) -- it never blocks on the upload itself -- so the host->device traffic of scene i+1 runs
    under the kernels of scene i."""

    def __init__(self, cfg, device, n_loaders=4, native_threads=4, with_viewed=True, with_stage1=True):
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:      # loader threads select the device by index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.with_viewed = with_viewed
        self.with_stage1 = with_stage1
        self.native_threads = native_threads
        self.pool = ThreadPoolExecutor(max_workers=n_loaders, thread_name_prefix="bff-loader")
        self.local = threading.local()
        host_lib()
        _lib.load()

    def _loaded(self, item):
        """This loader thread's (stream, staging buffers), made on first use, and `item` -- loaded here if it is a
        loader (io.load_scene / io.load_scene_classes of one scene: the file reads run on this thread too; loaders that
        take `staging` decode depth straight into pinned memory)."""
        tl = self.local
        if not hasattr(tl, "stream"):
            torch.cuda.set_device(self.device)
            tl.stream = torch.cuda.Stream(device=self.device)
            tl.staging = Staging()
            tl.class_staging = Staging()              # the classes' small tables do not wait for the scene's depth copy
        if callable(item):
            item = item(staging=tl.staging) if _takes_staging(item) else item()
        return tl, item

    def _work(self, scene):
        tl, scene = self._loaded(scene)
        with torch.cuda.stream(tl.stream):
            ds = prepare_scene_fast(scene, self.cfg, self.device, self.with_viewed, tl.staging, self.native_threads)
            st1 = None
            if self.with_stage1 and getattr(scene, "stage1", None) is not None:
                st1 = prepare_stage1_fast(scene.stage1, self.device, tl.staging)
                tl.staging.fence()
            ev = torch.cuda.Event()
            ev.record()
        return ds, st1, ev

    def submit(self, scene):
        return self.pool.submit(self._work, scene)

    def _work_classes(self, item, classes):
        """One scene for several classes: (SceneGeometry, [DeviceScene per class], ready event)."""
        tl, item = self._loaded(item)
        masks = [item.masks[c] for c in classes]
        with torch.cuda.stream(tl.stream):
            geom = prepare_geometry_fast(item.scene, self.cfg, masks, self.device, self.with_viewed, tl.staging,
                                         self.native_threads)
            dss = [prepare_class_fast(geom, m, self.cfg, tl.class_staging, self.native_threads) for m in masks]
            ev = torch.cuda.Event()
            ev.record()
        return geom, dss, ev

    def submit_classes(self, item, classes):
        """`item`: a scene.SceneClasses or a callable that loads one (on the loader thread); `classes`: the classes to
        prepare, in order.  Future of (SceneGeometry, [DeviceScene], ready event)."""
        return self.pool.submit(self._work_classes, item, classes)

    def close(self):
        self.pool.shutdown(wait=True)


def bench_host_inclusive(scenes, cfg, device, query, sim, steps=40, n_loaders=4, native_threads=4):
    """Scenes/s from HOST arrays: every step takes a scene in the reference's host formats (float64 cloud, RLE dicts,
    poses, raw 16-bit depth frames as the PNGs store them -- here at half the working resolution, ScanNet's sensor
    ratio -- scaled and resized on the device as P:432-436) through the ingestion pipeline and then through the same
    device path as the resident benchmark.  Loader threads run `lookahead` scenes ahead of the compute thread."""
    from .projection import projection_back, projection_front
    from .refinement import refine_class
    import copy
    host = []
    for sc in scenes:
        sc = copy.copy(sc)
        if getattr(sc, "depths_raw", None) is None:
            sc.depths_raw = {f: np.ascontiguousarray(np.round(d[::2, ::2].astype(np.float64) * 1000.0).astype(np.uint16))
                             for f, d in sc.depths.items()}
        # the decoded frames as a decoder with a page-locked output delivers them (io.decode_depth_pngs into pinned
        # memory): one pinned block in upload order, set up once -- the upload then reads it in place
        order = frame_union([sc.mask_2d], viewed_frame_ids(sc.color_files, cfg.downsample_ratio) if with_viewed_counts(cfg) else [])
        f0 = sc.depths_raw[order[0]]
        block = torch.empty((len(order),) + tuple(f0.shape), dtype=torch.int16).pin_memory()
        view = block.numpy().view(np.uint16)
        for k, f in enumerate(order):
            view[k] = sc.depths_raw[f]
        sc.depths_raw = {f: view[k] for k, f in enumerate(order)}
        sc.depth_staged = (block, order)
        # host formats: the mask_2d file's confidences are host tensors
        sc.mask_2d = [dict(fr, confidences=fr["confidences"].cpu()) if torch.is_tensor(fr["confidences"]) and fr["confidences"].is_cuda
                      else fr for fr in sc.mask_2d]
        host.append(sc)
    ing = Ingestor(cfg, device, n_loaders=n_loaders, native_threads=native_threads)
    from .pipeline import scene_streams
    streams = scene_streams(device)[:2]
    lookahead = n_loaders + 1

    def run(k):
        futs = [ing.submit(host[i % len(host)]) for i in range(min(lookahead, k))]
        pend = None
        for i in range(k):
            ds, st1, ev = futs[i].result()
            if i + lookahead < k:
                futs.append(ing.submit(host[(i + lookahead) % len(host)]))
            st = streams[i % 2]
            st.wait_event(ev)
            with torch.cuda.stream(st):
                fr = projection_front(ds, cfg, stage1=st1)
            if pend is not None:
                finish(*pend)
            pend = (i, fr, st1, ds)
            futs[i] = None
        if pend is not None:
            finish(*pend)

    def finish(i, fr, st1, ds):
        with torch.cuda.stream(streams[i % 2]):
            res = projection_back(fr, want_groups=False)
            refine_class([(ds.scene_id, st1, res)], cfg, query, sim, device)

    run(min(6, steps))
    torch.cuda.synchronize()
    del trace_log[:]                                 # BFF_INGEST_TRACE: the timed calls only (first calls allocate pinned staging)
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ing.close()
    if _TRACE:
        import collections
        import sys
        acc = collections.defaultdict(lambda: [0.0, 0])
        for phase, sec in trace_log:
            acc[phase][0] += sec
            acc[phase][1] += 1
        for phase, (sec, cnt) in acc.items():
            print(f"ingest trace: {phase:42s} {1e3 * sec / max(cnt, 1):7.3f} ms per call ({cnt} calls)", file=sys.stderr)
        print(f"ingest trace: whole leg {1e3 * dt / steps:.3f} ms per scene", file=sys.stderr)
    sc = host[0]
    f0 = next(iter(sc.depths_raw.values()))
    depth_bytes = len(sc.depths_raw) * f0.nbytes
    run_bytes = 8 * sum(np.asarray(r["counts"]).size // 2 for fr in sc.mask_2d for r in fr["segmented_frame_masks"])
    cloud_bytes = np.asarray(sc.points).nbytes
    total = depth_bytes + run_bytes + cloud_bytes
    return {"value": steps / dt, "unit": "scenes/s", "ms_per_scene": 1e3 * dt / steps, "steps": steps,
            "loader_threads": n_loaders, "native_threads_per_loader": native_threads,
            "host_to_device_bytes_per_scene": int(total),
            "pcie_floor_ms": round(total / 55e9 * 1e3, 2),     # ~55 GB/s measured host->device from pinned memory (63 GB/s spec)
            "depth": f"uint16 {f0.shape[0]}x{f0.shape[1]} per frame in page-locked memory (as io.decode_depth_pngs delivers them), "
                     f"tiled on the device; /1000 + bilinear resize to {cfg.height_2d}x{cfg.width_2d} per point inside the sweep",
            "note": "inputs start in host memory in the reference's formats (float64 cloud, RLE dicts, pose matrices, decoded "
                    "16-bit depth frames); includes RLE -> run tables, pose inverses, the spatial sort (device), all uploads, "
                    "then the same device path as `value`.  PNG decode from disk is NOT included (io.decode_depth_pngs: "
                    "~0.4 ms per 480x640 frame and core)"}
