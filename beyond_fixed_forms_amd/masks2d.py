"""Dense 2-D masks -> run tables and RLE on the device (include/bff_hip.h: a1b).

The 2-D stage (SEG:276-305) holds every frame's masks as a dense bool tensor (M,1,H,W) on the GPU and turns them into
RLE one mask at a time before saving (encode_2d_masks RLE:63-80 -> rle_encode_batch RLE:10-32: one nonzero and one
host copy per mask).  Here a frame is encoded by two kernels with one device scan in between, and what comes out are
the int32 [start, end) run tables the projection reads (scene.DeviceScene.run_start / run_end / mask_run_offs):

    encode_masks(frames)        dense tensor(s) -> DeviceRuns (run tables on the device, nothing read back but a total)
    to_device_runs(masks_2d)    a mask_2d list with its dense entries replaced by DeviceRuns: the in-process hand-off
    encode_2d_masks(masks_2d)   the drop-in for RLE:63-80: dense entries -> RLE dicts, one read-back for the whole list

scene.run_tables accepts all three forms of an entry's `segmented_frame_masks` (RLE dicts, dense tensor, DeviceRuns).
"""
from __future__ import annotations

import dataclasses
import threading
from typing import List, Optional

import numpy as np
import torch

TILE_PIXELS = 8192        # pixels of a mask per block of the count pass (= bff_masks2d_tile_pixels(), checked by the tests)
MAX_PIXELS = (1 << 31) - 1


def runs_to_rles(start, end, offs, length):
    """Run tables (0-based [start, end), mask g owning runs offs[g]..offs[g+1]) -> the list rle_encode_batch returns
    (RLE:10-32): {"length", "counts"} with counts[2k] = start + 1, counts[2k+1] = end - start, int64.  Pure NumPy."""
    start, end = np.asarray(start).astype(np.int64), np.asarray(end).astype(np.int64)
    offs = np.asarray(offs).astype(np.int64)
    lo, hi = (int(offs[0]), int(offs[-1])) if offs.size else (0, 0)
    counts = np.empty(2 * (hi - lo), dtype=np.int64)
    counts[0::2] = start[lo:hi] + 1
    counts[1::2] = end[lo:hi] - start[lo:hi]
    return [dict(length=int(length), counts=counts[2 * (int(a) - lo):2 * (int(b) - lo)].copy())
            for a, b in zip(offs[:-1], offs[1:])]


_fetch_lock = threading.Lock()          # _lib.fetch reuses pinned staging: one caller at a time (loader threads)


def _fetch_runs(*tensors):
    """The one place run tables cross to the host (one stream synchronisation for all of `tensors`)."""
    from . import _lib
    with _fetch_lock, torch.cuda.device(tensors[0].device):
        return _lib.fetch(*tensors)


@dataclasses.dataclass(eq=False)
class DeviceRuns:
    """Run tables of the masks of one or more frames, on the device: mask g owns run_start[k] / run_end[k] (int32,
    0-based, end exclusive) for k in [mask_run_offs[g], mask_run_offs[g+1]).  The DeviceRuns of one frame of a list
    handed to encode_masks is a view: run_start / run_end are the call's shared tables and mask_run_offs (a slice of
    the shared offsets) holds absolute positions in them; `owner` / `first_mask` say which masks of which call."""
    run_start: torch.Tensor
    run_end: torch.Tensor
    mask_run_offs: torch.Tensor          # int32 [n_masks + 1]
    n_pixels: int
    n_masks: int
    frame_offs: Optional[List[int]] = None      # several frames: frame f = masks [frame_offs[f], frame_offs[f+1])
    owner: Optional["DeviceRuns"] = dataclasses.field(default=None, repr=False)
    first_mask: int = 0

    def __len__(self):
        return self.n_masks

    def to_rles(self):
        """-> [{"length": H*W, "counts": int64 ndarray}] as rle_encode_batch returns them; one read-back."""
        if self.n_masks == 0:
            return []
        return runs_to_rles(*_fetch_runs(self.run_start, self.run_end, self.mask_run_offs), self.n_pixels)

    def frames(self):
        """One view per frame of a DeviceRuns that holds several."""
        fo = self.frame_offs if self.frame_offs is not None else [0, self.n_masks]
        return [DeviceRuns(self.run_start, self.run_end, self.mask_run_offs[a:b + 1], self.n_pixels, b - a,
                           owner=self, first_mask=a) for a, b in zip(fo[:-1], fo[1:])]


def is_dense(x) -> bool:
    return torch.is_tensor(x)


def _as_rows(t, device=None):
    """One frame's dense masks -> contiguous uint8 [M][H*W] on the device, and its (H, W) when the shape says."""
    if not torch.is_tensor(t):
        raise TypeError(f"dense masks must be a torch tensor, got {type(t).__name__}")
    if t.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"dense masks must be bool or uint8, got {t.dtype}")
    hw = None
    if t.dim() == 4 and t.shape[1] == 1:
        hw = (int(t.shape[2]), int(t.shape[3]))
    elif t.dim() == 3:
        hw = (int(t.shape[1]), int(t.shape[2]))
    elif t.dim() != 2 and t.numel():
        raise ValueError(f"dense masks must be (M,1,H,W), (M,H,W) or (M,H*W), got {tuple(t.shape)}")
    m = int(t.shape[0]) if t.dim() else 0
    if device is not None and t.device != torch.device(device):
        t = t.to(device)
    elif device is None and not t.is_cuda:
        t = t.to("cuda")
    rows = t.reshape(m, -1) if m else t.reshape(0, (hw[0] * hw[1]) if hw else 0)
    rows = rows.contiguous()
    return (rows.view(torch.uint8) if rows.dtype == torch.bool else rows), hw


def _encode(frames, device=None) -> DeviceRuns:
    """All frames' masks into one pair of run tables: the count pass per frame, one cumsum over all counts, one
    read-back of the total (8 bytes), exact allocation, the run pass per frame."""
    from . import _lib
    rows = [_as_rows(f, device)[0] for f in frames]
    live = [r for r in rows if r.shape[0]]
    dev = live[0].device if live else torch.device(device if device is not None else "cuda")
    n_pixels = int(live[0].shape[1]) if live else 0
    if any(int(r.shape[1]) != n_pixels for r in live):
        raise ValueError("encode_masks: frames of different H*W in one call")
    if n_pixels > MAX_PIXELS:
        raise ValueError(f"encode_masks: H*W = {n_pixels} pixels, at most 2^31 - 1")
    frame_offs = [0]
    for r in rows:
        frame_offs.append(frame_offs[-1] + int(r.shape[0]))
    n = frame_offs[-1]
    i32 = torch.int32
    offs = torch.zeros(n + 1, dtype=i32, device=dev)
    if n == 0 or n_pixels == 0:
        z = torch.zeros(0, dtype=i32, device=dev)
        return DeviceRuns(z, z.clone(), offs, n_pixels, n, frame_offs)
    with torch.cuda.device(dev):
        nw = (n_pixels + 63) // 64
        bits = torch.empty((n, nw), dtype=torch.int64, device=dev)          # scratch: freed when this returns
        counts = torch.empty(n, dtype=i32, device=dev)
        for r, a, b in zip(rows, frame_offs[:-1], frame_offs[1:]):
            if b > a:
                _lib.masks2d_count(r, bits[a:b], counts[a:b])
        cum = torch.cumsum(counts, 0)                                        # int64
        offs[1:] = cum
        total = int(cum[-1].item())                                          # the call's one read-back
        if total >= 1 << 31:
            raise ValueError(f"encode_masks: {total} runs in one call, at most 2^31 - 1 (encode fewer frames per call)")
        run_start = torch.empty(total, dtype=i32, device=dev)
        run_end = torch.empty(total, dtype=i32, device=dev)
        for a, b in zip(frame_offs[:-1], frame_offs[1:]):
            if b > a:
                _lib.masks2d_runs(bits[a:b], n_pixels, offs[a:b + 1], run_start, run_end)
    return DeviceRuns(run_start, run_end, offs, n_pixels, n, frame_offs)


def encode_masks(frames, device=None):
    """frames: one dense tensor (M,1,H,W) / (M,H,W) / (M,H*W), bool or uint8 (any non-zero byte is a set pixel), on
    the device or on the host (then uploaded), contiguous or not -- or a list of them, one per frame (M may be 0).
    -> one DeviceRuns, or one per frame (views into tables the frames share)."""
    if torch.is_tensor(frames):
        d = _encode([frames], device)
        d.frame_offs = None
        return d
    return _encode(list(frames), device).frames()


def _dense_shape_check(t, height, width):
    if t.dim() >= 3:
        h, w = int(t.shape[-2]), int(t.shape[-1])
        if (h, w) != (height, width):
            raise ValueError(f"dense mask {h}x{w}: mask RLE length {h * w} != H*W = {height * width}")
    elif t.dim() == 2 and t.shape[0] and int(t.shape[1]) != height * width:
        raise ValueError(f"dense mask: mask RLE length {int(t.shape[1])} != H*W = {height * width}")


def to_device_runs(masks_2d, device=None):
    """The same mask_2d list with the dense `segmented_frame_masks` replaced by DeviceRuns (one encode_masks call for
    all of them; no run is read back).  Entries in another form are passed on as they are."""
    idx = [i for i, fr in enumerate(masks_2d) if is_dense(fr["segmented_frame_masks"])]
    out = list(masks_2d)
    if idx:
        for i, d in zip(idx, encode_masks([masks_2d[i]["segmented_frame_masks"] for i in idx], device)):
            out[i] = dict(masks_2d[i], segmented_frame_masks=d)
    return out


def encode_2d_masks(masks_2d, device=None):
    """Drop-in for encode_2d_masks (RLE:63-80): every entry's dense `segmented_frame_masks` becomes its list of RLE
    dicts, in place, with one read-back for the whole list; entries that already hold RLE dicts are left alone.  An entry
    that holds DeviceRuns (to_device_runs, reproject.instance_masks_2d) becomes RLE dicts too: one read-back per call
    whose tables the entries view."""
    idx = [i for i, fr in enumerate(masks_2d) if is_dense(fr["segmented_frame_masks"])]
    if idx:
        runs = _encode([masks_2d[i]["segmented_frame_masks"] for i in idx], device)
        rles = runs.to_rles()
        for i, a, b in zip(idx, runs.frame_offs[:-1], runs.frame_offs[1:]):
            masks_2d[i]["segmented_frame_masks"] = rles[a:b]
    fetched = {}
    for fr in masks_2d:
        d = fr["segmented_frame_masks"]
        if isinstance(d, DeviceRuns):
            own = d.owner if d.owner is not None else d
            if id(own) not in fetched:
                fetched[id(own)] = own.to_rles()
            fr["segmented_frame_masks"] = fetched[id(own)][d.first_mask:d.first_mask + len(d)]
    return masks_2d
