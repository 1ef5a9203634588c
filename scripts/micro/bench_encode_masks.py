"""Dense 2-D masks -> run tables on the device: the two kernels of masks2d.hip, masks2d.encode_masks end to end, the
composition the library offered before (pack_rows + rows_to_rle) and the reference's per-mask loop, on config-2 frames
(30 x 968 x 1296 bool) whose masks come from synthetic.make_scene("c2")'s generator.  The legs are interleaved round
by round; a torch device-to-device copy of the same tensor, timed in the same rounds, is the yardstick for "streams at
HBM speed".  One JSON line on stdout (and --out FILE).

    python scripts/micro/bench_encode_masks.py --rounds 20 --scene-frames 300 --out profiles/masks2d/bench_encode_masks.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beyond_fixed_forms_amd import _lib, masks2d                      # noqa: E402
from beyond_fixed_forms_amd.scene import runs_from_rles               # noqa: E402
from beyond_fixed_forms_amd.synthetic import _rle_from_dense, make_scene    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--inner", type=int, default=100, help="launches per timed window of a kernel leg")
ap.add_argument("--distinct", type=int, default=8, help="distinct generated frames (the scene leg repeats them as copies)")
ap.add_argument("--scene-frames", type=int, default=300, help="frames of the whole-scene call (0: skip it)")
ap.add_argument("--scene-rounds", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_encode_masks: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

# ---- frames with the benchmark's own run statistics: the generator of make_scene("c2"), few views, a small cloud
scene = make_scene("c2", seed=0, n_views=args.distinct, n_points=4000, device=dev)
h, w = scene.height, scene.width
p = h * w
frames = []
for fr in scene.mask_2d:
    rs, re, offs = (torch.from_numpy(a).to(dev) for a in runs_from_rles(fr["segmented_frame_masks"]))
    frames.append(_lib.unpack_rows(_lib.rle_to_rows(rs, re, offs, p), p).view(-1, 1, h, w))
assert frames, "the generator produced no frame with masks"
frame = frames[0]
m = frame.shape[0]
rows8 = frame.view(m, p).view(torch.uint8)
nbytes = m * p
runs_per_mask = sum(len(r["counts"]) // 2 for fr in scene.mask_2d for r in fr["segmented_frame_masks"]) / (m * len(frames))


def timed(fn, inner):
    """Milliseconds per call: device events around `inner` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def wall(fn):
    """Milliseconds of one call that ends synchronised (host clock: the call's read-backs are part of it)."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


nw = (p + 63) // 64
bits = torch.empty((m, nw), dtype=torch.int64, device=dev)
counts = torch.empty(m, dtype=torch.int32, device=dev)
dst = torch.empty_like(rows8)
_lib.masks2d_count(rows8, bits, counts)
offs = torch.zeros(m + 1, dtype=torch.int32, device=dev)
offs[1:] = torch.cumsum(counts, 0)
total = int(offs[-1].item())
run_start = torch.empty(total, dtype=torch.int32, device=dev)
run_end = torch.empty(total, dtype=torch.int32, device=dev)

legs = {
    "copy_d2d": (lambda: dst.copy_(rows8), "events"),
    "count_pass": (lambda: _lib.masks2d_count(rows8, bits, counts), "events"),
    "run_pass": (lambda: _lib.masks2d_runs(bits, p, offs, run_start, run_end), "events"),
    "encode_masks": (lambda: masks2d.encode_masks(frame), "wall"),
    "parent_pack_rows_rows_to_rle": (lambda: _lib.rows_to_rle(_lib.pack_rows(rows8), p), "wall"),
    "encode_masks_to_rles": (lambda: masks2d.encode_masks(frame).to_rles(), "wall"),
    "reference_loop_on_device": (lambda: _rle_from_dense(frame.view(m, p)), "wall"),
}
samples = {k: [] for k in legs}
for rnd in range(args.rounds + 2):                     # two warm-up rounds
    for name, (fn, how) in legs.items():
        if name == "reference_loop_on_device" and rnd % 4:          # the slow leg: every fourth round
            continue
        ms = timed(fn, args.inner) if how == "events" else wall(fn)
        if rnd >= 2:
            samples[name].append(ms)

# the same result from every leg that makes one
a = masks2d.encode_masks(frame)
exp = _rle_from_dense(frame.view(m, p))
got = a.to_rles()
assert all((g["counts"] == e["counts"]).all() and g["length"] == e["length"] for g, e in zip(got, exp))
old = _lib.rows_to_rle(_lib.pack_rows(rows8), p)
assert all((g["counts"] == e["counts"]).all() for g, e in zip(old, exp))


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


res = {"bench": "encode_masks", "device": torch.cuda.get_device_name(0), "frame": [m, h, w], "dense_bytes_per_frame": nbytes,
       "runs_per_mask": round(runs_per_mask, 1), "runs_in_frame": total, "tile_pixels": masks2d.TILE_PIXELS,
       "rounds": args.rounds, "inner": args.inner, "legs": {k: summary(v) for k, v in samples.items()},
       "timing": {k: how for k, (_, how) in legs.items()},
       "note": "events: device events around `inner` launches; wall: host clock around one synchronised call (includes its "
               "read-backs).  reference_loop_on_device = rle_encode_batch's loop (RLE:10-32: one nonzero + one host copy per "
               "mask) as synthetic._rle_from_dense restates it for a device tensor."}
med = lambda k: res["legs"][k]["median_ms"]
res["count_pass_GBps_dense"] = round(nbytes / med("count_pass") / 1e6, 1)
res["copy_read_GBps"] = round(nbytes / med("copy_d2d") / 1e6, 1)
res["count_pass_over_copy_time"] = round(med("count_pass") / med("copy_d2d"), 3)
res["encode_masks_over_parent_time"] = round(med("encode_masks") / med("parent_pack_rows_rows_to_rle"), 4)
res["encode_masks_to_rles_over_parent_time"] = round(med("encode_masks_to_rles") / med("parent_pack_rows_rows_to_rle"), 4)
res["encode_masks_over_reference_loop_time"] = round(med("encode_masks") / med("reference_loop_on_device"), 5)

# ---- (b) a whole scene's frames in ONE encode_masks call (distinct generated frames, repeated as separate copies)
if args.scene_frames:
    many = [frames[i % len(frames)].clone() for i in range(args.scene_frames)]
    t = [wall(lambda: masks2d.encode_masks(many)) for _ in range(args.scene_rounds + 1)][1:]
    n_masks = sum(f.shape[0] for f in many)
    res["scene_call"] = {"frames": len(many), "masks": n_masks, "dense_bytes": n_masks * p, "distinct_frames": len(frames),
                         **summary(t), "GBps_dense": round(n_masks * p / statistics.median(t) / 1e6, 1)}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
