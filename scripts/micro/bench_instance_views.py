"""The views of 3-D instances (views.py) on a generator scene of the c2 shape -- 200 000 points, 300 depth frames
of 968 x 1296 -- for K in {64, 4096} instances: every instance a few intervals of the Morton-sorted cloud, so that it fills
a short span of its bit row as a real instance does; lengths vary by a factor of ten and instances overlap.  The legs,
interleaved round by round, each timed with device events around `inner` calls:

  table         _lib.visibility_table over all frames (the build the views consume; it waits once for its pair count)
  views         bff_instance_views + bff_select_views (top 5, 3 crop levels)
  torch         the same counts and boxes in plain torch on the same box: the instances as a dense float32 (K, N) matrix
                times the dense visibility (N, F) for the counts, and per slot four scatter_reduce (amin / amax) over the
                instances' (instance, point) membership list for the boxes.  Its results are compared with the kernel's.

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_instance_views.py --rounds 5 --out profiles/instance_views/bench_instance_views.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from beyond_fixed_forms_amd import _lib                                  # noqa: E402
from beyond_fixed_forms_amd.config import Config                         # noqa: E402
from beyond_fixed_forms_amd.scene import DEPTH_THRESH, geometry_for_depth_frames   # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of every leg (after one warm-up round)")
ap.add_argument("--inner", type=int, default=3, help="calls per timed window")
ap.add_argument("--rows", type=int, nargs="+", default=[64, 4096])
ap.add_argument("--views", type=int, default=None, help="frames of the scene (default: config 2's 300)")
ap.add_argument("--points", type=int, default=None, help="points of the scene (default: config 2's 200 000)")
ap.add_argument("--torch-rounds", type=int, default=2, help="rounds of the torch leg")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_instance_views: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

scene = make_scene("c2", seed=0, n_views=args.views, n_points=args.points, device=dev)
h, w = scene.height, scene.width
geom = geometry_for_depth_frames(scene, Config.with_defaults(width_2d=w, height_2d=h), list(scene.poses), dev)
n, f, nw = geom.n_points, len(geom.frame_ids), geom.nw
poses = torch.from_numpy(np.ascontiguousarray(geom.inv_pose_host)).to(dev)


def build_table():
    return _lib.visibility_table(geom.xyz, n, poses, geom.cam_intr, geom.sweep_depth, h, w, DEPTH_THRESH, geom.tile_bounds,
                                 depth_size=geom.depth_size, with_count=True)


def make_rows(k, seed=0):
    """int64 [k][nw] in the sorted order: instance i = three intervals of the sorted cloud near one place."""
    rng = np.random.default_rng(seed)
    total = rng.integers(500, 5000, k) if k > 64 else rng.integers(n // 128, n // 32, k)
    centre = rng.integers(0, n, k)
    start, end, offs = [], [], [0]
    for i in range(k):
        cuts = np.sort(centre[i] + rng.integers(-3 * total[i], 3 * total[i], 3))
        for c in cuts:
            s = int(np.clip(c, 0, n - 1))
            e = int(np.clip(c + total[i] // 3, s + 1, n))
            if start and len(start) > offs[-1] and s < end[-1]:        # runs of one row: sorted and disjoint
                s = end[-1]
                if s >= e:
                    continue
            start.append(s), end.append(e)
        offs.append(len(start))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    return _lib.rle_to_rows(t(start), t(end), t(offs), n)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, out


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


table = build_table()
mask, off, pix, n_pairs = table
res = {"bench": "instance_views", "device": torch.cuda.get_device_name(0), "points": n, "frames": f, "height": h, "width": w,
       "visible_pairs": n_pairs, "table_bytes": sum(_lib.visibility_table_bytes(n, f, n_pairs)),
       "lds_words": _lib.instance_views_lds_words(), "rounds": args.rounds, "inner": args.inner,
       "torch_rounds": args.torch_rounds, "rows": {},
       "note": "device events around `inner` calls; legs interleaved round by round on one box"}

# the dense statement of the table for the torch leg
vis = _lib.unpack_rows(mask[:, :nw].contiguous(), n).bool()                       # [F][N]
u_full = torch.zeros((f, n), dtype=torch.int32, device=dev)
v_full = torch.zeros((f, n), dtype=torch.int32, device=dev)
u_full[vis], v_full[vis] = pix[:n_pairs] & 0xffff, (pix[:n_pairs] >> 16) & 0xffff
vis_t = vis.t().to(torch.float32).contiguous()                                     # [N][F]


def views_leg(rows):
    visible, box = _lib.instance_views(rows, (mask, off, pix), n_pairs, h, w)
    return (visible, box) + _lib.select_views(visible, box, h, w, 5, 1, 3, 0.1)


def torch_leg(dense, ik, ip, k):
    counts = (dense @ vis_t).to(torch.int32)
    box = torch.empty((k, f, 4), dtype=torch.int32, device=dev)
    for s in range(f):
        seen = vis[s][ip]
        for c, (plane, empty, how) in enumerate(((u_full, w, "amin"), (v_full, h, "amin"), (u_full, -1, "amax"), (v_full, -1, "amax"))):
            vals = torch.where(seen, plane[s][ip], torch.full_like(ip, empty, dtype=torch.int32))
            box[:, s, c] = torch.full((k,), empty, dtype=torch.int32, device=dev).scatter_reduce(0, ik, vals, how)
    return counts, box


with _lib.launch_stream():
    for k in args.rows:
        rows = make_rows(k)
        area = _lib.popcount_rows(rows)
        words = (rows != 0).sum(dim=1)
        times = {"table": [], "views": []}
        for rnd in range(args.rounds + 1):                                         # one warm-up round
            ms_t, _ = timed(build_table, 1)
            ms_v, got = timed(lambda: views_leg(rows), args.inner)
            if rnd >= 1:
                times["table"].append(ms_t), times["views"].append(ms_v)
        out = {name: summary(v) for name, v in times.items()}
        out.update(points_per_instance=round(float(area.float().mean()), 1), words_per_instance=round(float(words.float().mean()), 1),
                   max_words=int(words.max()), views_over_table=round(out["views"]["median_ms"] / out["table"]["median_ms"], 4))
        dense = _lib.unpack_rows(rows, n).to(torch.float32)
        ik, ip = torch.nonzero(dense, as_tuple=True)
        t_times = []
        for rnd in range(args.torch_rounds + 1):                                   # one warm-up round
            ms, ref = timed(lambda: torch_leg(dense, ik, ip, k), 1)
            if rnd >= 1:
                t_times.append(ms)
        out["torch"] = summary(t_times)
        out["torch"]["equal"] = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
        out["torch_over_views"] = round(out["torch"]["median_ms"] / out["views"]["median_ms"], 1)
        del dense, ik, ip, ref
        res["rows"][str(k)] = out

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
