"""The voxel grid and the split of 3-D instances into connected parts (spatial.voxel_grid, spatial.split_rows; DESIGN
7g) on a config-2-shaped scene: synthetic.make_scene("c2", cut_masks=False, distinct_masks=True), the stage-2 rows
project_scene gives for it, and those rows with pairs OR-ed together (the over-merged case).  The legs, interleaved round by round, wall clock around one call
(both hold read-backs):

  grid             voxel_grid of the cloud (bounds, keys, library sort, ranks, neighbours; two read-backs)
  split            split_rows of the stage-2 rows (occupancy, prefix, union, count, emit; two read-backs)
  split_merged     the same for the rows OR-ed in pairs
  host_split       the same statement on the host: scipy.ndimage.label per row over the dense cell volume (3 x 3 x 3
                   structure) where scipy imports, tests/spatial_ref.py on a stated subsample of the points otherwise

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_split_instances.py --rounds 10 --out profiles/split_instances/bench_split_instances.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from beyond_fixed_forms_amd import _lib, spatial                        # noqa: E402
from beyond_fixed_forms_amd.config import Config                        # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene             # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--cells", type=float, nargs="+", default=[0.05, 0.1], help="cell sizes, metres")
ap.add_argument("--min-points", type=int, default=1)
ap.add_argument("--host-rounds", type=int, default=3, help="rounds of the host leg")
ap.add_argument("--subsample", type=int, default=20_000, help="points of the host leg when scipy is missing")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_split_instances: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

# whole silhouettes, different objects per view: most objects become stage-2 instances
scene = with_sensor_depth(make_scene("c2", seed=0, device=dev, cut_masks=False, distinct_masks=True))
cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
res2 = project_scene(scene, cfg, device="cuda:0", return_result=True)
rows = res2.rows.contiguous()
k, n = int(rows.shape[0]), int(scene.points.shape[0])
merged = rows[0:k - k % 2:2] | rows[1:k:2] if k >= 2 else rows
pts_dev = torch.from_numpy(np.ascontiguousarray(scene.points[:, :3], dtype=np.float64)).to(dev)
try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def host_scipy(grid_host, dense):
    """Per row: the dense cell volume, scipy's labelling, the points' labels, the kept components' sizes."""
    q, vox = grid_host
    shape = q.max(0) + 1
    sizes = []
    for row in dense:
        vol = np.zeros(shape, bool)
        cells = q[vox[row & (vox >= 0)]]
        vol[tuple(cells.T)] = True
        lab, _ = ndimage.label(vol, structure=np.ones((3, 3, 3)))
        sizes.append(np.bincount(lab[tuple(cells.T)]))
    return sizes


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


res = {"bench": "split_instances", "device": torch.cuda.get_device_name(0), "points": n, "stage2_rows": k,
       "merged_rows": int(merged.shape[0]), "points_per_row": [int(c) for c in _lib.unpack_rows(rows, n).sum(1).tolist()][:64],
       "rounds": args.rounds, "min_points": args.min_points, "cells": {},
       "note": "wall clock around one call, device idle before and after; legs interleaved round by round"}
with _lib.launch_stream():
    for cell in args.cells:
        grid = spatial.voxel_grid(pts_dev, cell)
        legs = {"grid": lambda cell=cell: spatial.voxel_grid(pts_dev, cell),
                "split": lambda grid=grid: spatial.split_rows(grid, rows, n, args.min_points),
                "split_merged": lambda grid=grid: spatial.split_rows(grid, merged, n, args.min_points)}
        times = {name: [] for name in legs}
        for rnd in range(args.rounds + 2):             # two warm-up rounds
            for name, fn in legs.items():
                ms, _ = wall(fn)
                if rnd >= 2:
                    times[name].append(ms)
        out = {name: summary(v) for name, v in times.items()}
        parts, parent, _ = spatial.split_rows(grid, rows, n, args.min_points)
        parts_m, _, points_m = spatial.split_rows(grid, merged, n, args.min_points)
        out.update(cells_occupied=grid.n_voxels, parts=int(parts.shape[0]), parts_of_merged=int(parts_m.shape[0]),
                   parts_of_merged_with_100_points=int((points_m >= 100).sum()))
        # the host leg
        keys, vox = grid.keys.cpu().numpy(), grid.vox.cpu().numpy()
        dense = _lib.unpack_rows(rows, n).cpu().numpy()
        host = []
        if ndimage is not None:
            q = np.stack([keys & ((1 << 21) - 1), (keys >> 21) & ((1 << 21) - 1), keys >> 42], 1)
            for _ in range(args.host_rounds):
                t0 = time.perf_counter()
                sizes = host_scipy((q, vox), dense)
                host.append((time.perf_counter() - t0) * 1e3)
            out["host_split"] = dict(summary(host), what="scipy.ndimage.label per row over the dense cell volume, grid given",
                                     volume=[int(s) for s in q.max(0) + 1],
                                     components=int(sum((s[1:] >= args.min_points).sum() for s in sizes)))
            out["host_split"]["components_equal_parts"] = out["host_split"]["components"] == out["parts"]
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import spatial_ref
            pick = np.sort(np.random.default_rng(0).choice(n, min(n, args.subsample), replace=False))
            sub_rows = spatial_ref.pack(dense[:, pick])
            for _ in range(args.host_rounds):
                t0 = time.perf_counter()
                spatial_ref.split_ref(scene.points[pick], cell, sub_rows, len(pick), args.min_points)
                host.append((time.perf_counter() - t0) * 1e3)
            out["host_split"] = dict(summary(host), what=f"tests/spatial_ref.py on a subsample of {len(pick)} of {n} points, "
                                                         "grid build included")
        out["host_over_device"] = round(out["host_split"]["median_ms"] / out["split"]["median_ms"], 1)
        res["cells"][str(cell)] = out

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
