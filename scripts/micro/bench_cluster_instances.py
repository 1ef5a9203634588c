"""The density index and the clustering of 3-D instances by density (density.density_index, density.cluster_rows; DESIGN
7j) on a config-2-shaped scene: synthetic.make_scene("c2", cut_masks=False, distinct_masks=True), the stage-2 rows
project_scene gives for it, and those rows with pairs OR-ed together (the over-merged case).  The legs, interleaved round
by round, wall clock around one call (all hold read-backs):

  index            density_index of the cloud (the grid at a cell a hair above eps, the points of every cell, the gathered cloud)
  cluster          cluster_rows of the stage-2 rows (elements, core, link, count, emit; two read-backs)
  cluster_merged   the same for the rows OR-ed in pairs
  sklearn          sklearn.cluster.DBSCAN per row on the same rows, where sklearn imports: its fit alone, the row's points
                   gathered beforehand; its cluster count and clustered points are set beside the device's

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_cluster_instances.py --rounds 10 --out profiles/cluster_instances/bench_cluster_instances.json
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
from beyond_fixed_forms_amd import _lib, density                        # noqa: E402
from beyond_fixed_forms_amd.config import Config                        # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene             # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--eps", type=float, nargs="+", default=[0.05, 0.1], help="neighbourhood radii, metres")
ap.add_argument("--min-samples", type=int, default=8)
ap.add_argument("--min-points", type=int, default=1)
ap.add_argument("--host-rounds", type=int, default=3, help="rounds of the sklearn leg")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_cluster_instances: needs the GPU (there is no CPU path to time)")
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
    from sklearn.cluster import DBSCAN
except ImportError:
    DBSCAN = None


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


dense = _lib.unpack_rows(rows, n).cpu().numpy()
res = {"bench": "cluster_instances", "device": torch.cuda.get_device_name(0), "points": n, "stage2_rows": k,
       "merged_rows": int(merged.shape[0]), "points_per_row": [int(c) for c in dense.sum(1).tolist()][:64],
       "rounds": args.rounds, "min_samples": args.min_samples, "min_points": args.min_points, "eps": {},
       "note": "wall clock around one call, device idle before and after; legs interleaved round by round"}
with _lib.launch_stream():
    for eps in args.eps:
        index = density.density_index(pts_dev, eps)
        legs = {"index": lambda eps=eps: density.density_index(pts_dev, eps),
                "cluster": lambda index=index: density.cluster_rows(index, rows, n, args.min_samples, args.min_points),
                "cluster_merged": lambda index=index: density.cluster_rows(index, merged, n, args.min_samples, args.min_points)}
        times = {name: [] for name in legs}
        for rnd in range(args.rounds + 2):             # two warm-up rounds
            for name, fn in legs.items():
                ms, _ = wall(fn)
                if rnd >= 2:
                    times[name].append(ms)
        out = {name: summary(v) for name, v in times.items()}
        parts, parent, points = density.cluster_rows(index, rows, n, args.min_samples, args.min_points)
        parts_m, _, points_m = density.cluster_rows(index, merged, n, args.min_samples, args.min_points)
        offs = index.nearest.offs.cpu().numpy().astype(np.int64)
        out.update(cells_occupied=index.nearest.grid.n_voxels, points_per_cell_max=int(np.diff(offs).max()),
                   clusters=int(parts.shape[0]), points_kept=int(points.sum()), points_in_rows=int(dense.sum()),
                   clusters_of_merged=int(parts_m.shape[0]), clusters_of_merged_with_100_points=int((points_m >= 100).sum()))
        if DBSCAN is not None:
            host = []
            clouds = [np.ascontiguousarray(scene.points[row, :3], dtype=np.float64) for row in dense]
            for rnd in range(args.host_rounds):
                t0 = time.perf_counter()
                fits = [DBSCAN(eps=eps, min_samples=args.min_samples).fit(x) if len(x) else None for x in clouds]
                host.append((time.perf_counter() - t0) * 1e3)
            clusters = int(sum(int(f.labels_.max()) + 1 for f in fits if f is not None))
            out["sklearn"] = dict(summary(host), what="sklearn.cluster.DBSCAN.fit per row, the rows' points gathered beforehand",
                                  clusters=clusters, clusters_equal=clusters == out["clusters"] if args.min_points == 1 else None,
                                  points_kept=int(sum(int((f.labels_ >= 0).sum()) for f in fits if f is not None)))
            out["sklearn_over_device"] = round(out["sklearn"]["median_ms"] / out["cluster"]["median_ms"], 1)
        else:
            out["sklearn"] = "sklearn does not import here: no host leg"
        res["eps"][str(eps)] = out

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
