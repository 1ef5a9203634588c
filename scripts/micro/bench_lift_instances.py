"""The nearest-neighbour search on the voxel grid and the many-row bit gather (lift.nearest_index, lift.nearest,
lift.lift_rows) at two sizes, the legs interleaved round by round and timed with device events around one call:

  c2        the config-2 generator cloud (200 000 points, synthetic.make_scene("c2") with one view: the cloud is drawn
            before the views, so it is that scene's) as the target, its subsample at --voxel as the source; one row per
            generator object
  2M        a 2 000 000-point cloud of the same generator geometry as the target, the c2 cloud as the source, --rows
            random rows

  index     nearest_index of the source (the voxel grid, the cells' point lists, the gathered cloud; holds read-backs)
  search    nearest of every target point (bff_nn_search)
  lift      lift_rows (bff_rows_to_columns + bff_lift_bits, the two allocations included)
  transpose / gather   the two entry points alone, into buffers made before
  cdist     the baseline a user would otherwise write, on the same device in the same session: torch.cdist of a chunk of
            queries against the whole source, argmin, a radius test; on the first --baseline-queries targets only where
            that is stated, never extrapolated

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_lift_instances.py --rounds 10 --out profiles/lift_instances/bench_lift_instances.json
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
from beyond_fixed_forms_amd import _lib, lift                            # noqa: E402
from beyond_fixed_forms_amd._lib import _ptr, call                      # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--voxel", type=float, default=0.05, help="subsample_voxel of the c2 size, metres")
ap.add_argument("--rows", type=int, default=100, help="rows of the 2M size")
ap.add_argument("--big-points", type=int, default=2_000_000)
ap.add_argument("--big-radius", type=float, default=0.05, help="max_dist of the 2M size, metres")
ap.add_argument("--baseline-queries", type=int, default=200_000, help="targets the cdist leg of the 2M size runs on")
ap.add_argument("--baseline-rounds", type=int, default=3)
ap.add_argument("--chunk-bytes", type=int, default=1 << 30, help="bytes of one cdist chunk's distance matrix")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_lift_instances: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def cdist_nearest(src, qs, radius):
    """Chunked torch.cdist + argmin + the radius test -> nn int32 (the first index among equal distances)."""
    chunk = max(1, args.chunk_bytes // (8 * max(1, src.shape[0])))
    out = torch.empty(qs.shape[0], dtype=torch.int32, device=qs.device)
    for a in range(0, qs.shape[0], chunk):
        d, i = torch.cdist(qs[a:a + chunk], src).min(1)
        out[a:a + chunk] = torch.where(d <= radius, i, torch.full_like(i, -1)).to(torch.int32)
    return out


def one_size(name, source, target, radius, rows, baseline_queries):
    m, n, k = int(source.shape[0]), int(target.shape[0]), int(rows.shape[0])
    index = lift.nearest_index(source, radius)
    nn = lift.nearest(index, target)
    kw, nw_out = (k + 63) // 64, (n + 63) // 64
    cols = torch.empty((m, kw), dtype=torch.int64, device=dev)
    out = torch.empty((k, nw_out), dtype=torch.int64, device=dev)
    legs = {"index": lambda: lift.nearest_index(source, radius),
            "search": lambda: lift.nearest(index, target),
            "lift": lambda: lift.lift_rows(nn, rows, m, n),
            "transpose": lambda: call("bff_rows_to_columns", _ptr(rows), k, int(rows.shape[1]), m, _ptr(cols)),
            "gather": lambda: call("bff_lift_bits", _ptr(cols), m, k, _ptr(nn), n, _ptr(out))}
    b = min(n, baseline_queries)
    base_q = target[:b].contiguous()
    base_rounds = args.rounds if b == n else args.baseline_rounds
    legs_b = {"cdist": lambda: cdist_nearest(source, base_q, radius), "search_same_queries": lambda: lift.nearest(index, base_q)}
    times = {name: [] for name in list(legs) + list(legs_b)}
    with _lib.launch_stream():
        for rnd in range(args.rounds + 2):                 # two warm-up rounds
            for leg, fn in legs.items():
                ms, _ = timed(fn)
                if rnd >= 2:
                    times[leg].append(ms)
            if rnd < base_rounds + 1:                      # one warm-up round
                for leg, fn in legs_b.items():
                    ms, _ = timed(fn)
                    if rnd >= 1:
                        times[leg].append(ms)
        base_nn = cdist_nearest(source, base_q, radius)
    res = {name_: summary(v) for name_, v in times.items()}
    cells = (index.offs[1:] - index.offs[:-1]).double()
    res.update(source_points=m, target_points=n, rows=k, radius=radius, cells=index.grid.n_voxels,
               points_per_cell={"mean": round(float(cells.mean()), 2), "max": int(cells.max())},
               targets_without_source=int((nn < 0).sum()), baseline_queries=b,
               baseline_chunk_queries=max(1, args.chunk_bytes // (8 * max(1, m))),
               baseline_agrees=int((base_nn == nn[:b]).sum()),
               cdist_over_search=round(res["cdist"]["median_ms"] / res["search_same_queries"]["median_ms"], 1),
               lift_equals_permute_bits=None)
    if (nn >= 0).all():
        res["lift_equals_permute_bits"] = bool(torch.equal(lift.lift_rows(nn, rows, m, n), _lib.permute_bits(rows, nn, n)))
    return res


def object_rows(obj):
    """One bit row per generator object (the room is -1) of a cloud."""
    ids = np.unique(obj)
    return _lib.pack_rows(torch.from_numpy(np.stack([obj == i for i in ids])).to(dev).contiguous())


res = {"bench": "lift_instances", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
       "note": "device events around one call, legs interleaved round by round; cdist is float64, chunked so that one "
               "distance matrix takes --chunk-bytes"}
c2 = make_scene("c2", seed=0, n_views=1, n_masks=1, n_stage1=1)
full = torch.from_numpy(np.ascontiguousarray(c2.points[:, :3])).to(dev)
sample = lift.subsample(full, args.voxel)
small = full[sample.long()].contiguous()
res["c2"] = dict(one_size("c2", small, full, lift.lift_max_dist({"subsample_voxel": args.voxel}),
                          object_rows(c2.point_object[sample.cpu().numpy()]), 1 << 62), subsample_voxel=args.voxel)
big = make_scene((args.big_points, 1, 120, 160, 1), seed=0, n_stage1=1)     # the same cuboids: they are drawn first
target = torch.from_numpy(np.ascontiguousarray(big.points[:, :3])).to(dev)
gen = torch.Generator(device="cpu").manual_seed(0)
rows = torch.randint(-2 ** 63, 2 ** 63 - 1, (args.rows, (full.shape[0] + 63) // 64), dtype=torch.int64, generator=gen).to(dev)
res["2M"] = one_size("2M", full, target, args.big_radius, rows, args.baseline_queries)

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
