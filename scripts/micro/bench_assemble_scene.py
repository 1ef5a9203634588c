"""The 3-D mask NMS of the scene assembly (assemble.nms_rows) at K in {256, 1024, 4096} rows over N = 200 000
points: every row one interval of the cloud around one of K / 8 objects with jittered ends, so that duplicates, near
duplicates and partial overlaps all occur; scores with ties.  The legs, interleaved round by round, wall clock around one
call with the device idle before and after:

  gram          bff_cross_popcount of the rows with themselves         | torch: the unpacked rows as float32, d @ d.T
  pairs         bff_nms_pairs (IoU, scope all)                         | torch: inter / (a_i + a_j - inter) in float32, the test, triu
  greedy        bff_nms_greedy (the walk and `by`)                     | torch: one masked OR per rank on the device, no read-back
  nms_rows      the whole call: clean copy, areas, rank, the three above, two read-backs

The torch legs state the same work; their keep sets are compared with the device's.  One JSON line on stdout (and --out
FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_assemble_scene.py --rounds 10 --out profiles/assemble_scene/bench_assemble_scene.json
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
from beyond_fixed_forms_amd import _lib, assemble                       # noqa: E402
from beyond_fixed_forms_amd._lib import _ptr, call                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--rows", type=int, nargs="+", default=[256, 1024, 4096])
ap.add_argument("--points", type=int, default=200_000)
ap.add_argument("--thres", type=float, default=0.5)
ap.add_argument("--torch-rounds", type=int, default=3, help="rounds of the torch legs")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_assemble_scene: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()
n = args.points


def make_rows(k, seed=0):
    rng = np.random.default_rng(seed)
    objects = max(1, k // 8)
    lo = rng.integers(0, n - 20_000, objects)
    ln = rng.integers(2_000, 20_000, objects)
    which = rng.integers(0, objects, k)
    jitter = rng.choice([0.0, 0.0, 0.05, 0.3], size=k)
    start = np.clip(lo[which] + (jitter * ln[which] * rng.uniform(-1, 1, k)).astype(np.int64), 0, n - 1)
    end = np.clip(lo[which] + ln[which] + (jitter * ln[which] * rng.uniform(-1, 1, k)).astype(np.int64), start + 1, n)
    t = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    rows = _lib.rle_to_rows(t(start), t(end), t(np.arange(k + 1)), n)
    return rows, rng.integers(0, 16, k) / 16.0


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def torch_greedy(h):
    removed = torch.zeros(h.shape[0], dtype=torch.bool, device=dev)
    for r in range(h.shape[0]):
        removed |= h[r] & ~removed[r]
    return ~removed


res = {"bench": "assemble_scene", "device": torch.cuda.get_device_name(0), "points": n, "thres": args.thres,
       "rounds": args.rounds, "torch_rounds": args.torch_rounds, "rows": {},
       "note": "wall clock around one call, device idle before and after; legs interleaved round by round"}
thr = torch.tensor(args.thres, dtype=torch.float32, device=dev)
with _lib.launch_stream():
    for k in args.rows:
        rows, score = make_rows(k)
        cls = np.zeros(k, np.int32)
        order = np.lexsort((np.arange(k), -score))
        order_dev = torch.from_numpy(order.astype(np.int32)).to(dev)
        area = _lib.popcount_rows(rows)
        inter = _lib.cross_popcount(rows, rows)
        w = (k + 63) // 64
        sup = torch.empty((k, w), dtype=torch.int64, device=dev)
        keep_bits = torch.empty(w, dtype=torch.int64, device=dev)
        by = torch.empty(k, dtype=torch.int32, device=dev)
        n_kept = torch.empty(1, dtype=torch.int32, device=dev)
        pairs = lambda: call("bff_nms_pairs", _ptr(inter), _ptr(area), _ptr(order_dev), None, k, 0, args.thres, _ptr(sup))
        greedy = lambda: call("bff_nms_greedy", _ptr(sup), k, _ptr(keep_bits), _ptr(by), _ptr(n_kept))
        legs = {"gram": lambda: _lib.cross_popcount(rows, rows), "pairs": pairs, "greedy": greedy,
                "nms_rows": lambda: assemble.nms_rows(rows, n, score, cls, args.thres)}
        times = {name: [] for name in legs}
        for rnd in range(args.rounds + 2):             # two warm-up rounds
            for name, fn in legs.items():
                ms, _ = wall(fn)
                if rnd >= 2:
                    times[name].append(ms)
        out = {name: summary(v) for name, v in times.items()}
        kept, _ = assemble.nms_rows(rows, n, score, cls, args.thres)
        out.update(kept=len(kept), slices=_lib.load().bff_cross_popcount_slices(k, k, rows.shape[1]))
        # the torch statement of the same work
        dense = _lib.unpack_rows(rows, n)[torch.from_numpy(order).to(dev)].to(torch.float32)

        def torch_pairs(g):
            a = torch.diagonal(g)
            v = g / (a[:, None] + a[None, :] - g)
            return torch.triu(~(v < thr), 1)

        t_times = {"gram": [], "pairs": [], "greedy": []}
        for rnd in range(args.torch_rounds + 1):       # one warm-up round
            ms_g, g = wall(lambda: dense @ dense.T)
            ms_p, h = wall(lambda: torch_pairs(g))
            ms_w, keep = wall(lambda: torch_greedy(h))
            if rnd >= 1:
                t_times["gram"].append(ms_g), t_times["pairs"].append(ms_p), t_times["greedy"].append(ms_w)
        out["torch"] = {name: summary(v) for name, v in t_times.items()}
        out["torch"]["keep_equal"] = bool(np.array_equal(order[keep.cpu().numpy()], kept.numpy()))
        out["torch_over_device"] = {name: round(out["torch"][name]["median_ms"] / out[name]["median_ms"], 1) for name in t_times}
        del dense, g, h
        res["rows"][str(k)] = out

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
