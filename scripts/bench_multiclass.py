#!/usr/bin/env python3
"""Multi-class projection vs one run per class (DESIGN.md "Multi-class projection").

One c2-shaped scene; K classes derived from it, each keeping a deterministic ~15 % of the mask_2d frames (about the
real V / V_all) and its own query string.  The same (class, scene) pairs are timed both ways, interleaved in one
process:
  single  K single-class scenes: each uploads the scene and runs the fused sweep over its mask AND viewed frames;
  multi   the scene's geometry once (cloud, poses, depth, viewed counts by bff_count_viewed), then K class tables.
Two legs: `resident` (scenes already on the device; single = K scene calls, multi = one viewed-count sweep + K scene
calls) and `host` (from host arrays: pipeline.project_stream vs pipeline.project_classes_stream, ingestion included).
Also times bff_count_viewed alone for several frame tiles.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from beyond_fixed_forms_amd import _lib, pipeline  # noqa: E402
from beyond_fixed_forms_amd.config import Config  # noqa: E402
from beyond_fixed_forms_amd.ingest import prepare_class_fast, prepare_geometry_fast, prepare_scene_fast  # noqa: E402
from beyond_fixed_forms_amd.projection import projection_back, projection_front  # noqa: E402
from beyond_fixed_forms_amd.scene import SceneClasses, count_geometry_viewed, viewed_frame_ids  # noqa: E402
from beyond_fixed_forms_amd.synthetic import class_scene, derive_classes, make_scene, with_sensor_depth  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def resident_pairs(items, cfg, streams):
    """Project (DeviceScene, geometry-or-None) pairs pipelined over the scene streams; a geometry's viewed counts are
    recomputed first (its share of the multi-class work)."""
    def front(i):
        ds, geom = items[i]
        st = streams[i % len(streams)]
        with _lib.on_stream(st):
            if geom is not None:
                count_geometry_viewed(geom, geom.viewed_ids)
            return projection_front(ds, cfg)

    def back(i, fr):
        with _lib.on_stream(streams[i % len(streams)]):
            projection_back(fr, want_groups=False)

    for _ in pipeline.pipelined(len(items), front, back):
        pass


def tile_sweep(geom, cfg, ids, tiles, reps=20):
    """bff_count_viewed alone over `ids`, kernel time per call (events around `reps` back-to-back launches)."""
    idx = np.array([geom.slot[f] for f in ids])
    inv = torch.from_numpy(np.ascontiguousarray(geom.inv_pose_host[idx])).cuda()
    d_idx = torch.from_numpy(idx.astype(np.int32)).cuda()
    out = torch.zeros(geom.n_points, dtype=torch.int32, device="cuda")
    res = {}
    for fpb in tiles:
        call = lambda: _lib.count_viewed(geom.xyz, geom.n_points, inv, geom.cam_intr, geom.sweep_depth, d_idx, geom.height,
                                         geom.width, 0.08, out, tile_bounds=geom.tile_bounds, depth_size=geom.depth_size,
                                         frames_per_block=fpb)
        call()
        best = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            e1.synchronize()
            best.append(e0.elapsed_time(e1) / reps)
        res[str(fpb)] = round(min(best), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--fraction", type=float, default=0.15)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=4, help="copies of the scene per timed host run")
    ap.add_argument("--tiles", default="0,1,2,4,8,16,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda:0")
    scene = make_scene(args.shape, seed=0, device=dev, cut_masks=False, n_objects=40, distinct_masks=True)
    cfg = Config.with_defaults(width_2d=scene.width, height_2d=scene.height)
    masks = derive_classes(scene, k=args.classes, fraction=args.fraction, seed=0)
    classes = list(masks)
    viewed = viewed_frame_ids(scene.color_files, cfg.downsample_ratio)
    # host form: depth as the sensor's uint16 PNG frames at half the working resolution (ScanNet), as bench.py's
    # host-inclusive leg; the scene's frames in one pinned block is not assumed here (decoded frames in pageable memory)
    host = with_sensor_depth(scene)
    host.mask_2d = [dict(fr, confidences=fr["confidences"].cpu()) for fr in host.mask_2d]
    hmasks = {c: [dict(fr, confidences=fr["confidences"].cpu()) for fr in m] for c, m in masks.items()}
    streams = pipeline.scene_streams(dev)
    n_pairs = len(classes)

    # ---- device-resident leg
    singles = [(prepare_scene_fast(class_scene(host, hmasks[c]), cfg, dev), None) for c in classes]
    geom = prepare_geometry_fast(host, cfg, [hmasks[c] for c in classes], dev)
    geom.viewed_ids = viewed
    multis = [(prepare_class_fast(geom, hmasks[c], cfg), None) for c in classes]
    multis[0] = (multis[0][0], geom)                  # the one viewed-count sweep of the scene rides with class 0
    torch.cuda.synchronize()
    for _ in range(2):                                # warm-up: workspaces, allocator pools, tap tables
        resident_pairs(singles, cfg, streams)
        resident_pairs(multis, cfg, streams)
    t_res = {"single": [], "multi": []}
    for _ in range(args.rounds):
        t_res["single"].append(timed(lambda: resident_pairs(singles * args.repeat, cfg, streams)))
        t_res["multi"].append(timed(lambda: resident_pairs(multis * args.repeat, cfg, streams)))

    # ---- host leg: project_stream over K single-class scenes vs project_classes_stream over one scene x K classes
    single_src = [class_scene(host, hmasks[c]) for _ in range(args.repeat) for c in classes]
    multi_src = [(SceneClasses(host, hmasks), classes) for _ in range(args.repeat)]
    noop = lambda *a: None
    run_single = lambda: pipeline.project_stream(single_src, cfg, dev, noop, with_stage1=False)
    run_multi = lambda: pipeline.project_classes_stream(multi_src, cfg, dev, noop)
    run_single(); run_multi()
    t_host = {"single": [], "multi": []}
    for _ in range(args.rounds):
        t_host["single"].append(timed(run_single))
        t_host["multi"].append(timed(run_multi))

    pairs = n_pairs * args.repeat
    rate = lambda ts: round(pairs / statistics.median(ts), 2)
    mask_frames = sorted({fr["frame_id"][:-4] for m in masks.values() for fr in m}, key=int)
    tiles = [int(t) for t in args.tiles.split(",")]
    out = {
        "metric": "multiclass_pairs_per_s", "shape": args.shape, "classes": n_pairs,
        "frames_per_class": [len(masks[c]) for c in classes], "mask_frames_all": len(scene.mask_2d),
        "viewed_frames": len(viewed), "n_points": int(scene.points.shape[0]), "pairs_per_run": pairs,
        "resident": {"single": rate(t_res["single"]), "multi": rate(t_res["multi"]),
                     "speedup": round(statistics.median(t_res["single"]) / statistics.median(t_res["multi"]), 3)},
        "host": {"single": rate(t_host["single"]), "multi": rate(t_host["multi"]),
                 "speedup": round(statistics.median(t_host["single"]) / statistics.median(t_host["multi"]), 3)},
        "count_viewed_ms": {"viewed_frames": tile_sweep(geom, cfg, viewed, tiles),
                            "all_frames": tile_sweep(geom, cfg, list(dict.fromkeys(mask_frames + viewed)), tiles)},
        "depth": f"uint16 {host.depths_raw[viewed[0]].shape} sensor frames, layout {os.environ.get('BFF_DEPTH_TILES', 'f32')}",
        "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
