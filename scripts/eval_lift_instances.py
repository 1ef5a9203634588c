#!/usr/bin/env python3
"""What running the projection stage on a voxel subsample and lifting its instances back costs in AP and saves in time,
on generator scenes.

    python scripts/eval_lift_instances.py [--seeds 0 1 2 3] [--voxels 0.05 0.1 0.15 0.2]
                                          [--out profiles/lift_instances/ap_lift_instances.json]

Each scene (synthetic.make_scene, cut_masks=False: a 2-D mask is the whole silhouette of its cuboid) goes through
project_scene; the legs are scored by evaluation.Evaluator against the generator's own ground truth
(SceneInputs.point_object: every cuboid an instance of the query class, the room an instance of a second valid class,
every confidence 1.0 as in the per-class evaluation script):

    full                          the projection at all N points
    small                         the projection on lift.subsample's points, scored on those points' own ground truth
    lifted                        the small run's instances carried to the full cloud (lift.nearest, lift.lift_instances,
                                  lift_max_dist = 2 x subsample_voxel), scored like "full"

With the sizes of the sub-clouds and the wall clock of one project_scene call per scene, device idle before and after
(median of --repeats calls after a warm-up; the call prepares the scene on the host too).  The scenes of a leg are the
scans of one evaluation.  These are generator scenes, not a dataset: the numbers compare the legs with each other on this
geometry and say nothing about ScanNet; subsample_voxel stays untuned.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beyond_fixed_forms_amd import _lib, lift  # noqa: E402
from beyond_fixed_forms_amd.config import Config  # noqa: E402
from beyond_fixed_forms_amd.evaluation import Evaluator  # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene  # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth  # noqa: E402

QUERY = "table"
LABELS = [QUERY, "room"]
DEV = "cuda:0"
SCENE = dict(shape="c1", n_views=24, distinct_masks=True, cut_masks=False)        # 20 000 points, 480 x 640, 5 masks a view


def ground_truth(evaluator, obj):
    # scannet200's `- 2 + 1`: label id = sem - 1, so the cuboids (label 1) are sem 2 and the room (label 2) is sem 3
    return evaluator.prepare_ground_truth(np.where(obj >= 0, 2, 3).astype(np.int32), (obj + 1).astype(np.int32))


def score(results, scenes, truth):
    leg = Evaluator(LABELS, device=DEV)
    n_pred = []
    for seed, scene in scenes.items():
        res = results[seed]
        preds = [{"scan_id": scene.scene_id, "label_id": float(LABELS.index(c) + 1), "conf": 1.0} for c in res.final_class]
        n_pred.append(len(preds))
        leg.add_scan(preds, ground_truth=truth[seed], pred_rows=res.rows if preds else None)
    cls = leg.evaluate()["classes"][QUERY]
    return {"ap": float(cls["ap"]), "ap50": float(cls["ap50%"]), "ap25": float(cls["ap25%"]), "instances": n_pred}


def project(scenes, cfg, repeats):
    """-> ({seed: Stage2Result}, the median wall clock of one project_scene call per scene, ms)."""
    results, ms = {}, []
    for seed, scene in scenes.items():
        times = []
        for r in range(repeats + 1):                       # one warm-up call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[seed] = project_scene(scene, cfg, DEV, return_result=True)
            torch.cuda.synchronize()
            if r:
                times.append((time.perf_counter() - t0) * 1e3)
        ms.append(round(statistics.median(times), 3))
    return results, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.05, 0.1, 0.15, 0.2], help="subsample_voxel values (untuned)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_instances", "ap_lift_instances.json"))
    args = ap.parse_args()
    _lib.load()
    scenes = {seed: with_sensor_depth(make_scene(seed=seed, query=QUERY, device=DEV, **SCENE)) for seed in args.seeds}
    evaluator = Evaluator(LABELS, device=DEV)
    truth = {seed: ground_truth(evaluator, scene.point_object) for seed, scene in scenes.items()}
    first = scenes[args.seeds[0]]
    cfg = Config.with_defaults(width_2d=first.width, height_2d=first.height)
    full, full_ms = project(scenes, cfg, args.repeats)
    legs = {"full": dict(score(full, scenes, truth), points=[int(s.points.shape[0]) for s in scenes.values()],
                         project_scene_ms=full_ms)}
    for voxel in args.voxels:
        keys = dict(cfg, subsample_voxel=voxel)
        radius = lift.lift_max_dist(keys)
        samples = {seed: lift.subsample(scene.points, lift.subsample_voxel(keys), DEV).cpu().numpy() for seed, scene in scenes.items()}
        smalls = {seed: dataclasses.replace(scene, points=scene.points[samples[seed]], stage1=None,
                                            point_object=scene.point_object[samples[seed]]) for seed, scene in scenes.items()}
        small_truth = {seed: ground_truth(evaluator, s.point_object) for seed, s in smalls.items()}
        small, small_ms = project(smalls, cfg, args.repeats)
        lifted, lost = {}, []
        for seed, scene in scenes.items():
            nn = lift.nearest(lift.nearest_index(smalls[seed].points, radius, DEV), scene.points)
            lost.append(int((nn < 0).sum()))
            lifted[seed] = lift.lift_instances(nn, small[seed], len(samples[seed]), scene.points.shape[0])
        sizes = [int(len(s)) for s in samples.values()]
        legs[f"small, voxel {voxel}"] = dict(score(small, smalls, small_truth), points=sizes, project_scene_ms=small_ms)
        legs[f"lifted, voxel {voxel}"] = dict(score(lifted, scenes, truth), lift_max_dist=radius, points_without_source=lost)
    for name, leg in legs.items():
        print(f"{name:<24} AP {leg['ap']:.3f}  AP50 {leg['ap50']:.3f}  AP25 {leg['ap25']:.3f}   instances {leg['instances']}"
              f"   {leg.get('points', '')} {leg.get('project_scene_ms', '')}")
    out = {"what": "AP of the query class on generator scenes: the projection stage at full resolution, on a voxel subsample, "
                   "and the subsample's instances lifted to the full cloud; not a dataset result",
           "scene": dict(SCENE, seeds=args.seeds, query=QUERY), "device": torch.cuda.get_device_name(0),
           "ground_truth": "point_object: every cuboid an instance of the query class, the room a second class",
           "confidence": 1.0, "project_scene_ms": "wall clock of one call, device idle before and after, host preparation "
                                                  f"included; median of {args.repeats} calls after a warm-up, per scene",
           "legs": legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
