#!/usr/bin/env python3
"""What snapping instances to superpoints does to AP, on generator scenes.

    python scripts/eval_snap_instances.py [--seeds 0 1 2 3] [--ratio 0.5] [--cell 0.25] [--leak 0.1]
                                          [--out profiles/snap_instances/ap_snap_instances.json]

Each scene (synthetic.make_scene, cut_masks=False: a 2-D mask is the whole silhouette of its cuboid) goes through
project_scene + refine_class; its superpoints are synthetic.make_superpoints (an object's points inside one voxel cell).
The legs are scored by evaluation.Evaluator against the generator's own ground truth (SceneInputs.point_object: every cuboid
an instance of the query class, the room an instance of a second valid class, every confidence 1.0 as in the per-class
evaluation script):

    as they are                   the final instances
    snapped / exclusive           superpoints.snap_instances of them, mode "snap" / "exclusive"
    stage-2 snapped, refined      the stage-2 instances snapped (mode "snap") before refine_class matches them
    ... leak 0.1                  the same three with a tenth of the cells' superpoints straddling the objects in them

The scenes of a leg are the scans of one evaluation.  These are generator scenes, not a dataset: the numbers compare the
legs with each other on this geometry and say nothing about ScanNet; snap_ratio stays untuned.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beyond_fixed_forms_amd import _lib, superpoints  # noqa: E402
from beyond_fixed_forms_amd.config import Config  # noqa: E402
from beyond_fixed_forms_amd.evaluation import Evaluator  # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene  # noqa: E402
from beyond_fixed_forms_amd.refinement import TextSimilarity, refine_class  # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, make_superpoints, make_text_bank, with_sensor_depth  # noqa: E402

QUERY = "table"
LABELS = [QUERY, "room"]
DEV = "cuda:0"
SCENE = dict(shape="c1", n_views=24, distinct_masks=True, cut_masks=False)        # 20 000 points, 480 x 640, 5 masks a view


def score(results, scenes, truth):
    leg = Evaluator(LABELS, device=DEV)
    n_pred = []
    for seed, scene in scenes.items():
        fin = results[seed]
        preds = [{"scan_id": scene.scene_id, "label_id": float(LABELS.index(c) + 1), "conf": 1.0} for c in fin.final_class]
        n_pred.append(len(preds))
        leg.add_scan(preds, ground_truth=truth[seed], pred_rows=fin.rows if preds else None)
    cls = leg.evaluate()["classes"][QUERY]
    return {"ap": float(cls["ap"]), "ap50": float(cls["ap50%"]), "ap25": float(cls["ap25%"]), "rc": float(cls["rc"]),
            "rc50": float(cls["rc50%"]), "rc25": float(cls["rc25%"]), "instances": n_pred}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--ratio", type=float, default=0.5, help="snap_ratio (untuned)")
    ap.add_argument("--cell", type=float, default=0.25, help="make_superpoints' cell, metres")
    ap.add_argument("--leak", type=float, default=0.1, help="share of cells whose superpoint ignores the object id")
    ap.add_argument("--min-points", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snap_instances", "ap_snap_instances.json"))
    args = ap.parse_args()
    _lib.load()
    bank, index = make_text_bank(768, seed=0)
    sim = TextSimilarity(lambda text: bank[index[text.replace(" ", "_")]][None, :], DEV)
    scenes = {seed: make_scene(seed=seed, query=QUERY, device=DEV, **SCENE) for seed in args.seeds}
    evaluator = Evaluator(LABELS, device=DEV)
    truth = {}
    for seed, scene in scenes.items():
        obj = scene.point_object
        # scannet200's `- 2 + 1`: label id = sem - 1, so the cuboids (label 1) are sem 2 and the room (label 2) is sem 3
        truth[seed] = evaluator.prepare_ground_truth(np.where(obj >= 0, 2, 3).astype(np.int32), (obj + 1).astype(np.int32))
    cfg = Config.with_defaults(width_2d=scenes[args.seeds[0]].width, height_2d=scenes[args.seeds[0]].height)
    stage2 = {}
    for seed, scene in scenes.items():
        sc = with_sensor_depth(scene)
        stage2[seed] = (sc, project_scene(sc, cfg, DEV, return_result=True))
    refine = lambda s2: refine_class([(sc.scene_id, sc.stage1, s2[seed]) for seed, (sc, _) in stage2.items()], cfg, QUERY, sim, DEV)
    final = refine({seed: res for seed, (_, res) in stage2.items()})
    as_is = {seed: final[scene.scene_id] for seed, scene in scenes.items()}
    legs = {"as they are": score(as_is, scenes, truth)}
    spp_stats = {}
    for leak in (0.0, args.leak):
        tag = "" if leak == 0.0 else f", leak {leak}"
        indexes = {seed: superpoints.superpoint_index(make_superpoints(scene, args.cell, leak, seed), DEV)
                   for seed, scene in scenes.items()}
        spp_stats[f"leak {leak}"] = {"superpoints": [ix.n_segments for ix in indexes.values()],
                                     "median_points": [float(np.median(ix.size_host)) for ix in indexes.values()]}
        for mode, name in (("snap", "snapped"), ("exclusive", "exclusive")):
            keys = dict(snap_ratio=args.ratio, snap_mode=mode, snap_min_points=args.min_points)
            got = {seed: superpoints.snap_instances(indexes[seed], fin, keys) for seed, fin in as_is.items()}
            legs[f"{name}{tag}"] = dict(score(got, scenes, truth), config=keys)
        keys = dict(snap_ratio=args.ratio, snap_mode="snap", snap_min_points=args.min_points)
        snapped2 = {seed: superpoints.snap_instances(indexes[seed], res, keys) for seed, (_, res) in stage2.items()}
        refined = refine(snapped2)
        legs[f"stage-2 snapped, refined{tag}"] = dict(score({seed: refined[scene.scene_id] for seed, scene in scenes.items()},
                                                           scenes, truth), config=keys)
    for name, leg in legs.items():
        print(f"{name:<40} AP {leg['ap']:.3f}  AP50 {leg['ap50']:.3f}  AP25 {leg['ap25']:.3f}  RC50 {leg['rc50']:.3f}"
              f"   instances {leg['instances']}")
    n_gt = [int((t.vert_count[t.label_ids == 1] >= 100).sum()) for t in truth.values()]
    out = {"what": "AP of the query class on generator scenes, final instances as they are / snapped to superpoints / stage-2 "
                   "snapped before the refinement, with clean and with leaky superpoints; not a dataset result",
           "scene": dict(SCENE, seeds=args.seeds, query=QUERY), "superpoints": dict(cell=args.cell, leak=args.leak, **spp_stats),
           "ground_truth": "point_object: every cuboid an instance of the query class, the room a second class",
           "confidence": 1.0, "gt_instances_per_scene": n_gt, "legs": legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
