#!/usr/bin/env python3
"""What clustering instances by density does to AP, on generator scenes.

    python scripts/eval_cluster_instances.py [--seeds 0 1 2 3] [--eps 0.15 0.3] [--min-samples 8] [--min-points 20]
                                             [--out profiles/cluster_instances/ap_cluster_instances.json]

Each scene (synthetic.make_scene, cut_masks=False: a 2-D mask is the whole silhouette of its cuboid) goes through
project_scene + refine_class once; the final instances are then scored four ways by evaluation.Evaluator against the
generator's own ground truth (SceneInputs.point_object: every cuboid an instance of the query class, the room an instance
of a second valid class, every confidence 1.0 as in the per-class evaluation script):

    as they are              the final instances
    clustered                density.cluster_instances of them
    over-merged              the final instances OR-ed in pairs (rows 0|1, 2|3, ...): two objects of one class in one instance
    over-merged, clustered   density.cluster_instances of those

The seeds, the scenes and the scoring are scripts/eval_split_instances.py's, so the two tables sit side by side.  The
scenes of a leg are the scans of one evaluation.  These are generator scenes, not a dataset: the numbers compare the legs
with each other on this geometry and say nothing about ScanNet; cluster_eps and cluster_min_samples stay untuned.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beyond_fixed_forms_amd import _lib, density, spatial  # noqa: E402
from beyond_fixed_forms_amd.config import Config  # noqa: E402
from beyond_fixed_forms_amd.evaluation import Evaluator  # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene  # noqa: E402
from beyond_fixed_forms_amd.refinement import TextSimilarity, refine_class  # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, make_text_bank, with_sensor_depth  # noqa: E402

QUERY = "table"
LABELS = [QUERY, "room"]
DEV = "cuda:0"
SCENE = dict(shape="c1", n_views=24, distinct_masks=True, cut_masks=False)        # 20 000 points, 480 x 640, 5 masks a view


def over_merged(fin):
    """The instances OR-ed in pairs; the class and the confidence of a pair are its first member's."""
    out = copy.copy(fin)
    if fin.rows is None or fin.rows.shape[0] < 2:
        return out
    k = int(fin.rows.shape[0])
    pairs = fin.rows[0:k - k % 2:2] | fin.rows[1:k:2]
    first = list(range(0, k - k % 2, 2)) + ([k - 1] if k % 2 else [])
    out.rows = torch.cat([pairs, fin.rows[k - k % 2:]])                 # an odd last instance stays as it is
    out.final_class = [fin.final_class[i] for i in first]
    out.conf = spatial._take(fin.conf, torch.tensor(first))
    return out


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
    ap.add_argument("--eps", type=float, nargs="+", default=[0.15, 0.3], help="cluster_eps values, metres (untuned)")
    ap.add_argument("--min-samples", type=int, default=8, help="cluster_min_samples (untuned)")
    ap.add_argument("--min-points", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_instances", "ap_cluster_instances.json"))
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
    trip = []
    for seed, scene in scenes.items():
        sc = with_sensor_depth(scene)
        trip.append((sc.scene_id, sc.stage1, project_scene(sc, cfg, DEV, return_result=True)))
    final = refine_class(trip, cfg, QUERY, sim, DEV)
    as_is = {seed: final[scene.scene_id] for seed, scene in scenes.items()}
    merged = {seed: over_merged(fin) for seed, fin in as_is.items()}
    legs = {"as they are": score(as_is, scenes, truth), "over-merged": score(merged, scenes, truth)}
    for eps in args.eps:
        keys = dict(cluster_eps=eps, cluster_min_samples=args.min_samples, cluster_min_points=args.min_points, cluster_mode="split")
        indices = {seed: density.density_index(scene.points, eps, DEV) for seed, scene in scenes.items()}
        for name, src in (("clustered", as_is), ("over-merged, clustered", merged)):
            parts = {seed: density.cluster_instances(indices[seed], fin, keys) for seed, fin in src.items()}
            legs[f"{name} (cluster_eps {eps}, cluster_min_samples {args.min_samples}, cluster_min_points {args.min_points})"] = \
                dict(score(parts, scenes, truth), config=keys)
    for name, leg in legs.items():
        print(f"{name:<90} AP {leg['ap']:.3f}  AP50 {leg['ap50']:.3f}  AP25 {leg['ap25']:.3f}   instances {leg['instances']}")
    n_gt = [int((t.vert_count[t.label_ids == 1] >= 100).sum()) for t in truth.values()]
    out = {"what": "AP of the query class on generator scenes, final instances as they are / clustered by density / over-merged / both; "
                   "not a dataset result", "scene": dict(SCENE, seeds=args.seeds, query=QUERY),
           "ground_truth": "point_object: every cuboid an instance of the query class, the room a second class",
           "confidence": 1.0, "gt_instances_per_scene": n_gt, "legs": legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
