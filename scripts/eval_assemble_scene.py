#!/usr/bin/env python3
"""What assembling a scene from several classes' files does to AP, on generator scenes.

    python scripts/eval_assemble_scene.py [--seeds 0 1 2 3] [--thres 0.3 0.5 0.7] [--keep 0.9]
                                          [--out profiles/assemble_scene/ap_assemble_scene.json]

Each scene (synthetic.make_scene, cut_masks=False: a 2-D mask is the whole silhouette of its cuboid) goes through
project_scene + refine_class once.  A second class's file is imitated the way the refinement produces one: every final
instance once more, bit for bit (a matched stage-1 mask handed to two classes) or with --keep of its points (a near
duplicate), at a lower confidence.  The legs, scored by evaluation.Evaluator against the generator's own ground truth
(SceneInputs.point_object: every cuboid an instance of the query class, the room an instance of a second valid class),
every instance counted for the query class and every confidence 1.0 as in the per-class evaluation script:

    as they are                     the final instances of the one class
    both files, no NMS              assemble_scene of the two files with assemble_nms_thres off: every duplicate is a false positive
    both files, NMS                 assemble_scene with assemble_nms_thres (both criteria)
    both files, NMS, exclusive      the same with assemble_exclusive

The seeds, the scenes and the scoring are scripts/eval_cluster_instances.py's.  These are generator scenes, not a dataset:
the numbers compare the legs with each other on this geometry and say nothing about ScanNet; assemble_nms_thres stays
untuned.
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
from beyond_fixed_forms_amd import _lib, assemble  # noqa: E402
from beyond_fixed_forms_amd.config import Config  # noqa: E402
from beyond_fixed_forms_amd.evaluation import Evaluator  # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene  # noqa: E402
from beyond_fixed_forms_amd.refinement import TextSimilarity, refine_class  # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, make_text_bank, with_sensor_depth  # noqa: E402

QUERY = "table"
LABELS = [QUERY, "room"]
DEV = "cuda:0"
SCENE = dict(shape="c1", n_views=24, distinct_masks=True, cut_masks=False)        # 20 000 points, 480 x 640, 5 masks a view


def second_file(fin, n_points, keep, seed):
    """The final instances once more, each with `keep` of its points, at half the confidence."""
    out = copy.copy(fin)
    if fin.rows is None:
        return out
    gen = torch.Generator(device=DEV).manual_seed(seed)
    dense = _lib.unpack_rows(fin.rows, n_points)
    if keep < 1.0:
        dense = dense & (torch.rand(dense.shape, device=DEV, generator=gen) < keep)
    out.rows = _lib.pack_rows(dense.contiguous())
    out.conf = torch.as_tensor([0.5 * float(c) for c in fin.conf])
    return out


def score(rows_of, scenes, truth):
    leg = Evaluator(LABELS, device=DEV)
    n_pred = []
    for seed, scene in scenes.items():
        rows = rows_of[seed]
        k = 0 if rows is None else int(rows.shape[0])
        preds = [{"scan_id": scene.scene_id, "label_id": 1.0, "conf": 1.0} for _ in range(k)]
        n_pred.append(k)
        leg.add_scan(preds, ground_truth=truth[seed], pred_rows=rows if k else None)
    cls = leg.evaluate()["classes"][QUERY]
    return {"ap": float(cls["ap"]), "ap50": float(cls["ap50%"]), "ap25": float(cls["ap25%"]), "rc": float(cls["rc"]),
            "rc50": float(cls["rc50%"]), "rc25": float(cls["rc25%"]), "instances": n_pred}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--thres", type=float, nargs="+", default=[0.3, 0.5, 0.7], help="assemble_nms_thres values (untuned)")
    ap.add_argument("--keep", type=float, nargs="+", default=[1.0, 0.9], help="share of its points a duplicate keeps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_scene", "ap_assemble_scene.json"))
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
    n_of = {seed: int(scene.points.shape[0]) for seed, scene in scenes.items()}
    legs = {"as they are": score({seed: fin.rows for seed, fin in as_is.items()}, scenes, truth)}
    for keep in args.keep:
        again = {seed: second_file(fin, n_of[seed], keep, seed) for seed, fin in as_is.items()}
        configs = [("no NMS", {})]
        for thres in args.thres:
            for criterion in assemble.CRITERIA:
                keys = dict(assemble_nms_thres=thres, assemble_criterion=criterion)
                configs.append((f"NMS {criterion} {thres}", keys))
                if criterion == "iou":
                    configs.append((f"NMS {criterion} {thres}, exclusive", dict(keys, assemble_exclusive=True)))
        for name, keys in configs:
            rows = {seed: assemble.assemble_scene({QUERY: as_is[seed], f"{QUERY} again": again[seed]}, n_of[seed], keys, DEV).rows
                    for seed in scenes}
            legs[f"both files (duplicates keep {keep}), {name}"] = dict(score(rows, scenes, truth), config=keys, keep=keep)
    for name, leg in legs.items():
        print(f"{name:<70} AP {leg['ap']:.3f}  AP50 {leg['ap50']:.3f}  AP25 {leg['ap25']:.3f}   instances {leg['instances']}")
    n_gt = [int((t.vert_count[t.label_ids == 1] >= 100).sum()) for t in truth.values()]
    out = {"what": "AP of the query class on generator scenes: one class's final instances as they are / a second file of "
                   "duplicates assembled with them, without and with the NMS; not a dataset result",
           "scene": dict(SCENE, seeds=args.seeds, query=QUERY),
           "ground_truth": "point_object: every cuboid an instance of the query class, the room a second class",
           "confidence": 1.0, "gt_instances_per_scene": n_gt, "legs": legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
