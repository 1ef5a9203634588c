#!/usr/bin/env python3
"""What the source of the depth frames does to AP, on generator scenes.

    python scripts/eval_depth_sources.py [--seeds 0 1 2 3] [--out profiles/eval/ap_depth_sources.json]

Each scene (synthetic.make_scene, cut_masks=False: a 2-D mask is the whole silhouette of its cuboid) goes through
project_scene + refine_class five times -- sensor depth, depth rendered from the cloud at stride 8, splatted at stride 4
with a 0.02 m footprint, rasterised from the scene's mesh at stride 4, the same clipped at 0.05 m -- and every leg is
scored by evaluation.Evaluator against the generator's own ground truth (SceneInputs.point_object): every cuboid is
an instance of the query class, the room an instance of a second valid class, every confidence 1.0 as in the per-class
evaluation script.  The scenes of a leg are the scans of one evaluation.

These are generator scenes, not a dataset: the numbers compare the depth sources with each other on this geometry and
say nothing about ScanNet.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beyond_fixed_forms_amd import _lib  # noqa: E402
from beyond_fixed_forms_amd.config import Config  # noqa: E402
from beyond_fixed_forms_amd.evaluation import Evaluator  # noqa: E402
from beyond_fixed_forms_amd.projection import project_scene  # noqa: E402
from beyond_fixed_forms_amd.refinement import TextSimilarity, refine_class  # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh, make_text_bank, with_sensor_depth  # noqa: E402

QUERY = "table"
LABELS = [QUERY, "room"]
DEV = "cuda:0"
SCENE = dict(shape="c1", n_views=24, distinct_masks=True, cut_masks=False)        # 20 000 points, 480 x 640, 5 masks a view
MESH_VERTICES = 20_000

LEGS = {
    "sensor depth": dict(),
    "depth_from_cloud: 8": dict(depth_from_cloud=8),
    "depth_from_cloud: 4, cloud_splat_radius: 0.02": dict(depth_from_cloud=4, cloud_splat_radius=0.02),
    "depth_from_mesh: 4": dict(depth_from_mesh=4),
    "depth_from_mesh: 4, mesh_near_clip: 0.05": dict(depth_from_mesh=4, mesh_near_clip=0.05),
}


def leg_scene(scene, seed, keys):
    """The scene as the leg's depth source sees it: sensor frames (16-bit, half resolution), or none at all."""
    if not keys:
        return with_sensor_depth(scene)
    out = copy.copy(scene)
    out.depths, out.depths_raw, out.depth_staged = {}, None, None
    if "depth_from_mesh" in keys:
        out.mesh_vertices, out.faces = make_scene_mesh(seed, n_vertices=MESH_VERTICES)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "ap_depth_sources.json"))
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
    legs = {}
    for name, keys in LEGS.items():
        t0 = time.perf_counter()
        cfg = Config.with_defaults(width_2d=scenes[args.seeds[0]].width, height_2d=scenes[args.seeds[0]].height, **keys)
        trip = []
        for seed, scene in scenes.items():
            sc = leg_scene(scene, seed, keys)
            trip.append((sc.scene_id, sc.stage1, project_scene(sc, cfg, DEV, return_result=True)))
        final = refine_class(trip, cfg, QUERY, sim, DEV)
        leg = Evaluator(LABELS, device=DEV)
        n_pred = []
        for seed, scene in scenes.items():
            fin = final[scene.scene_id]
            preds = [{"scan_id": scene.scene_id, "label_id": float(LABELS.index(c) + 1), "conf": 1.0} for c in fin.final_class]
            n_pred.append(len(preds))
            leg.add_scan(preds, ground_truth=truth[seed], pred_rows=fin.rows if preds else None)
        cls = leg.evaluate()["classes"][QUERY]
        legs[name] = {"config": keys, "ap": float(cls["ap"]), "ap50": float(cls["ap50%"]), "ap25": float(cls["ap25%"]),
                      "rc": float(cls["rc"]), "rc50": float(cls["rc50%"]), "rc25": float(cls["rc25%"]),
                      "stage2_instances": [int(t[2].rows.shape[0]) for t in trip], "final_instances": n_pred,
                      "seconds": round(time.perf_counter() - t0, 2)}
        print(f"{name:<50} AP {cls['ap']:.3f}  AP50 {cls['ap50%']:.3f}  AP25 {cls['ap25%']:.3f}   final instances {n_pred}")
    n_gt = [int((t.vert_count[t.label_ids == 1] >= 100).sum()) for t in truth.values()]
    out = {"what": "AP of the query class on generator scenes, per depth source; not a dataset result",
           "scene": dict(SCENE, seeds=args.seeds, mesh_vertices=MESH_VERTICES, query=QUERY),
           "ground_truth": "point_object: every cuboid an instance of the query class, the room a second class",
           "confidence": 1.0, "gt_instances_per_scene": n_gt, "legs": legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
