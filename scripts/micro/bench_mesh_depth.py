"""Depth frames rasterised from a triangle mesh (bff_render_mesh_depth_u16) on a config-2-sized scene: the generator's
room and cuboids tessellated to about as many vertices as the config-2 cloud has points (200 k), 300 frames, 968 x 1296,
strides 2, 4 and 8.  The vertices are the scene's cloud (the faces index it, as ScanNet's do).  The legs, interleaved
round by round, device events around `inner` back-to-back calls:

  mesh_stride_s    bff_render_mesh_depth_u16 (fill of the scratch, raster kernel, narrowing kernel)
  clip_stride_s    bff_render_mesh_depth_clip_u16 at near_clip = 0.05 m on the same mesh and frames: triangles that cross
                   the near plane are rare at this tessellation, so this is the cost of the clip kernel itself
  clip_coarse_stride_s  the same entry point on the room and cuboids as make_scene_mesh gives them (one cell per face, 112
                   triangles): every wall crosses the near plane and covers much of the frame (one stride, --coarse-stride)
  points_stride_s  bff_render_depth_u16 on the same vertices and frames (with its culling table)
  count_viewed     bff_count_viewed on the same vertices and frames, against the scene's uploaded sensor depth: the yardstick

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_mesh_depth.py --rounds 10 --out profiles/render_depth/bench_mesh_depth.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beyond_fixed_forms_amd import _lib                                # noqa: E402
from beyond_fixed_forms_amd.config import Config                        # noqa: E402
from beyond_fixed_forms_amd.scene import (checked_faces, mesh_for_render, padded_points, prepare_geometry,   # noqa: E402
                                          rendered_depth_size)
from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh, with_sensor_depth                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
ap.add_argument("--strides", type=int, nargs="+", default=[2, 4, 8])
ap.add_argument("--views", type=int, default=None, help="frames of the scene (default: config 2's 300)")
ap.add_argument("--vertices", type=int, default=200_000, help="vertices the surfaces are tessellated to (about)")
ap.add_argument("--near-clip", type=float, default=0.05, help="near plane of the clip legs, metres")
ap.add_argument("--coarse-stride", type=int, default=4, help="stride of the leg on the un-tessellated room")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_mesh_depth: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

scene = with_sensor_depth(make_scene("c2", seed=0, n_views=args.views, device=dev))       # poses, uint16 sensor depth
vertices, faces = make_scene_mesh(seed=0, n_vertices=args.vertices)
scene.points = np.concatenate([vertices, np.zeros_like(vertices)], axis=1)                 # the cloud is the vertex array
h, w = scene.height, scene.width
geom = prepare_geometry(scene, Config.with_defaults(width_2d=w, height_2d=h), [scene.mask_2d], device=dev, with_viewed=False)
n, f = geom.n_points, len(geom.frame_ids)
_, _, faces_dev = mesh_for_render(torch.as_tensor(checked_faces(faces, n)).to(dev), geom.xyz, n, geom.unsort)
inv = torch.from_numpy(np.ascontiguousarray(geom.inv_pose_host)).to(dev)
coarse_v, coarse_f = make_scene_mesh(seed=0)                                                # one cell per face
coarse_soa = np.zeros((3, padded_points(coarse_v.shape[0])))
coarse_soa[:, :coarse_v.shape[0]] = coarse_v.T
coarse_soa = torch.from_numpy(coarse_soa).to(dev)
_, _, coarse_faces = mesh_for_render(torch.as_tensor(checked_faces(coarse_f, coarse_v.shape[0])).to(dev), None, 0,
                                     vertices=coarse_soa, n_vertices=coarse_v.shape[0])
d_idx = torch.arange(f, dtype=torch.int32, device=dev)
viewed = torch.zeros(n, dtype=torch.int32, device=dev)
k9 = ctypes.cast((ctypes.c_double * 9)(*[float(v) for v in geom.cam_intr.reshape(-1)]), ctypes.c_void_p)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


legs = {"count_viewed": lambda: _lib.count_viewed(geom.xyz, n, inv, geom.cam_intr, geom.sweep_depth, d_idx, h, w, 0.08, viewed,
                                                  tile_bounds=geom.tile_bounds, depth_size=geom.depth_size)}
frames = {}
scratch = torch.empty(max(f * int(np.prod(rendered_depth_size(h, w, s))) for s in args.strides + [args.coarse_stride]),
                      dtype=torch.int32, device=dev)
for s in args.strides:
    dh, dw = rendered_depth_size(h, w, s)
    out_m = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    out_p = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    out_c = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    frames[s] = (out_m, out_p, out_c)
    legs[f"clip_stride_{s}"] = lambda dh=dh, dw=dw, out=out_c: _lib.call(
        "bff_render_mesh_depth_clip_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(faces_dev), faces_dev.shape[0],
        _lib._ptr(inv), k9, f, h, w, dh, dw, args.near_clip, 0, _lib._ptr(scratch), _lib._ptr(out))
    legs[f"mesh_stride_{s}"] = lambda dh=dh, dw=dw, out=out_m: _lib.call(
        "bff_render_mesh_depth_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(faces_dev), faces_dev.shape[0],
        _lib._ptr(inv), k9, f, h, w, dh, dw, 0, _lib._ptr(scratch), _lib._ptr(out))
    legs[f"points_stride_{s}"] = lambda dh=dh, dw=dw, out=out_p: _lib.call(
        "bff_render_depth_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(inv), k9, f, h, w, dh, dw, 0,
        _lib._ptr(scratch), _lib._ptr(out), _lib._ptr(geom.tile_bounds))
cdh, cdw = rendered_depth_size(h, w, args.coarse_stride)
out_coarse = torch.empty((f, cdh, cdw), dtype=torch.int16, device=dev)
legs[f"clip_coarse_stride_{args.coarse_stride}"] = lambda: _lib.call(
    "bff_render_mesh_depth_clip_u16", _lib._ptr(coarse_soa), coarse_v.shape[0], coarse_soa.shape[1], _lib._ptr(coarse_faces),
    coarse_faces.shape[0], _lib._ptr(inv), k9, f, h, w, cdh, cdw, args.near_clip, 0, _lib._ptr(scratch), _lib._ptr(out_coarse))
times = {k: [] for k in legs}
with _lib.launch_stream():
    for rnd in range(args.rounds + 2):                 # two warm-up rounds
        for name, fn in legs.items():
            ms = timed(fn, args.inner)
            if rnd >= 2:
                times[name].append(ms)
torch.cuda.synchronize()

res = {"bench": "mesh_depth", "device": torch.cuda.get_device_name(0), "vertices": n, "triangles": int(faces_dev.shape[0]),
       "frames": f, "image": [h, w], "rounds": args.rounds, "inner": args.inner, "lane_box": _lib.load().bff_mesh_lane_box(),
       "near_clip": args.near_clip, "coarse_triangles": int(coarse_faces.shape[0]),
       "legs": {k: summary(v) for k, v in times.items()},
       "note": "device events around `inner` calls, legs interleaved round by round; mesh / clip / points = the call as the "
               "ABI defines it (fill of the scratch, kernel, narrowing kernel), frames_per_block = the library's choice"}
med = lambda k: res["legs"][k]["median_ms"]
for s in args.strides:
    out_m, out_p, out_c = frames[s]
    res[f"stride_{s}"] = {"frame": list(out_m.shape[1:]),
                          "mesh_texels_with_depth": round(float((out_m != 0).float().mean()), 4),
                          "points_texels_with_depth": round(float((out_p != 0).float().mean()), 4),
                          "clip_texels_with_depth": round(float((out_c != 0).float().mean()), 4),
                          "clip_equals_mesh_where_mesh_has_depth": bool(((out_c == out_m) | (out_m == 0)).all()),
                          "clip_over_mesh_time": round(med(f"clip_stride_{s}") / med(f"mesh_stride_{s}"), 3),
                          "mesh_over_count_viewed_time": round(med(f"mesh_stride_{s}") / med("count_viewed"), 3),
                          "mesh_over_points_time": round(med(f"mesh_stride_{s}") / med(f"points_stride_{s}"), 3)}

res[f"coarse_stride_{args.coarse_stride}"] = {"frame": [cdh, cdw],
                                              "clip_texels_with_depth": round(float((out_coarse != 0).float().mean()), 4)}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
