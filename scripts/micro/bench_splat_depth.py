"""Depth frames rendered from the cloud with a surfel footprint per point (bff_render_splat_depth_u16) on a
config-2-sized scene: bench_mesh_depth.py's cloud (the generator's room and cuboids tessellated to about 200 k vertices,
which are the scene's cloud), 300 frames, 968 x 1296, strides 2, 4 and 8, radius 0.02 m.  The legs, interleaved round by
round, device events around `inner` back-to-back calls:

  splat_stride_s   bff_render_splat_depth_u16 (fill of the scratch, splat kernel, narrowing kernel), with the culling table
  points_stride_s  bff_render_depth_u16 on the same cloud and frames (with its culling table): one texel per point
  mesh_stride_s    bff_render_mesh_depth_u16 on the triangles the cloud was tessellated from

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_splat_depth.py --rounds 10 --out profiles/render_depth/bench_splat_depth.json
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
from beyond_fixed_forms_amd.scene import checked_faces, mesh_for_render, prepare_geometry, rendered_depth_size   # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh, with_sensor_depth                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
ap.add_argument("--strides", type=int, nargs="+", default=[2, 4, 8])
ap.add_argument("--radius", type=float, default=0.02, help="splat radius, metres")
ap.add_argument("--views", type=int, default=None, help="frames of the scene (default: config 2's 300)")
ap.add_argument("--vertices", type=int, default=200_000, help="points the surfaces are tessellated to (about)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_splat_depth: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

scene = with_sensor_depth(make_scene("c2", seed=0, n_views=args.views, device=dev))       # poses; the depth is not used
vertices, faces = make_scene_mesh(seed=0, n_vertices=args.vertices)
scene.points = np.concatenate([vertices, np.zeros_like(vertices)], axis=1)                 # the cloud is the vertex array
h, w = scene.height, scene.width
geom = prepare_geometry(scene, Config.with_defaults(width_2d=w, height_2d=h), [scene.mask_2d], device=dev, with_viewed=False)
n, f = geom.n_points, len(geom.frame_ids)
_, _, faces_dev = mesh_for_render(torch.as_tensor(checked_faces(faces, n)).to(dev), geom.xyz, n, geom.unsort)
inv = torch.from_numpy(np.ascontiguousarray(geom.inv_pose_host)).to(dev)
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


legs, frames = {}, {}
scratch = torch.empty(max(f * int(np.prod(rendered_depth_size(h, w, s))) for s in args.strides), dtype=torch.int32, device=dev)
for s in args.strides:
    dh, dw = rendered_depth_size(h, w, s)
    out_s = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    out_p = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    out_m = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    frames[s] = (out_s, out_p, out_m)
    legs[f"splat_stride_{s}"] = lambda dh=dh, dw=dw, out=out_s: _lib.call(
        "bff_render_splat_depth_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(inv), k9, f, h, w, dh, dw, args.radius,
        0, _lib._ptr(scratch), _lib._ptr(out), _lib._ptr(geom.tile_bounds))
    legs[f"points_stride_{s}"] = lambda dh=dh, dw=dw, out=out_p: _lib.call(
        "bff_render_depth_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(inv), k9, f, h, w, dh, dw, 0,
        _lib._ptr(scratch), _lib._ptr(out), _lib._ptr(geom.tile_bounds))
    legs[f"mesh_stride_{s}"] = lambda dh=dh, dw=dw, out=out_m: _lib.call(
        "bff_render_mesh_depth_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(faces_dev), faces_dev.shape[0],
        _lib._ptr(inv), k9, f, h, w, dh, dw, 0, _lib._ptr(scratch), _lib._ptr(out))
times = {k: [] for k in legs}
with _lib.launch_stream():
    for rnd in range(args.rounds + 2):                 # two warm-up rounds
        for name, fn in legs.items():
            ms = timed(fn, args.inner)
            if rnd >= 2:
                times[name].append(ms)
torch.cuda.synchronize()

res = {"bench": "splat_depth", "device": torch.cuda.get_device_name(0), "points": n, "triangles": int(faces_dev.shape[0]),
       "frames": f, "image": [h, w], "radius": args.radius, "rounds": args.rounds, "inner": args.inner,
       "lane_box": _lib.load().bff_splat_lane_box(), "legs": {k: summary(v) for k, v in times.items()},
       "note": "device events around `inner` calls, legs interleaved round by round; a call = fill of the scratch, kernel, "
               "narrowing kernel, frames_per_block = the library's choice"}
med = lambda k: res["legs"][k]["median_ms"]
for s in args.strides:
    out_s, out_p, out_m = frames[s]
    held = out_p != 0
    us, up = out_s.to(torch.int32) & 0xffff, out_p.to(torch.int32) & 0xffff
    res[f"stride_{s}"] = {"frame": list(out_s.shape[1:]),
                          "splat_texels_with_depth": round(float((out_s != 0).float().mean()), 4),
                          "points_texels_with_depth": round(float(held.float().mean()), 4),
                          "mesh_texels_with_depth": round(float((out_m != 0).float().mean()), 4),
                          "splat_not_larger_where_points_have_depth": bool(((us <= up) & (us != 0))[held].all()),
                          "splat_over_points_time": round(med(f"splat_stride_{s}") / med(f"points_stride_{s}"), 3),
                          "splat_over_mesh_time": round(med(f"splat_stride_{s}") / med(f"mesh_stride_{s}"), 3)}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
