"""The label z-buffer (bff_render_labels_u16) beside the depth renderer of the same kernel, and the label image -> run
tables step, on a config-2-sized scene: bench_splat_depth.py's cloud (the generator's room and cuboids tessellated to
about 200 k points), 300 frames, 968 x 1296, strides 2, 4 and 8, radius 0.02 m; the cloud is cut into slabs along x and
every second slab is an instance (40 by default, about half the points stay background).  The legs,
interleaved round by round, device events around `inner` back-to-back calls:

  labels_stride_s      bff_render_labels_u16 with the radius (fill of the scratch, kernel, narrowing to two frames)
  splat_stride_s       bff_render_splat_depth_u16 with the same arguments
  labels0_stride_s     bff_render_labels_u16 with radius 0
  points_stride_s      bff_render_depth_u16 with the same arguments
  runs_stride_s        reproject.label_runs of the frames labels_stride_s rendered (wall clock: it holds a read-back)

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_render_labels.py --rounds 10 --out profiles/render_labels/bench_render_labels.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beyond_fixed_forms_amd import _lib, reproject                      # noqa: E402
from beyond_fixed_forms_amd.config import Config                        # noqa: E402
from beyond_fixed_forms_amd.scene import rendered_depth_size            # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, make_scene_mesh, with_sensor_depth   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
ap.add_argument("--strides", type=int, nargs="+", default=[2, 4, 8])
ap.add_argument("--radius", type=float, default=0.02, help="splat radius, metres")
ap.add_argument("--views", type=int, default=None, help="frames of the scene (default: config 2's 300)")
ap.add_argument("--vertices", type=int, default=200_000, help="points the surfaces are tessellated to (about)")
ap.add_argument("--instances", type=int, default=40, help="instances: the cloud cut into this many slabs along x")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_render_labels: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

scene = with_sensor_depth(make_scene("c2", seed=0, n_views=args.views, device=dev))       # poses; the depth is not used
vertices, _ = make_scene_mesh(seed=0, n_vertices=args.vertices)
scene.points = np.concatenate([vertices, np.zeros_like(vertices)], axis=1)
h, w = scene.height, scene.width
geom = reproject.geometry_for_frames(scene, Config.with_defaults(width_2d=w, height_2d=h), list(scene.poses), dev)
n, f = geom.n_points, len(geom.frame_ids)
# instances: every second slab of the cloud along x (the others are background), in the original point order
x = vertices[:, 0]
slab = np.minimum(((x - x.min()) / max(float(np.ptp(x)), 1e-9) * (2 * args.instances)).astype(np.int64), 2 * args.instances - 1)
dense = np.stack([slab == 2 * k for k in range(args.instances)])
rows = _lib.pack_rows(torch.from_numpy(dense).to(dev))
lab = reproject.point_labels(rows, n, geom.unsort)
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


def wall(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


legs, frames, kinds = {}, {}, {}
scratch = torch.empty(max(f * int(np.prod(rendered_depth_size(h, w, s))) for s in args.strides), dtype=torch.int32, device=dev)
P = _lib._ptr
for s in args.strides:
    dh, dw = rendered_depth_size(h, w, s)
    out_l, out_ld = (torch.empty((f, dh, dw), dtype=torch.int16, device=dev) for _ in range(2))
    out_d = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    frames[s] = (out_l, out_ld, out_d)

    def labels_leg(radius, dh=dh, dw=dw, out_l=out_l, out_ld=out_ld):
        _lib.call("bff_render_labels_u16", P(geom.xyz), n, geom.xyz.shape[1], P(lab), P(inv), k9, f, h, w, dh, dw, radius, 0,
                  P(scratch), P(out_l), P(out_ld), P(geom.tile_bounds))

    legs[f"labels0_stride_{s}"] = lambda leg=labels_leg: leg(0.0)
    legs[f"points_stride_{s}"] = lambda dh=dh, dw=dw, out=out_d: _lib.call(
        "bff_render_depth_u16", P(geom.xyz), n, geom.xyz.shape[1], P(inv), k9, f, h, w, dh, dw, 0, P(scratch), P(out),
        P(geom.tile_bounds))
    legs[f"labels_stride_{s}"] = lambda leg=labels_leg: leg(args.radius)          # after labels0: out_l keeps these frames
    legs[f"splat_stride_{s}"] = lambda dh=dh, dw=dw, out=out_d: _lib.call(
        "bff_render_splat_depth_u16", P(geom.xyz), n, geom.xyz.shape[1], P(inv), k9, f, h, w, dh, dw, args.radius, 0, P(scratch),
        P(out), P(geom.tile_bounds))
    legs[f"runs_stride_{s}"] = lambda out_l=out_l: reproject.label_runs(out_l, h, w, 1, args.instances)
    kinds[f"runs_stride_{s}"] = wall
times = {k: [] for k in legs}
with _lib.launch_stream():
    for rnd in range(args.rounds + 2):                 # two warm-up rounds
        for name, fn in legs.items():
            ms = kinds.get(name, timed)(fn, args.inner if name not in kinds else 1)
            if rnd >= 2:
                times[name].append(ms)
torch.cuda.synchronize()

res = {"bench": "render_labels", "device": torch.cuda.get_device_name(0), "points": n, "instances": args.instances,
       "labelled_points": round(float((lab != 0).float().mean()), 4), "frames": f, "image": [h, w], "radius": args.radius,
       "rounds": args.rounds, "inner": args.inner, "legs": {k: summary(v) for k, v in times.items()},
       "note": "device events around `inner` calls (runs_*: wall clock around one call), legs interleaved round by round; a "
               "render call = fill of the scratch, kernel, narrowing kernel, frames_per_block = the library's choice"}
med = lambda k: res["legs"][k]["median_ms"]
for s in args.strides:
    out_l, out_ld, out_d = frames[s]
    runs, _ = reproject.label_runs(out_l, h, w, 1, args.instances)
    res[f"stride_{s}"] = {"frame": list(out_l.shape[1:]),
                          "depth_half_equals_splat_frame": bool(torch.equal(out_ld, out_d)),
                          "texels_with_label": round(float((out_l != 0).float().mean()), 4),
                          "masks": runs.n_masks, "runs": int(runs.run_start.shape[0]),
                          "labels_over_splat_time": round(med(f"labels_stride_{s}") / med(f"splat_stride_{s}"), 3),
                          "labels0_over_points_time": round(med(f"labels0_stride_{s}") / med(f"points_stride_{s}"), 3)}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
