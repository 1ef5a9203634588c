"""Depth frames rendered from the cloud (bff_render_depth_u16) on a config-2 scene (200 k points, 300 frames, 968 x 1296),
strides 8 and 2.  Two legs, each interleaved round by round with its yardstick:

  (a) the renderer alone (its fill, the splat kernel and the narrowing kernel) against bff_count_viewed on the same cloud
      and frames -- the same float64 geometry per (point, frame), a depth gather instead of an atomic -- device events
      around `inner` back-to-back launches;
  (b) ingest.prepare_scene_fast from host arrays, the scene's uint16 sensor depth uploaded against no depth at all and
      the frames rendered on the device, host clock around one synchronised call.

One JSON line on stdout (and --out FILE).  There is no pass mark: the numbers are what they are.

    python scripts/micro/bench_render_depth.py --rounds 12 --out profiles/render_depth/bench_render_depth.json
"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from beyond_fixed_forms_amd import _lib                                # noqa: E402
from beyond_fixed_forms_amd.config import Config                        # noqa: E402
from beyond_fixed_forms_amd.ingest import Staging, prepare_scene_fast   # noqa: E402
from beyond_fixed_forms_amd.scene import prepare_geometry, rendered_depth_size    # noqa: E402
from beyond_fixed_forms_amd.synthetic import make_scene, with_sensor_depth        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=12, help="interleaved rounds of every leg (after two warm-up rounds)")
ap.add_argument("--inner", type=int, default=10, help="launches per timed window of a kernel leg (rounds x inner >= 100)")
ap.add_argument("--strides", type=int, nargs="+", default=[8, 2])
ap.add_argument("--views", type=int, default=None, help="frames of the scene (default: config 2's 300)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_render_depth: needs the GPU (there is no CPU path to time)")
dev = torch.device("cuda:0")
_lib.load()

scene = with_sensor_depth(make_scene("c2", seed=0, n_views=args.views, device=dev))       # uint16 484 x 648 per frame
h, w = scene.height, scene.width
cfg = Config.with_defaults(width_2d=w, height_2d=h)
geom = prepare_geometry(scene, cfg, [scene.mask_2d], device=dev, with_viewed=True)
n, f = geom.n_points, len(geom.frame_ids)
inv = torch.from_numpy(np.ascontiguousarray(geom.inv_pose_host)).to(dev)
d_idx = torch.arange(f, dtype=torch.int32, device=dev)
viewed = torch.zeros(n, dtype=torch.int32, device=dev)
k9 = (ctypes.c_double * 9)(*[float(v) for v in geom.cam_intr.reshape(-1)])


def timed(fn, inner):
    """Milliseconds per call: device events around `inner` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def wall(fn):
    """Milliseconds of one call that ends synchronised (host clock)."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


# ---- (a) the renderer alone, buffers allocated once, against the viewed sweep
legs = {"count_viewed": lambda: _lib.count_viewed(geom.xyz, n, inv, geom.cam_intr, geom.sweep_depth, d_idx, h, w, 0.08, viewed,
                                                  tile_bounds=geom.tile_bounds, depth_size=geom.depth_size)}
buffers, shapes = {}, {}
for s in args.strides:
    dh, dw = rendered_depth_size(h, w, s)
    out = torch.empty((f, dh, dw), dtype=torch.int16, device=dev)
    scratch = torch.empty(f * dh * dw, dtype=torch.int32, device=dev)
    buffers[s], shapes[s] = (out, scratch), (dh, dw)

    def render(out=out, scratch=scratch, dh=dh, dw=dw, bounds=geom.tile_bounds):
        _lib.call("bff_render_depth_u16", _lib._ptr(geom.xyz), n, geom.xyz.shape[1], _lib._ptr(inv), ctypes.cast(k9, ctypes.c_void_p),
                  f, h, w, dh, dw, 0, _lib._ptr(scratch), _lib._ptr(out), _lib._ptr(bounds))
    legs[f"render_stride_{s}"] = render
    legs[f"render_stride_{s}_no_culling"] = lambda render=render: render(bounds=None)
kernel = {k: [] for k in legs}
with _lib.launch_stream():
    for rnd in range(args.rounds + 2):                 # two warm-up rounds
        for name, fn in legs.items():
            ms = timed(fn, args.inner)
            if rnd >= 2:
                kernel[name].append(ms)

# ---- (b) prepare_scene_fast from host arrays: uploaded uint16 depth against depth rendered on the device
bare = copy.copy(scene)
bare.depths, bare.depths_raw, bare.depth_staged = {}, None, None
prep = {"uploaded_u16": (scene, cfg, Staging())}
for s in args.strides:
    prep[f"rendered_stride_{s}"] = (bare, Config.with_defaults(width_2d=w, height_2d=h, depth_from_cloud=s), Staging())
host = {k: [] for k in prep}
for rnd in range(args.rounds + 2):
    for name, (sc, c, st) in prep.items():
        ms = wall(lambda: prepare_scene_fast(sc, c, device=dev, staging=st))
        if rnd >= 2:
            host[name].append(ms)

res = {"bench": "render_depth", "device": torch.cuda.get_device_name(0), "points": n, "frames": f, "image": [h, w],
       "rounds": args.rounds, "inner": args.inner, "launches_per_kernel_leg": args.rounds * args.inner,
       "kernel_legs": {k: summary(v) for k, v in kernel.items()}, "prepare_scene_fast": {k: summary(v) for k, v in host.items()},
       "uploaded_depth_bytes": int(sum(d.nbytes for d in scene.depths_raw.values())),
       "note": "kernel_legs: device events around `inner` launches, legs interleaved round by round; render = the call as the "
               "ABI defines it (fill of the scratch, splat kernel, narrowing kernel).  prepare_scene_fast: host clock around "
               "one synchronised call from host arrays, one Staging per leg, legs interleaved."}
med = lambda d, k: res[d][k]["median_ms"]
for s in args.strides:
    out = buffers[s][0]
    legs[f"render_stride_{s}"]()
    torch.cuda.synchronize()
    res[f"stride_{s}"] = {"frame": list(shapes[s]), "texels_with_depth": round(float((out != 0).float().mean()), 4),
                          "render_over_count_viewed_time": round(med("kernel_legs", f"render_stride_{s}") / med("kernel_legs", "count_viewed"), 3),
                          "prepare_rendered_over_uploaded_time": round(med("prepare_scene_fast", f"rendered_stride_{s}") /
                                                                       med("prepare_scene_fast", "uploaded_u16"), 3)}

line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
