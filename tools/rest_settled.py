"""How much of bench.py's resting frame stands settled, and what the frame costs where nothing does.

    python tools/rest_settled.py [--radius R] [--size WxH] [--lights N] [--steps 200] [--warmup 10]

bench.py's config 3 main loop (camera and scene at rest, the 16 point lights riding their spiral at roll_light = 0.002 i), one line of
JSON: the parts of the one launch and how many stood settled (zr_get_rest_settled) after frames 10, 50, 100, 150 and warmup + steps,
then the loop timed as bench.py times it (Mpixel/s).  --radius sets every point light's radius (the scene's is 1.5): raised until
`settled` reads 0 everywhere, the run shows what k_lighting_stand costs a frame it cannot help - to be set beside the same run with
ZR_NO_REST_SETTLE=1 in the environment, which rests through k_lighting_rest.  --size sets the frame's extent (the scene's is
1920x1080): at 128x72 the GPU has next to nothing to do and the loop's time per frame is the host's own cost of a frame.
"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from zeldaengine_amd import dist as zdist, engine, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--radius", type=float, default=None)
ap.add_argument("--size", default=None)
ap.add_argument("--lights", type=int, default=16, help="point lights (the scene's 16)")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()

W, H = (int(x) for x in args.size.lower().split("x")) if args.size else (1920, 1080)
cfg = scenes.config3(width=W, height=H, n_point=args.lights)
if args.radius is not None:
    cfg["point"] = cfg["point"].copy()
    cfg["point"]["Direction"][:, 3] = args.radius
dr = zdist.DistributedRenderer(cfg["width"], cfg["height"], 1024, device_index=0, rank=0, world=1)
engine.load_scene(dr.r, cfg)
dr.r.set_timing_interval(0)


def frame(i):
    dr.r.update_uniforms(cfg["camera"], cfg["dir"], cfg["point"], cfg["spot"], 0.0, 0.002 * i, 0.016 * i)
    dr.frame()


share = {}
n = args.warmup + args.steps
for i in range(n):
    frame(i)
    if i + 1 in (10, 50, 100, 150, n):
        parts, settled = dr.r.rest_settled()
        share[i + 1] = settled
dr.synchronize()
gc.collect(); gc.disable()
for i in range(args.warmup):
    frame(n + i)
dr.synchronize(); torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(args.steps):
    frame(n + args.warmup + i)
dr.synchronize(); torch.cuda.synchronize()
el = time.perf_counter() - t0
k = dr.r.light_keep()
print(json.dumps({"size": [W, H], "lights": args.lights, "radius": args.radius, "no_rest_settle": "ZR_NO_REST_SETTLE" in os.environ, "parts": parts, "settled_after_frame": share,
                  "settled_at_end": dr.r.rest_settled()[1], "us_per_frame": round(el / args.steps * 1e6, 2),
                  "mpixels_s": round(cfg["width"] * cfg["height"] * args.steps / el / 1e6, 1), "read_by_arg": k["read_by_arg"]}))
dr.r.close()
