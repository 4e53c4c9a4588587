"""What casting rays costs: on the benchmark scene (config 3, 10 000 instances, 1920x1080, one frame rendered and finished),
  one      one ray from the camera's position at an instance's centre, which hits, through zr_raycast: the call's latency on the host
           (the copy in, one launch that goes through all three levels and the winner's record, the copy back, one wait)
  aimed    4 096 rays from the camera's position aimed at random instances' centres
  grid     one camera ray per pixel of a 480 x 270 grid over the frame (129 600 rays)
each with the bounds on and with ZR_RAY_NO_BOUNDS (every triangle of every shown instance).  A case is timed on the host round the
call, after a warm-up call of the same shape; every figure is the median of three windows of REPEAT calls with their spread (max - min),
in microseconds per call and Mrays/s.  Nothing is compared against another build: a record, not a bar.  Run it under a time limit:
    timeout -k 10 600 python tools/raycast_time.py [--out FILE.json]
One JSON line per case; --out collects them in one file."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import abi, engine as gpu_engine, scenes

SCENE = "config3(10000) 1920x1080, shadow map 1024, one frame"
REPEAT = {"one": 200, "aimed": 20, "grid": 3}
REPEAT_NO_BOUNDS = {"one": 20, "aimed": 2, "grid": 1}


def setup(width=1920, height=1080):
    cfg = scenes.config3(10000, width, height)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    g.set_timing_interval(0)
    g.render()
    g.finish()
    return cfg, g


def rays_of(cfg, g, case):
    if case in ("one", "aimed"):
        n = 1 if case == "one" else 4096
        rng = np.random.default_rng(7)
        inst = [o["instances"] for o in cfg["objects"] if o.get("instances") is not None]
        pos = np.concatenate([np.asarray(i["InstancePosition"], dtype=np.float64) for i in inst])
        eye = g.camera_ray(g.W / 2 + 0.5, g.H / 2 + 0.5)[0]["origin"].astype(np.float64)
        tgt = pos[rng.integers(0, len(pos), n)]
        return abi.make_rays(np.tile(eye, (n, 1)), tgt - eye, 0.0, 2.0)
    xs, ys = np.meshgrid(np.arange(480), np.arange(270))
    return np.concatenate([g.camera_ray((x + 0.5) * g.W / 480.0, (y + 0.5) * g.H / 270.0) for x, y in zip(xs.ravel(), ys.ravel())])


def med(v):
    return round(float(np.median(v)), 2), round(max(v) - min(v), 2)


def time_case(g, rays, flags, repeat):
    hits = g.raycast(rays, flags)                                        # warm-up: the shape's staging, the code object
    windows = []
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(repeat):
            hits = g.raycast(rays, flags)
        windows.append((time.perf_counter() - t) / repeat * 1e6)
    us, spread = med(windows)
    return {"rays": len(rays), "no_bounds": bool(flags & abi.RAY_NO_BOUNDS), "hits": int((hits["flags"] & 1).sum()), "us_per_call": us, "us_spread": spread,
            "mrays_per_s": round(len(rays) / us, 3), "calls_per_window": repeat}


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cfg, g = setup()
    rows = []
    try:
        for case in ("one", "aimed", "grid"):
            rays = rays_of(cfg, g, case)
            for flags, repeat in ((0, REPEAT[case]), (abi.RAY_NO_BOUNDS, REPEAT_NO_BOUNDS[case])):
                row = {"case": case, "scene": SCENE}
                row.update(time_case(g, rays, flags, repeat))
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        g.close()
    if out:
        json.dump(rows, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
