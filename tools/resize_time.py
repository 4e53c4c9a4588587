"""What a resize costs: on the benchmark scene (config 3, 10 000 instances) a live context goes 1920x1080 <-> 1280x720,
  resize    zr_resize, then the first frame at the new extent (zr_render + zr_finish), each timed on the host
  rebuild   the only thing a host could do before: zr_destroy + zr_create + load_scene of the same scene, then its first frame
Every case alternates the two extents; each figure is the median of five with its spread (max - min).  Before each timed call two frames
are rendered and finished at the old extent, so that both ways start from a context at rest with its pools, map and plans made.
`bytes` is what each way allocates on the device for the step, read off hipMemGetInfo around it (the scene's own buffers are part of the
rebuild's, and of nothing the resize does).  Run it under a time limit:
    timeout -k 10 600 python tools/resize_time.py [--out FILE.json]
One JSON line per case; --out collects them in one file."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import engine as gpu_engine, scenes

EXTENTS = ((1920, 1080), (1280, 720))
RUNS = 5


def med(v):
    return round(float(np.median(v)), 3), round(max(v) - min(v), 3)


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def scene(extent):
    cfg = scenes.config3(10000, extent[0], extent[1])
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    g.set_timing_interval(0)
    return cfg, g


def settle(g):
    for _ in range(2):
        g.render()
    g.finish()


def first_frame(g):
    t = time.perf_counter()
    g.render(); g.finish()
    return (time.perf_counter() - t) * 1e3


def resize_case():
    rows = {e: {"call_ms": [], "first_frame_ms": [], "bytes": []} for e in EXTENTS}
    cfg, g = scene(EXTENTS[0])
    at = 0
    for _ in range(2 * RUNS):
        settle(g)
        to = EXTENTS[at ^ 1]
        before = free_bytes()
        t = time.perf_counter()
        g.resize(*to)
        rows[to]["call_ms"].append((time.perf_counter() - t) * 1e3)
        # (the old set is released inside the call: the difference is new minus old; the peak inside the call is old plus new)
        rows[to]["bytes"].append(before - free_bytes())
        rows[to]["first_frame_ms"].append(first_frame(g))
        at ^= 1
    g.close()
    return rows


def rebuild_case():
    rows = {e: {"call_ms": [], "first_frame_ms": [], "bytes": []} for e in EXTENTS}
    cfg, g = scene(EXTENTS[0])
    at = 0
    for _ in range(2 * RUNS):
        settle(g)
        to = EXTENTS[at ^ 1]
        t = time.perf_counter()
        g.close()
        mid = free_bytes()
        cfg, g = scene(to)
        rows[to]["call_ms"].append((time.perf_counter() - t) * 1e3)
        rows[to]["first_frame_ms"].append(first_frame(g))
        rows[to]["bytes"].append(mid - free_bytes())          # everything the new context holds after its first frame
        at ^= 1
    g.close()
    return rows


def main():
    out = []
    for name, case in (("resize", resize_case), ("rebuild", rebuild_case)):
        for extent, r in case().items():
            line = {"case": name, "to": "%dx%d" % extent, "runs": RUNS, "call_ms": med(r["call_ms"]), "first_frame_ms": med(r["first_frame_ms"]),
                    "bytes": int(np.median(r["bytes"]))}
            print(json.dumps(line), flush=True)
            out.append(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
