"""What a texture update costs, on scenes.config3(textured=True) (10 000 instances, 1920x1080) with its material at 512^2 and at 2048^2:
  host     one slot update (zr_object_set_texture, base colour) plus the next frame
  device   the same through zr_object_update_texture_async, the image already on the GPU
  rebuild  zr_scene_clear + re-add of the whole scene with the new image - the only route before the update calls
each as the median wall time of 15 repetitions (rebuild: 5) with finish() before and after (so "the next frame" is a whole unpipelined frame, and
"none" - the same frame without an update - is the figure to subtract).  Then the frame PERIOD with two frames in flight: the mean of
60 frames with one 512^2 device update before each against none.  The protocol of instance_update_time.py: 5 frames to settle first.
Run it under a time limit:
    timeout -k 10 600 python tools/texture_update_time.py [512 2048]
One JSON line per case."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from zeldaengine_amd import abi, engine as gpu_engine, scenes

REPS = 15


def timed(fn, reps=REPS):
    out = []
    for i in range(reps):
        t = time.perf_counter()
        fn(i)
        out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)


def load(g, cfg, images):
    mat, keep = abi.make_material(images)
    cfg["objects"][0]["material"] = mat
    gpu_engine.load_scene(g, cfg)
    return keep


def run(dim):
    cfg = scenes.config3(10000)
    images = scenes.synthetic_material(dim)
    alt = [np.ascontiguousarray(np.roll(images[0], 7 * (k + 1), axis=1)) for k in range(2)]      # two other base-colour images, used in turn
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    keep = load(g, cfg, images)
    dev = torch.device("cuda", 0)
    d_alt = [torch.from_numpy(a).to(dev) for a in alt]
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for _ in range(5):
        g.render()
    g.finish()

    def none(i):
        g.render(); g.finish()

    def host(i):
        g.object_set_texture(0, 0, alt[i & 1]); g.render(); g.finish()

    def device(i):
        g.object_update_texture_async(0, 0, d_alt[i & 1], stream=ts); g.render(); g.finish()

    def rebuild(i):
        nonlocal keep
        g.scene_clear()
        keep = load(g, cfg, [alt[i & 1]] + images[1:])
        g.render(); g.finish()

    for name, fn in (("none", none), ("host", host), ("device", device), ("rebuild", rebuild)):
        fn(0)                                                # (first use: staging slots, events, the threshold table)
        reps = 5 if name == "rebuild" else REPS              # (a rebuild builds seven chains on the CPU: seconds at 2048^2)
        med, lo, hi = timed(fn, reps)
        print(json.dumps({"texture": dim, "case": name, "ms_median": med, "ms_min": lo, "ms_max": hi, "reps": reps}), flush=True)
    ts.synchronize()
    if dim == 512:
        for per_frame in (False, True):
            for i in range(5):
                if per_frame:
                    g.object_update_texture_async(0, 0, d_alt[i & 1], stream=ts)
                g.render()
            g.finish(); ts.synchronize()
            t = time.perf_counter()
            for i in range(60):
                if per_frame:
                    g.object_update_texture_async(0, 0, d_alt[i & 1], stream=ts)
                g.render()
            g.finish(); ts.synchronize()
            print(json.dumps({"texture": dim, "case": "period, one device update per frame" if per_frame else "period, no update",
                              "ms_per_frame": round((time.perf_counter() - t) / 60 * 1e3, 4), "frames": 60, "overflow": g.stats()["overflow"]}), flush=True)
    g.close()
    del keep


if __name__ == "__main__":
    for d in (sys.argv[1:] or ["512", "2048"]):
        run(int(d))
