"""What overlaying lines costs: on the benchmark scene (config 3, 10 000 instances, 1920x1080) with the camera orbiting 2 degrees per
frame, so that every frame is drawn, and 0, 12 (a box's edges), 1 000 and 16 384 segments in the list,
  host     zr_read_color_scaled(1) next to zr_read_color_overlaid(1) on the same frames: per frame update, zr_render, zr_finish (not
           timed), then the two calls into preallocated buffers, each timed on the host, their order swapped every frame
  kernels  (--kernel-loop) the same four cases, three windows each, per frame one zr_read_color_overlaid(1), for a
           rocprofv3 --kernel-trace run of its own; --kernel-summary reads that trace and gives, per case, the GPU time of
           k_overlay_setup and k_overlay_apply
A window is WINDOW frames after WARMUP; every figure is the median of three windows with their spread (max - min).  The comparison is
against the existing path on the same frames, never against the code under test.  Run it under a time limit:
    timeout -k 10 600 python tools/overlay_time.py [--out FILE.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/overlay_time.py --kernel-loop [frames]
    python tools/overlay_time.py --kernel-summary DIR [frames] [--out FILE.json]
One JSON line per case; --out collects them in one file."""
import ctypes as C
import json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import abi, engine as gpu_engine, scenes

WINDOW, WARMUP = 200, 10
SEGMENTS = (0, 12, 1000, 16384)
SCENE = "config3(10000) 1920x1080, shadow map 1024, camera orbiting 2 degrees per frame"


def setup(width=1920, height=1080):
    cfg = scenes.config3(10000, width, height)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    g.set_timing_interval(0)
    return cfg, g


def orbit(cfg, g, i):
    a = math.radians(45.0 + 2.0 * i)
    cam = abi.make_camera((math.sqrt(50.0) * math.cos(a), math.sqrt(50.0) * math.sin(a), 5.0), (0.0, 0.0, 0.0))
    g.update_uniforms(cam, cfg["dir"], cfg["point"], cfg["spot"], 0.0, 0.0, 0.0)


def box_edges(lo, hi, rgba=(255, 200, 0, 255)):
    """the twelve edges of an axis-aligned box"""
    c = [[(lo[k], hi[k])[(i >> k) & 1] for k in range(3)] for i in range(8)]
    return [tuple(c[i]) + tuple(c[j]) + rgba + (0,) for i in range(8) for j in range(i + 1, 8) if bin(i ^ j).count("1") == 1]


def segments(n):
    """0: none; 12: a box round the scene's middle; more: the box and random segments up to 2 units long among the instances, a third XRAY"""
    if n == 0:
        return []
    rows = box_edges((-1.0, -1.0, 0.0), (1.0, 1.0, 1.5))
    rng = np.random.default_rng(n)
    while len(rows) < n:
        a = rng.uniform((-7.0, -7.0, 0.0), (7.0, 7.0, 2.0))
        b = a + rng.uniform(-1.0, 1.0, 3)
        rows.append(tuple(a) + tuple(b) + tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(64, 256)), int(len(rows) % 3 == 0)))
    return rows[:n]


def med(v):
    return round(float(np.median(v)), 2), round(max(v) - min(v), 2)


def host_case(cfg, g, frame0, n_seg):
    L, h = g.L, g.h
    plain, lined = np.zeros((g.H, g.W, 4), dtype=np.uint8), np.zeros((g.H, g.W, 4), dtype=np.uint8)
    p_plain, p_lined = plain.ctypes.data_as(C.c_void_p), lined.ctypes.data_as(C.c_void_p)
    g.overlay_set(segments(n_seg))
    calls = (("read_color_scaled_1", lambda: L.zr_read_color_scaled(h, 1, p_plain, plain.nbytes)),
             ("read_color_overlaid_1", lambda: L.zr_read_color_overlaid(h, 1, 0, p_lined, lined.nbytes)))
    runs = {name: [] for name, _ in calls}
    for _ in range(3):
        acc = {name: 0.0 for name, _ in calls}
        for i in range(frame0, frame0 + WARMUP + WINDOW):
            orbit(cfg, g, i)
            g.render()
            g.finish()
            for k in range(2):
                name, call = calls[(i + k) % 2]
                t = time.perf_counter()
                rc = call()
                dt = time.perf_counter() - t
                assert rc == 0, rc
                if i >= frame0 + WARMUP:
                    acc[name] += dt
        frame0 += WARMUP + WINDOW
        for name, _ in calls:
            runs[name].append(1e6 * acc[name] / WINDOW)
    row = {"part": "host", "segments": n_seg, "frames_per_window": WINDOW, "windows": 3, "pixels_drawn_last_frame": int((plain != lined).any(axis=2).sum())}
    for name, _ in calls:
        row[name + "_us"], row[name + "_spread_us"] = med(runs[name])
    return row, frame0


def measure(out_path):
    import gc
    cfg, g = setup()
    gc.disable()
    rows, frame0 = [], 0
    for n_seg in SEGMENTS:
        row, frame0 = host_case(cfg, g, frame0, n_seg)
        rows.append(row)
        print(json.dumps(row), flush=True)
    g.close()
    if out_path:
        json.dump({"tool": "tools/overlay_time.py", "scene": SCENE, "rows": rows}, open(out_path, "w"), indent=1)


def kernel_loop(frames):
    """every case with segments, in the order of measure(), three windows of `frames` frames each: per frame one dispatch of each kernel"""
    cfg, g = setup()
    i = 0
    for n_seg in SEGMENTS[1:]:
        g.overlay_set(segments(n_seg))
        for _ in range(3 * frames):
            orbit(cfg, g, i)
            g.render()
            out = g.read_color_overlaid(1)
            i += 1
        g.finish()
        print(json.dumps({"kernel_loop": "overlaid at scale 1", "size": "%dx%d" % (g.W, g.H), "frames": 3 * frames, "segments": n_seg,
                          "pixels_drawn_last_frame": int((out != g.color()).any(axis=2).sum())}), flush=True)
    g.close()


KERNELS = ("k_overlay_setup", "k_overlay_apply")


def kernel_summary(directory, frames, out_path):
    """the kernel trace of one --kernel-loop run: each kernel's dispatches in start order fall into 3 cases x 3 windows x `frames`"""
    import csv, glob
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    spans = {key: [] for key in KERNELS}
    for r in csv.DictReader(open(files[0])):
        for key in KERNELS:
            if key in r["Kernel_Name"]:
                spans[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows = []
    for c, n_seg in enumerate(SEGMENTS[1:]):
        row = {"part": "kernels", "segments": n_seg, "frames_per_window": frames, "windows": 3}
        for key in KERNELS:
            d = [ns for _, ns in sorted(spans[key])]
            if len(d) != len(SEGMENTS[1:]) * 3 * frames:
                row[key + "_us"] = "Measured: NOT YET (%d dispatches in the trace)" % len(d)
                continue
            w = [float(np.mean(d[(3 * c + k) * frames:(3 * c + k + 1) * frames])) / 1e3 for k in range(3)]
            row[key + "_us"], row[key + "_spread_us"] = med(w)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        json.dump({"tool": "tools/overlay_time.py --kernel-summary", "scene": SCENE, "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    out = a[a.index("--out") + 1] if "--out" in a else None
    if a[:1] == ["--kernel-loop"]:
        kernel_loop(int(a[1]) if len(a) > 1 else 50)
    elif a[:1] == ["--kernel-summary"]:
        kernel_summary(a[1], int(a[2]) if len(a) > 2 and a[2].isdigit() else 50, out)
    else:
        measure(out)
