"""What highlighting a selection costs: on the benchmark scene (config 3, 10 000 instances, 1920x1080) with the camera orbiting 2 degrees
per frame, so that every frame is drawn, and 0, 1, 100 and all instance slots selected, at radius 2 and 8,
  host     zr_read_color next to zr_read_color_highlighted(1) on the same frames: per frame update, zr_render, zr_finish (not timed), then
           the two calls into preallocated buffers, each timed on the host, their order swapped every frame
  kernels  (--kernel-loop) the same eight cases, three windows each, per frame zr_read_color_highlighted(1), zr_read_color_scaled(2) and
           zr_copy_frame_async's colour copy, for a rocprofv3 --kernel-trace run of its own; --kernel-summary reads that trace and gives,
           per case, the GPU time of k_highlight_mask and k_highlight_apply beside k_frame_scale<2> and the copy's kernel
A window is WINDOW frames after WARMUP; every figure is the median of three windows with their spread (max - min).  The comparison is
against the existing paths on the same frames, never against the code under test.  Run it under a time limit:
    timeout -k 10 600 python tools/highlight_time.py [--out FILE.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/highlight_time.py --kernel-loop [frames]
    python tools/highlight_time.py --kernel-summary DIR [frames] [--out FILE.json]
One JSON line per case; --out collects them in one file."""
import ctypes as C
import json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import abi, engine as gpu_engine, scenes

WINDOW, WARMUP = 100, 10
SELECTED = (0, 1, 100, None)        # None: every slot
RADII = (2, 8)


def setup(width=1920, height=1080):
    cfg = scenes.config3(10000, width, height)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    g.set_timing_interval(0)
    g.set_id_capture(True)
    return cfg, g


def orbit(cfg, g, i):
    a = math.radians(45.0 + 2.0 * i)
    cam = abi.make_camera((math.sqrt(50.0) * math.cos(a), math.sqrt(50.0) * math.sin(a), 5.0), (0.0, 0.0, 0.0))
    g.update_uniforms(cam, cfg["dir"], cfg["point"], cfg["spot"], 0.0, 0.0, 0.0)


def select(g, n):
    """the first n slots (None: all) into the set, the rest out -> how many are in"""
    base, slots = g.instance_slots()
    n = slots if n is None else min(n, slots)
    flags = np.zeros(slots, dtype=np.uint8)
    flags[:n] = 1
    for o, b in enumerate(base):
        e = base[o + 1] if o + 1 < len(base) else slots
        g.highlight_set(o, flags[b:e])
    return n


def med(v):
    return round(float(np.median(v)), 2), round(max(v) - min(v), 2)


def host_case(cfg, g, frame0, n_sel, radius):
    L, h = g.L, g.h
    plain, marked = np.zeros((g.H, g.W, 4), dtype=np.uint8), np.zeros((g.H, g.W, 4), dtype=np.uint8)
    p_plain, p_marked = plain.ctypes.data_as(C.c_void_p), marked.ctypes.data_as(C.c_void_p)
    n = select(g, n_sel)
    g.set_highlight_style(radius=radius)
    calls = (("read_color", lambda: L.zr_read_color(h, p_plain, plain.nbytes)),
             ("read_color_highlighted", lambda: L.zr_read_color_highlighted(h, 1, p_marked, marked.nbytes)))
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
    row = {"part": "host", "selected_slots": n, "radius": radius, "frames_per_window": WINDOW, "windows": 3,
           "pixels_marked_last_frame": int((plain != marked).any(axis=2).sum())}
    for name, _ in calls:
        row[name + "_us"], row[name + "_spread_us"] = med(runs[name])
    return row, frame0


def measure(out_path):
    import gc
    cfg, g = setup()
    gc.disable()
    rows, frame0 = [], 0
    for radius in RADII:
        for n_sel in SELECTED:
            row, frame0 = host_case(cfg, g, frame0, n_sel, radius)
            rows.append(row)
            print(json.dumps(row), flush=True)
    g.close()
    if out_path:
        json.dump({"tool": "tools/highlight_time.py", "scene": "config3(10000) 1920x1080, shadow map 1024, camera orbiting 2 degrees per frame", "rows": rows},
                  open(out_path, "w"), indent=1)


def kernel_loop(frames):
    """every case in the order of measure(), three windows of `frames` frames each: per frame one dispatch of each kernel"""
    import torch
    cfg, g = setup()
    full = torch.zeros(g.W * g.H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    i = 0
    for radius in RADII:
        for n_sel in SELECTED:
            n = select(g, n_sel)
            g.set_highlight_style(radius=radius)
            for _ in range(3 * frames):
                orbit(cfg, g, i)
                g.render()
                out = g.color_highlighted(1)
                g.color_scaled(2)
                g.copy_frame_async(full.data_ptr())
                i += 1
            g.finish()
            print(json.dumps({"kernel_loop": "highlighted at scale 1 + scale 2 + colour copy", "size": "%dx%d" % (g.W, g.H), "frames": 3 * frames,
                              "selected_slots": n, "radius": radius, "pixels_marked_last_frame": int((out != g.color()).any(axis=2).sum())}), flush=True)
    g.close()


KERNELS = (("k_highlight_mask", "k_highlight_mask"), ("k_highlight_apply", "k_highlight_apply"), ("k_frame_scale_2", "k_frame_scale<2"),
           ("colour_copy", "copyBuffer"))


def kernel_summary(directory, frames, out_path):
    """the kernel trace of one --kernel-loop run: each kernel's dispatches in start order fall into 8 cases x 3 windows x `frames`"""
    import csv, glob
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    spans = {key: [] for key, _ in KERNELS}
    copies = {}
    for r in csv.DictReader(open(files[0])):
        span = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for key, part in KERNELS:
            if part in r["Kernel_Name"]:
                spans[key].append(span)
        if "copyBuffer" in r["Kernel_Name"]:             # (uniform uploads and the set's words go through copy kernels too)
            copies.setdefault((r["Kernel_Name"], r.get("Grid_Size", r.get("Grid_Size_X", ""))), []).append(span)
    cases = [(n_sel, radius) for radius in RADII for n_sel in SELECTED]
    # the colour copy is the one copy of its size per frame: the group, by kernel and grid size, that holds one dispatch per frame
    exact = [v for v in copies.values() if len(v) == len(cases) * 3 * frames]
    if len(exact) == 1:
        spans["colour_copy"] = exact[0]
    rows = []
    for c, (n_sel, radius) in enumerate(cases):
        row = {"part": "kernels", "selected_slots": "all" if n_sel is None else n_sel, "radius": radius, "frames_per_window": frames, "windows": 3}
        for key, _ in KERNELS:
            want = len(cases) * 3 * frames
            s = sorted(spans[key])
            if want < len(s) <= want + 2 * len(cases):      # (the set's few words travel through the same copy kernel: the shortest ones)
                for x in sorted(s, key=lambda e: e[1])[:len(s) - want]:
                    s.remove(x)
            d = [ns for _, ns in s]
            if len(d) != want:      # (a copy that ran on a DMA engine leaves no kernel)
                row[key + "_us"] = "Measured: NOT YET (%d dispatches in the trace)" % len(d)
                continue
            w = [float(np.mean(d[(3 * c + k) * frames:(3 * c + k + 1) * frames])) / 1e3 for k in range(3)]
            row[key + "_us"], row[key + "_spread_us"] = med(w)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        json.dump({"tool": "tools/highlight_time.py --kernel-summary", "scene": "config3(10000) 1920x1080, shadow map 1024, camera orbiting 2 degrees per frame",
                   "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    out = a[a.index("--out") + 1] if "--out" in a else None
    if a[:1] == ["--kernel-loop"]:
        kernel_loop(int(a[1]) if len(a) > 1 else 50)
    elif a[:1] == ["--kernel-summary"]:
        kernel_summary(a[1], int(a[2]) if len(a) > 2 and a[2].isdigit() else 50, out)
    else:
        measure(out)
