"""What the wireframe costs: on the benchmark scene (config 3, 10 000 instances, 1920x1080), id capture on, at rest (the camera stands)
and with the camera orbiting 2 degrees per frame (every frame is drawn),
  host     zr_read_color next to zr_read_color_staged(ZR_STAGE_WIRE, 1) on the same frames: per frame update, zr_render, zr_finish (not
           timed), then the two calls into preallocated buffers, each timed on the host, their order swapped every frame
  kernels  (--kernel-loop) the same two cases, three windows each, per frame one zr_copy_frame_staged_async(ZR_STAGE_WIRE, 1) into a
           device buffer, for a rocprofv3 --kernel-trace run of its own; --kernel-summary reads that trace and gives, per case, the
           GPU time of k_wire_apply and, for comparison, of k_resolve_gbuffer on the same frames
A window is WINDOW frames after WARMUP; every figure is the median of three windows with their spread (max - min).  The comparison is
against the existing path on the same frames, never against the code under test.  Run it under a time limit:
    timeout -k 10 600 python tools/wire_time.py [--out FILE.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/wire_time.py --kernel-loop [frames]
    python tools/wire_time.py --kernel-summary DIR [frames] [--out FILE.json]
One JSON line per case; --out collects them in one file."""
import ctypes as C
import json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import abi, engine as gpu_engine, scenes

WINDOW, WARMUP = 200, 10
CASES = ("rest", "orbit")
SCENE = "config3(10000) 1920x1080, shadow map 1024, id capture on; rest: the camera stands, orbit: 2 degrees per frame"


def setup(width=1920, height=1080):
    cfg = scenes.config3(10000, width, height)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    g.set_timing_interval(0)
    g.set_id_capture(True)
    g.set_wire_style()
    return cfg, g


def camera(cfg, g, case, i):
    a = math.radians(45.0 + (2.0 * i if case == "orbit" else 0.0))
    cam = abi.make_camera((math.sqrt(50.0) * math.cos(a), math.sqrt(50.0) * math.sin(a), 5.0), (0.0, 0.0, 0.0))
    g.update_uniforms(cam, cfg["dir"], cfg["point"], cfg["spot"], 0.0, 0.0, 0.0)


def med(v):
    return round(float(np.median(v)), 2), round(max(v) - min(v), 2)


def host_case(cfg, g, frame0, case):
    L, h = g.L, g.h
    plain, wired = np.zeros((g.H, g.W, 4), dtype=np.uint8), np.zeros((g.H, g.W, 4), dtype=np.uint8)
    p_plain, p_wired = plain.ctypes.data_as(C.c_void_p), wired.ctypes.data_as(C.c_void_p)
    calls = (("read_color", lambda: L.zr_read_color(h, p_plain, plain.nbytes)),
             ("read_color_staged_wire_1", lambda: L.zr_read_color_staged(h, abi.STAGE_WIRE, 1, p_wired, wired.nbytes)))
    runs = {name: [] for name, _ in calls}
    for _ in range(3):
        acc = {name: 0.0 for name, _ in calls}
        for i in range(frame0, frame0 + WARMUP + WINDOW):
            camera(cfg, g, case, i)
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
    row = {"part": "host", "case": case, "frames_per_window": WINDOW, "windows": 3, "pixels_on_the_wire_last_frame": int((plain != wired).any(axis=2).sum())}
    for name, _ in calls:
        row[name + "_us"], row[name + "_spread_us"] = med(runs[name])
    return row, frame0


def measure(out_path):
    import gc
    cfg, g = setup()
    gc.disable()
    rows, frame0 = [], 0
    for case in CASES:
        row, frame0 = host_case(cfg, g, frame0, case)
        rows.append(row)
        print(json.dumps(row), flush=True)
    g.close()
    if out_path:
        json.dump({"tool": "tools/wire_time.py", "scene": SCENE, "rows": rows}, open(out_path, "w"), indent=1)


def kernel_loop(frames):
    """both cases, in the order of measure(), three windows of `frames` frames each: per frame one dispatch of k_wire_apply"""
    import torch
    cfg, g = setup()
    dest = torch.zeros((g.H, g.W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    i = 0
    for case in CASES:
        for _ in range(3 * frames):
            camera(cfg, g, case, i)
            g.render()
            g.copy_frame_staged_async(abi.STAGE_WIRE, 1, dest.data_ptr())
            i += 1
        g.finish()
        print(json.dumps({"kernel_loop": "wire at scale 1, device form", "size": "%dx%d" % (g.W, g.H), "frames": 3 * frames, "case": case,
                          "pixels_on_the_wire_last_frame": int((dest.cpu().numpy() != g.color()).any(axis=2).sum())}), flush=True)
    g.close()


KERNELS = ("k_wire_apply", "k_resolve_gbuffer")


def kernel_summary(directory, frames, out_path):
    """the kernel trace of one --kernel-loop run: k_wire_apply's dispatches in start order fall into 2 cases x 3 windows x `frames`;
    k_resolve_gbuffer's are reported per case as the mean of however many the case's frames ran (a resting frame keeps its GBuffer)"""
    import csv, glob
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    spans = {key: [] for key in KERNELS}
    for r in csv.DictReader(open(files[0])):
        for key in KERNELS:
            if key in r["Kernel_Name"]:
                spans[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    wire = sorted(spans["k_wire_apply"])
    rows = []
    for c, case in enumerate(CASES):
        row = {"part": "kernels", "case": case, "frames_per_window": frames, "windows": 3}
        if len(wire) != len(CASES) * 3 * frames:
            row["k_wire_apply_us"] = "Measured: NOT YET (%d dispatches in the trace)" % len(wire)
        else:
            mine = wire[3 * c * frames:3 * (c + 1) * frames]
            w = [float(np.mean([ns for _, ns in mine[k * frames:(k + 1) * frames]])) / 1e3 for k in range(3)]
            row["k_wire_apply_us"], row["k_wire_apply_spread_us"] = med(w)
            res = [ns for t, ns in spans["k_resolve_gbuffer"] if mine[0][0] <= t <= mine[-1][0]]
            row["k_resolve_gbuffer_dispatches"] = len(res)
            if res:
                row["k_resolve_gbuffer_mean_us"] = round(float(np.mean(res)) / 1e3, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        json.dump({"tool": "tools/wire_time.py --kernel-summary", "scene": SCENE, "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    out = a[a.index("--out") + 1] if "--out" in a else None
    if a[:1] == ["--kernel-loop"]:
        kernel_loop(int(a[1]) if len(a) > 1 else 50)
    elif a[:1] == ["--kernel-summary"]:
        kernel_summary(a[1], int(a[2]) if len(a) > 2 and a[2].isdigit() else 50, out)
    else:
        measure(out)
