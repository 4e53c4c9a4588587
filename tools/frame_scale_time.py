"""What delivering a scaled frame costs the host: on the benchmark scene (config 3, 10 000 instances, 1920x1080) with the camera orbiting 2
degrees per frame, so that every frame is drawn,
  host     zr_read_color next to zr_read_color_scaled at scales 2, 4 and 8 on the same frames: per frame update, zr_render, zr_finish (not
           timed), then the four calls one after the other into preallocated buffers, each timed on the host, their order rotated every frame
  device   the frame period with nothing copied, with zr_copy_frame_async's colour copy and with zr_copy_frame_scaled_async at scale 2
           behind every frame: a window is enqueued without a host synchronisation and finished once; the forms take turns window by window
  delta    zr_read_frame_delta_packed at delta scale 1 and at delta scale 2 on the same camera path: time and payload bytes per frame
A window is WINDOW frames after WARMUP; every figure is the median of three windows with their spread (max - min).  Run it under a time limit:
    timeout -k 10 600 python tools/frame_scale_time.py [--out FILE.json]
    ... --kernel-loop [frames]      zr_read_color_scaled at scale 2 and a full raw delivery at scale 1 per frame, for a rocprofv3
                                    --kernel-trace --stats run of its own: k_frame_scale beside k_delta_mark in one trace
One JSON line per part; --out collects them in one file."""
import ctypes as C
import json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import abi, engine as gpu_engine, scenes

WINDOW, WARMUP, SCALES = 200, 20, (2, 4, 8)


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


def med(v):
    return round(float(np.median(v)), 2), round(max(v) - min(v), 2)


def host_forms(cfg, g, frame0):
    """-> the row of the host forms, and the next frame number"""
    L, h = g.L, g.h
    bufs = {1: np.zeros((g.H, g.W, 4), dtype=np.uint8)}
    for s in SCALES:
        bufs[s] = np.zeros(gpu_engine.frame_scaled_extent(g.W, g.H, s)[::-1] + (4,), dtype=np.uint8)
    ptr = {s: b.ctypes.data_as(C.c_void_p) for s, b in bufs.items()}

    def read(s):
        t = time.perf_counter()
        rc = L.zr_read_color(h, ptr[1], bufs[1].nbytes) if s == 1 else L.zr_read_color_scaled(h, s, ptr[s], bufs[s].nbytes)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt

    order = (1,) + SCALES
    runs = {s: [] for s in order}
    for _ in range(3):
        acc = {s: 0.0 for s in order}
        for i in range(frame0, frame0 + WARMUP + WINDOW):
            orbit(cfg, g, i)
            g.render()
            g.finish()
            for k in range(len(order)):
                s = order[(i + k) % len(order)]
                dt = read(s)
                if i >= frame0 + WARMUP:
                    acc[s] += dt
        frame0 += WARMUP + WINDOW
        for s in order:
            runs[s].append(1e6 * acc[s] / WINDOW)
    row = {"part": "host", "frames_per_window": WINDOW, "windows": 3, "bytes_per_read_color": bufs[1].nbytes}
    row["read_color_us"], row["read_color_spread_us"] = med(runs[1])
    for s in SCALES:
        row["read_color_scaled_%d_us" % s], row["read_color_scaled_%d_spread_us" % s] = med(runs[s])
        row["read_color_scaled_%d_bytes" % s] = bufs[s].nbytes
    row["scale_2_below_read_color"] = bool(row["read_color_scaled_2_us"] < row["read_color_us"])
    return row, frame0


def device_forms(cfg, g, frame0):
    import torch
    full = torch.zeros(g.W * g.H * 4, dtype=torch.uint8, device="cuda")
    wd, hd = gpu_engine.frame_scaled_extent(g.W, g.H, 2)
    half = torch.zeros(wd * hd * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    forms = (("no_copy", lambda: None), ("copy_frame_async", lambda: g.copy_frame_async(full.data_ptr())),
             ("copy_frame_scaled_async_2", lambda: g.copy_frame_scaled_async(2, half.data_ptr())))
    runs = {name: [] for name, _ in forms}
    for _ in range(3):
        for name, enqueue in forms:
            for i in range(frame0, frame0 + WARMUP):
                orbit(cfg, g, i); g.render(); enqueue()
            g.finish()
            t = time.perf_counter()
            for i in range(frame0 + WARMUP, frame0 + WARMUP + WINDOW):
                orbit(cfg, g, i); g.render(); enqueue()
            g.finish()
            runs[name].append(1e6 * (time.perf_counter() - t) / WINDOW)
            frame0 += WARMUP + WINDOW
    row = {"part": "device", "frames_per_window": WINDOW, "windows": 3}
    for name, _ in forms:
        row[name + "_frame_us"], row[name + "_frame_spread_us"] = med(runs[name])
    return row, frame0


def delta_forms(cfg, g, frame0):
    L, h = g.L, g.h
    runs = {1: [], 2: []}
    for _ in range(3):
        for s in (1, 2):
            g.set_frame_delta(False)
            g.set_frame_delta_scale(s)
            g.set_frame_delta(abi.FRAME_DELTA_PACKED)
            total = g.frame_delta_tiles()
            tiles, offsets = np.zeros(total, dtype=np.uint32), np.zeros(total + 1, dtype=np.uint32)
            stream, hd = np.zeros(total * abi.RECORD_MAX_BYTES, dtype=np.uint8), abi.FrameDeltaPacked()
            p_t, p_o, p_s = (a.ctypes.data_as(C.c_void_p) for a in (tiles, offsets, stream))
            t_acc, n_bytes, n_tiles = 0.0, 0, 0
            for i in range(frame0, frame0 + WARMUP + WINDOW):
                orbit(cfg, g, i)
                g.render()
                g.finish()
                t = time.perf_counter()
                rc = L.zr_read_frame_delta_packed(h, p_t, tiles.size, p_o, offsets.size, p_s, stream.nbytes, C.byref(hd), C.sizeof(hd))
                dt = time.perf_counter() - t
                assert rc == 0, rc
                if i >= frame0 + WARMUP:
                    t_acc += dt; n_bytes += hd.bytes; n_tiles += hd.n_tiles
            runs[s].append((1e6 * t_acc / WINDOW, n_bytes / WINDOW, n_tiles / WINDOW, total))
        frame0 += WARMUP + WINDOW            # (both scales on the same frames)
    g.set_frame_delta(False)
    g.set_frame_delta_scale(1)
    row = {"part": "delta", "frames_per_window": WINDOW, "windows": 3}
    for s in (1, 2):
        k = "read_frame_delta_packed_scale_%d" % s
        row[k + "_us"], row[k + "_spread_us"] = med([r[0] for r in runs[s]])
        row[k + "_payload_bytes"] = int(round(float(np.median([r[1] for r in runs[s]]))))
        row[k + "_tiles"] = round(float(np.median([r[2] for r in runs[s]])), 2)
        row[k + "_total_tiles"] = runs[s][0][3]
    return row, frame0


def measure(out_path):
    import gc
    cfg, g = setup()
    gc.disable()
    rows, frame0 = [], 0
    for part in (host_forms, device_forms, delta_forms):
        row, frame0 = part(cfg, g, frame0)
        rows.append(row)
        print(json.dumps(row), flush=True)
    g.close()
    if out_path:
        json.dump({"tool": "tools/frame_scale_time.py", "scene": "config3(10000) 1920x1080, shadow map 1024, camera orbiting 2 degrees per frame", "rows": rows},
                  open(out_path, "w"), indent=1)


def kernel_loop(frames):
    cfg, g = setup()
    g.set_frame_delta(True)
    total = g.frame_delta_tiles()
    tiles, pixels = np.zeros(total, dtype=np.uint32), np.zeros((total, 32, 32, 4), dtype=np.uint8)
    for i in range(frames):
        orbit(cfg, g, i)
        g.render()
        out = g.color_scaled(2)
        g.frame_delta_reset()
        _, _, hd = g.read_frame_delta(tiles, pixels)
    print(json.dumps({"kernel_loop": "scale 2 + full raw delivery", "size": "%dx%d" % (g.W, g.H), "frames": frames, "scaled": list(out.shape), "last_delivery": hd}), flush=True)
    g.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["--kernel-loop"]:
        kernel_loop(int(a[1]) if len(a) > 1 else 100)
    else:
        measure(a[1] if a[:1] == ["--out"] else None)
