"""What delivering a frame costs the host: zr_read_frame_delta and zr_read_frame_delta_packed next to zr_read_color on the same frames of
the benchmark scene (config 3, 10 000 instances, 1920x1080, 2 040 tiles), in four regimes: rest; one instance moved per frame; 100
instances moved per frame; the camera orbiting 2 degrees per frame.  Per frame: update, zr_render, zr_finish (not timed), then a
delivery and zr_read_color one after the other into preallocated buffers, each call timed on the host, the order swapped every frame.
The raw and the packed form share one delivered copy, so a frame can be delivered through one of them only: every regime runs twice over
the same frames, once per form.  A window is WINDOW frames after WARMUP; a regime is three windows per form, reported as their medians
with the spread (max - min) of the three.  Run it under a time limit:
    timeout -k 10 900 python tools/frame_delta_time.py [--out FILE.json]
    ... --kernel-loop rest|full [frames] [raw|packed] [WxH]
                           the deliveries alone for a rocprofv3 --kernel-trace --stats run of its own (full: a zr_frame_delta_reset
                           before every delivery, so every tile is listed and packed or encoded), of the raw or the packed form, at
                           1920x1080 or another size (3840x2160: 8 160 tiles, what the packed form's placing was chosen at)
One JSON line per regime; --out collects them in one file."""
import ctypes as C
import json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zeldaengine_amd import abi, engine as gpu_engine, scenes

WINDOW, WARMUP, VARIANTS = 200, 20, 4


def setup(mode=1, width=1920, height=1080):
    cfg = scenes.config3(10000, width, height)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    g.set_timing_interval(0)
    g.set_frame_delta(mode)
    return cfg, g


def regimes(cfg, g):
    inst = cfg["objects"][0]["instances"]
    rng = np.random.default_rng(7)

    def still():
        g.update_uniforms(cfg["camera"], cfg["dir"], cfg["point"], cfg["spot"], 0.0, 0.0, 0.0)

    def moved(m):
        sets = []
        for _ in range(VARIANTS):
            first = int(rng.integers(0, len(inst) - m + 1))
            there = inst[first:first + m].copy()
            there["InstancePosition"][:, :2] += rng.uniform(-0.05, 0.05, (m, 2)).astype(np.float32)
            sets.append((first, there, inst[first:first + m].copy()))

        def step(i):                      # every frame one of the ranges goes there or back: each call changes the values
            still()
            first, there, back = sets[i % VARIANTS]
            g.object_set_instances(0, back if (i // VARIANTS) & 1 else there, first)
        return step

    def orbit(i):
        a = math.radians(45.0 + 2.0 * i)
        cam = abi.make_camera((math.sqrt(50.0) * math.cos(a), math.sqrt(50.0) * math.sin(a), 5.0), (0.0, 0.0, 0.0))
        g.update_uniforms(cam, cfg["dir"], cfg["point"], cfg["spot"], 0.0, 0.0, 0.0)

    return [("rest", lambda i: still()), ("one_instance_of_10000", moved(1)), ("100_instances_of_10000", moved(100)), ("camera_orbit", orbit)]


def window(g, step, bufs, frame0, packed):
    """-> (mean tiles per delivery, mean us per delivery, mean us per zr_read_color, mean payload bytes per delivery) over WINDOW frames;
    the delivery is zr_read_frame_delta, or zr_read_frame_delta_packed where `packed`"""
    tiles, pixels, color, hdr, offsets, stream, phdr = bufs
    L, h = g.L, g.h
    p_t, p_p, p_c = tiles.ctypes.data_as(C.c_void_p), pixels.ctypes.data_as(C.c_void_p), color.ctypes.data_as(C.c_void_p)
    p_o, p_s = offsets.ctypes.data_as(C.c_void_p), stream.ctypes.data_as(C.c_void_p)
    t_delta = t_color = 0.0
    n_tiles = n_bytes = 0

    def read_delta():
        t = time.perf_counter()
        if packed:
            rc = L.zr_read_frame_delta_packed(h, p_t, tiles.size, p_o, offsets.size, p_s, stream.nbytes, C.byref(phdr), C.sizeof(phdr))
        else:
            rc = L.zr_read_frame_delta(h, p_t, tiles.size, p_p, pixels.nbytes, C.byref(hdr), C.sizeof(hdr))
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt

    def read_color():
        t = time.perf_counter()
        rc = L.zr_read_color(h, p_c, color.nbytes)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt

    for i in range(frame0, frame0 + WARMUP + WINDOW):
        step(i)
        g.render()
        g.finish()
        if i & 1:
            c = read_color(); d = read_delta()
        else:
            d = read_delta(); c = read_color()
        if i >= frame0 + WARMUP:
            t_delta += d; t_color += c
            n_tiles += phdr.n_tiles if packed else hdr.n_tiles
            n_bytes += phdr.bytes if packed else hdr.n_tiles * abi.TILE_BYTES
    return n_tiles / WINDOW, 1e6 * t_delta / WINDOW, 1e6 * t_color / WINDOW, n_bytes / WINDOW


def measure(out_path):
    import gc
    cfg, g = setup(abi.FRAME_DELTA_PACKED)
    total = g.frame_delta_tiles()
    bufs = (np.zeros(total, dtype=np.uint32), np.zeros((total, 32, 32, 4), dtype=np.uint8), np.zeros((g.H, g.W, 4), dtype=np.uint8), abi.FrameDelta(),
            np.zeros(total + 1, dtype=np.uint32), np.zeros(total * abi.RECORD_MAX_BYTES, dtype=np.uint8), abi.FrameDeltaPacked())
    rows = []
    gc.disable()
    frame0 = 0
    for name, step in regimes(cfg, g):
        row = {"regime": name, "frames_per_window": WINDOW, "windows": 3, "total_tiles": total, "bytes_per_read_color": g.W * g.H * 4}
        for form, packed in (("read_frame_delta", False), ("read_frame_delta_packed", True)):
            g.set_frame_delta(abi.FRAME_DELTA_PACKED if packed else 1)      # (the form under test alone has its buffers)
            runs = []
            for k in range(3):
                runs.append(window(g, step, bufs, frame0, packed))
                frame0 += WARMUP + WINDOW
            tiles = float(np.median([r[0] for r in runs]))
            d, c = [r[1] for r in runs], [r[2] for r in runs]
            row.update({form + "_tiles": round(tiles, 2), form + "_payload_bytes": int(round(float(np.median([r[3] for r in runs])))),
                        form + "_us": round(float(np.median(d)), 2), form + "_spread_us": round(max(d) - min(d), 2),
                        "read_color_beside_" + form + "_us": round(float(np.median(c)), 2),
                        "read_color_beside_" + form + "_spread_us": round(max(c) - min(c), 2)})
        # the raw form's pass under the names profiles/r10_a_frame_delta.json was recorded with
        tiles = row["read_frame_delta_tiles"]
        row.update({"tiles_per_delivery": tiles, "bytes_per_delivery": int(round(16 + tiles * (4 + abi.TILE_BYTES))),
                    "read_color_us": row["read_color_beside_read_frame_delta_us"], "read_color_spread_us": row["read_color_beside_read_frame_delta_spread_us"]})
        row["color_over_delta"] = round(row["read_color_us"] / row["read_frame_delta_us"], 3)
        if name in ("rest", "one_instance_of_10000"):      # the raw form's bar: faster by more than the spread of the three windows
            row["faster_by_more_than_the_spread"] = bool(row["read_color_us"] - row["read_frame_delta_us"] > max(row["read_frame_delta_spread_us"], row["read_color_spread_us"]))
        row["raw_bytes_of_the_packed_tiles"] = int(round(row["read_frame_delta_packed_tiles"] * abi.TILE_BYTES))
        if row["read_frame_delta_packed_payload_bytes"]:
            row["raw_over_packed_bytes"] = round(row["raw_bytes_of_the_packed_tiles"] / row["read_frame_delta_packed_payload_bytes"], 3)
        row["packed_minus_raw_us"] = round(row["read_frame_delta_packed_us"] - row["read_frame_delta_us"], 2)
        if name == "rest":                                 # what was expected of the packed form: no more than the raw one, within the spread
            row["packed_within_the_spread_of_raw"] = bool(row["packed_minus_raw_us"] <= max(row["read_frame_delta_spread_us"], row["read_frame_delta_packed_spread_us"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    g.close()
    if out_path:
        json.dump({"tool": "tools/frame_delta_time.py", "scene": "config3(10000) 1920x1080, shadow map 1024", "rows": rows}, open(out_path, "w"), indent=1)


def kernel_loop(mode, frames, form, size):
    packed = form == "packed"
    cfg, g = setup(abi.FRAME_DELTA_PACKED if packed else 1, *size)
    step = regimes(cfg, g)[0][1]
    total = g.frame_delta_tiles()
    tiles, pixels = np.zeros(total, dtype=np.uint32), np.zeros((total, 32, 32, 4), dtype=np.uint8)
    offsets, stream = np.zeros(total + 1, dtype=np.uint32), np.zeros(total * abi.RECORD_MAX_BYTES, dtype=np.uint8)
    for i in range(frames):
        step(i)
        g.render()
        if mode == "full":
            g.frame_delta_reset()
        if packed:
            _, _, _, hd = g.read_frame_delta_packed(tiles, offsets, stream)
        else:
            _, _, hd = g.read_frame_delta(tiles, pixels)
    print(json.dumps({"kernel_loop": mode, "form": form, "size": "%dx%d" % (g.W, g.H), "frames": frames, "last_delivery": hd}), flush=True)
    g.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["--kernel-loop"]:
        kernel_loop(a[1], int(a[2]) if len(a) > 2 else 100, a[3] if len(a) > 3 else "raw",
                    tuple(int(v) for v in a[4].split("x")) if len(a) > 4 else (1920, 1080))
    else:
        measure(a[1] if a[:1] == ["--out"] else None)
