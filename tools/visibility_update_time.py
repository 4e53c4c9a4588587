"""Frame time with instances hidden and shown every frame, config 3 (10 000 instances, 1920x1080) and config 4 (1 M instances,
3840x2160), for 0 / 1 / 10 / 100 % of the instances toggled before each frame through the host form (zr_object_set_instance_visibility,
contiguous ranges) and the device form (zr_object_update_instance_visibility_async with an index list, tensors already on the GPU), and
one row per config with half the instances hidden and nothing toggled: what a hidden instance still costs.  The protocol of
instance_update_time.py: 5 frames to settle, then the mean wall time of 30 frames with one call before each, finish() at the end.  Run it
under a time limit:
    timeout -k 10 900 python tools/visibility_update_time.py [3|4 ...]
One JSON line per case."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from zeldaengine_amd import engine as gpu_engine, scenes

FRACTIONS = (0.0, 0.01, 0.1, 1.0)
VARIANTS = 4                        # distinct toggle sets, used in turn


def variants(n, frac, seed):
    """VARIANTS (first, count) ranges and index lists of frac * n instances."""
    m = int(round(frac * n))
    rng = np.random.default_rng(seed)
    out = []
    for v in range(VARIANTS):
        first = int(rng.integers(0, n - m + 1)) if m < n else 0
        idx = np.sort(rng.choice(n, m, replace=False)).astype(np.int32) if m < n else np.arange(n, dtype=np.int32)
        out.append((first, m, idx))
    return out


def timed(g, ts, update):
    for i in range(5):
        update(i); g.render()
    g.finish(); ts.synchronize()
    t = time.perf_counter()
    for i in range(30):
        update(i); g.render()
    g.finish(); ts.synchronize()
    return (time.perf_counter() - t) / 30


def run(config):
    cfg = scenes.config3(10000) if config == 3 else scenes.config4(1000000)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    n = len(cfg["objects"][0]["instances"])
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)

    def row(pct, form, dt, hidden_pct=0.0):
        st = g.stats()
        print(json.dumps({"config": config, "instances": n, "toggled_pct": pct, "hidden_pct": hidden_pct, "form": form,
                          "ms_per_frame": round(dt * 1e3, 4), "overflow": st["overflow"], "covered_pixels": st["covered_pixels"]}), flush=True)

    for frac in FRACTIONS:
        vs = variants(n, frac, 7)
        # every set is hidden on its even turns and shown on its odd ones (turn = i // VARIANTS)
        bytes_h = [np.zeros(m, np.uint8) for _, m, _ in vs], [np.ones(m, np.uint8) for _, m, _ in vs]
        d_idx = [torch.from_numpy(idx).to(dev) for _, _, idx in vs]
        d_val = [torch.zeros(len(idx), dtype=torch.uint8, device=dev) for _, _, idx in vs], [torch.ones(len(idx), dtype=torch.uint8, device=dev) for _, _, idx in vs]
        torch.cuda.synchronize()
        for form in ("host", "device"):
            if frac == 0.0 and form == "device":
                continue                                    # (0 %: no call at all, one row)

            def update(i):
                if frac == 0.0:
                    return
                v, show = i % VARIANTS, (i // VARIANTS) % 2
                if form == "host":
                    g.object_set_instance_visibility(0, bytes_h[show][v], vs[v][0])
                else:
                    g.object_update_instance_visibility_async(0, d_val[show][v], d_idx[v], stream=ts)

            dt = timed(g, ts, update)
            row(100.0 * frac, form if frac else "none", dt)
            g.object_set_instance_visibility(0, np.ones(n, np.uint8))      # the next case starts from everything shown
    half = (np.arange(n) % 2).astype(np.uint8)
    g.object_set_instance_visibility(0, half)
    row(0.0, "none", timed(g, ts, lambda i: None), hidden_pct=50.0)
    g.close()


if __name__ == "__main__":
    for c in (sys.argv[1:] or ["3", "4"]):
        run(int(c))
