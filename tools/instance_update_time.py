"""Frame time with instances moved every frame, config 3 (10 000 instances, 1920x1080) and config 4 (1 M instances, 3840x2160), for
0 / 1 / 10 / 100 % of the instances per frame through the host form (zr_object_set_instances, contiguous ranges) and the device form
(zr_object_update_instances_async with an index list, tensors already on the GPU).  The protocol of config4_time.py: 5 frames to settle,
then the mean wall time of 30 frames with one update before each, finish() at the end.  Run it under a time limit:
    timeout -k 10 900 python tools/instance_update_time.py [3|4 ...]
One JSON line per case."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from zeldaengine_amd import abi, engine as gpu_engine, scenes

FRACTIONS = (0.0, 0.01, 0.1, 1.0)
VARIANTS = 4                        # distinct update sets, used in turn


def variants(inst, frac, seed):
    """VARIANTS (first, values) ranges and (index, values) lists of frac * n instances, each nudged a little."""
    n = len(inst); m = int(round(frac * n))
    rng = np.random.default_rng(seed)
    out = []
    for v in range(VARIANTS):
        first = int(rng.integers(0, n - m + 1)) if m < n else 0
        idx = np.sort(rng.choice(n, m, replace=False)).astype(np.int32) if m < n else np.arange(n, dtype=np.int32)
        vals = inst[idx].copy()
        vals["InstancePosition"][:, :2] += rng.uniform(-0.02, 0.02, (m, 2)).astype(np.float32)
        rng_vals = inst[first:first + m].copy()
        rng_vals["InstancePosition"][:, :2] += rng.uniform(-0.02, 0.02, (m, 2)).astype(np.float32)
        out.append((first, rng_vals, idx, vals))
    return out


def run(config):
    cfg = scenes.config3(10000) if config == 3 else scenes.config4(1000000)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    inst = cfg["objects"][0]["instances"]
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    for frac in FRACTIONS:
        vs = variants(inst, frac, 7)
        dvs = [(torch.from_numpy(idx).to(dev), torch.from_numpy(vals.view(np.uint8).reshape(-1, 32).copy()).to(dev)) for _, _, idx, vals in vs]
        torch.cuda.synchronize()
        for form in ("host", "device"):
            if frac == 0.0 and form == "device":
                continue                                    # (0 %: no call at all, one row)

            def update(i):
                if frac == 0.0:
                    return
                first, rv, _, _ = vs[i % VARIANTS]
                if form == "host":
                    g.object_set_instances(0, rv, first)
                else:
                    d_idx, d_val = dvs[i % VARIANTS]
                    g.object_update_instances_async(0, d_val, d_idx, stream=ts)

            for i in range(5):
                update(i); g.render()
            g.finish(); ts.synchronize()
            t = time.perf_counter()
            for i in range(30):
                update(i); g.render()
            g.finish(); ts.synchronize()
            dt = (time.perf_counter() - t) / 30
            st = g.stats()
            print(json.dumps({"config": config, "instances": len(inst), "moved_pct": 100.0 * frac, "form": form if frac else "none",
                              "ms_per_frame": round(dt * 1e3, 4), "overflow": st["overflow"], "covered_pixels": st["covered_pixels"]}), flush=True)
    g.close()


if __name__ == "__main__":
    for c in (sys.argv[1:] or ["3", "4"]):
        run(int(c))
