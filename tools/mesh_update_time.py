"""Frame time with a mesh deformed every frame, config 3 (10 000 instances, 1920x1080) and config 4 (1 M instances, 3840x2160), each with
one non-instanced grid of about 1 M triangles under the spheres: no update, then the whole sphere mesh (559 vertices, every instance
draws it) and the whole grid (501 264 vertices), through the host form (zr_mesh_set_vertices) and the device form
(zr_mesh_update_vertices_async, tensors already on the GPU).  A refit costs the whole mesh whatever the range.  The protocol of
instance_update_time.py: 5 frames to settle, then the mean wall time of 30 frames with one update before each, finish() at the end.
Run it under a time limit:
    timeout -k 10 900 python tools/mesh_update_time.py [3|4 ...]
One JSON line per case."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from zeldaengine_amd import abi, engine as gpu_engine, scenes

VARIANTS = 4                        # distinct shapes, used in turn
GRID = 707                          # cells per side: 2 * 707^2 = 999 698 triangles


def fine_grid(size, n, z):
    """scenes.grid_plane's layout, built with numpy (n^2 cells, 2 n^2 triangles)."""
    v = np.zeros((n + 1) * (n + 1), abi.XkVertex)
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    v["Position"][:, 0] = (-size / 2 + size * j / n).ravel(); v["Position"][:, 1] = (-size / 2 + size * i / n).ravel(); v["Position"][:, 2] = z
    v["Normal"][:, 2] = 1.0; v["Color"][:] = 1.0
    v["TexCoord"][:, 0] = (j / n).ravel(); v["TexCoord"][:, 1] = (i / n).ravel()
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).ravel()
    idx = np.stack([a, a + 1, a + n + 2, a, a + n + 2, a + n + 1], axis=1).astype(np.uint32).ravel()
    return v, idx


def shapes(v, amp):
    out = []
    for k in range(VARIANTS):
        w = v.copy()
        w["Position"][:, 2] += (amp * np.sin(3.0 * v["Position"][:, 0] + 0.7 * k) * np.cos(2.0 * v["Position"][:, 1])).astype(np.float32)
        out.append(w)
    return out


def run(config):
    cfg = scenes.config3(10000) if config == 3 else scenes.config4(1000000)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
    gpu_engine.load_scene(g, cfg)
    extent = 16.0 if config == 3 else 120.0
    gv, gi = fine_grid(extent, GRID, -0.6)
    grid = g.mesh_create(gv, gi)
    g.object_add(grid)
    sv = cfg["objects"][0]["mesh"][0]
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    cases = [("none", None, None, None)]
    for name, mesh, verts, amp in (("sphere", 0, sv, 0.05), ("grid", grid, gv, 0.2)):
        hs = shapes(verts, amp)
        ds = [torch.from_numpy(h.view(np.uint8).reshape(-1, 44).copy()).to(dev) for h in hs]
        cases += [(name, mesh, "host", hs), (name, mesh, "device", ds)]
    torch.cuda.synchronize()
    for name, mesh, form, data in cases:
        def update(i):
            if form == "host":
                g.mesh_set_vertices(mesh, data[i % VARIANTS])
            elif form == "device":
                g.mesh_update_vertices_async(mesh, data[i % VARIANTS], stream=ts)

        for i in range(5):
            update(i); g.render()
        g.finish(); ts.synchronize()
        t = time.perf_counter()
        for i in range(30):
            update(i); g.render()
        g.finish(); ts.synchronize()
        dt = (time.perf_counter() - t) / 30
        st = g.stats()
        print(json.dumps({"config": config, "mesh": name, "vertices": 0 if mesh is None else len(data[0]), "form": form or "none",
                          "ms_per_frame": round(dt * 1e3, 4), "overflow": st["overflow"], "covered_pixels": st["covered_pixels"]}), flush=True)
    g.close()


if __name__ == "__main__":
    for c in (sys.argv[1:] or ["3", "4"]):
        run(int(c))
