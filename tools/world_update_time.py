"""What applying a world payload costs: zr_world_load_json against zr_world_update_json ("Reloading a world").

A content tree is synthesised in a temporary directory - the sample world's five Profabs (one model each, seven 512^2 PNGs per model),
six cubemap faces, a skydome image and mesh, a background - and the sample world (grass_01 and grass_02 at 10 000 instances) is loaded
from it at 1920 x 1080.  Then, for each way of applying a payload, from the settled state of that world (three frames after it):
  host_ms    wall time of the call
  frame_ms   GPU time, begin to end, of the first frame after it
as the median of five repetitions; between repetitions the world is put back with zr_world_update_json and settled again.
  load, identical       zr_world_load_json of the payload that is live (the baseline: the load path of the same build)
  update, identical     zr_world_update_json of the same
  update, camera        MainCamera.Position moved
  update, one light     one point light recoloured
  update, 10000->12000  grass_01's InstanceCount
  update, desc appended one more rock_02 entry at the end of Objects
  update, desc removed  the last entry of Objects (grass_02) gone
Run it under a time limit:
    timeout -k 10 600 python tools/world_update_time.py
One JSON line per case."""
import copy, json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from PIL import Image
from zeldaengine_amd import assets, engine as gpu_engine, scenes

REPS = 5
SUFFIX = ("_bc", "_m", "_r", "_n", "_ao", "_ev", "_ms")


def write_tree(root, dim=512):
    meshes = {"terrain": scenes.grid_plane(20.0, 4, 0.0), "rock_01": scenes.box((0.5, 0.5, 0.5), (0, 0, 0.5)),
              "rock_02": scenes.box((0.5, 0.5, 0.5), (0, 0, 0.5)), "grass_01": scenes.uv_sphere(16, 8), "grass_02": scenes.uv_sphere(16, 8)}
    images = scenes.synthetic_material(dim)
    for k, (name, (v, idx)) in enumerate(meshes.items()):
        for sub in ("models", "textures"):
            os.makedirs(os.path.join(root, "Profabs", name, sub))
        assets.write_obj(os.path.join(root, "Profabs", name, "models", name + ".obj"), v, idx)
        for img, suffix in zip(images, SUFFIX):
            Image.fromarray(np.roll(img, 13 * k, axis=1)).save(os.path.join(root, "Profabs", name, "textures", name + suffix + ".png"))
    os.makedirs(os.path.join(root, "Content", "Textures"))
    os.makedirs(os.path.join(root, "Content", "Models"))
    world = scenes.sample_world()
    cube = scenes.synthetic_cubemap(64)
    for face, name in zip(cube, world["Skydome"]["CubemapFileNames"]):
        Image.fromarray(np.ascontiguousarray(face)).save(os.path.join(root, "Content", "Textures", name))
    Image.fromarray(images[0]).save(os.path.join(root, "Content", "Textures", world["Skydome"]["SkydomeFileName"]))
    Image.fromarray(images[5]).save(os.path.join(root, "Content", "Textures", world["Background"]["BackgroundFileName"]))
    sv, si = scenes.uv_sphere(32, 16, 40.0)
    assets.write_obj(os.path.join(root, "Content", "Models", "skydome.obj"), sv, si)
    return world


def main():
    with tempfile.TemporaryDirectory() as root:
        base = write_tree(root)
        text = json.dumps(base)

        def edited(fn):
            w = copy.deepcopy(base)
            fn(w)
            return json.dumps(w)

        def camera(w): w["MainCamera"]["Position"] = [5.5, 4.5, 5.0]
        def light(w): w["PointLights"][3]["Color"] = [0.2, 0.8, 0.4]
        def grow(w): w["Objects"][3]["InstanceCount"] = 12000
        def append(w): w["Objects"].append(copy.deepcopy(w["Objects"][2]))
        def remove(w): del w["Objects"][-1]
        cases = [("load, identical", "load", text), ("update, identical", "update", text), ("update, camera", "update", edited(camera)),
                 ("update, one light", "update", edited(light)), ("update, 10000->12000", "update", edited(grow)),
                 ("update, desc appended", "update", edited(append)), ("update, desc removed", "update", edited(remove))]
        g = gpu_engine.Renderer(1920, 1080, 1024)
        g.set_asset_root(root)
        t = time.perf_counter()
        g.world_load_json(text)
        g.render(); g.finish()
        print(json.dumps({"case": "first load (Profabs read from disk) + frame", "host_ms": round((time.perf_counter() - t) * 1e3, 3)}), flush=True)

        def settle():
            for _ in range(3):
                g.render()
            g.finish()

        for name, how, payload in cases:
            host, frame, last = [], [], None
            for _ in range(REPS):
                g.world_update_json(text)
                settle()
                t = time.perf_counter()
                last = g.world_load_json(payload) if how == "load" else g.world_update_json(payload)
                host.append((time.perf_counter() - t) * 1e3)
                g.render(); g.finish()
                frame.append(g.frame_latencies(1)[0])
            print(json.dumps({"case": name, "host_ms": round(statistics.median(host), 3), "frame_ms": round(statistics.median(frame), 3),
                              "host_ms_min_max": [round(min(host), 3), round(max(host), 3)], "reps": REPS, "delta": last,
                              "overflow": g.stats()["overflow"]}), flush=True)
        g.close()


if __name__ == "__main__":
    main()
