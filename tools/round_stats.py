"""Per-round counters of the camera pass on the benchmark scene (ZR_DUMP_STATS=1 with a -DZR_DIAG library prints the raw device block)."""
import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zeldaengine_amd import engine as gpu_engine, scenes
cfg = scenes.config3(10000, cube_dim=64)
g = gpu_engine.Renderer(cfg["width"], cfg["height"], 1024)
gpu_engine.load_scene(g, cfg)
for i in range(5): g.render()
g.finish()
print(g.stats())
g.close()
