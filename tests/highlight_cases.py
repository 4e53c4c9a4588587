"""What tests/test_highlight_cpu.py (on the CPU oracle) and tests/test_gpu_highlight.py (on the renderer) share: the scene, the two
cameras, the highlight sets and the shapes.  The scene is the `spheres` scene of tests/test_gpu_ids.py, restated: a plane that crosses
the near plane, 400 instanced spheres, a box - slots 0, 1 .. 400, 401."""
import math

import numpy as np

from independent_scenes import Scene, _lights
from zeldaengine_amd import abi, scenes

SHAPES = [(7, 5), (33, 17), (66, 34), (130, 40), (257, 131), (410, 150), (192, 128)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
N_SPHERES = 400
N_SLOTS = N_SPHERES + 2
SLOT_BASE = [0, 1, 1 + N_SPHERES]
CAMERAS = ("side", "top")


def scene():
    s = Scene()
    s.add(scenes.grid_plane(40.0, 3, 0.0), [(90, 140, 60, 255), (0, 0, 0, 255), (200, 200, 200, 255), (127, 127, 255, 255),
                                             (255, 255, 255, 255), (0, 0, 0, 255), (255, 255, 255, 255)])
    s.add(scenes.uv_sphere(10, 5, 0.5), None, scenes.generate_instances(N_SPHERES, 0.5, 7.0, 0.3, 0.9, seed=17))
    s.add(scenes.box((0.6, 0.5, 0.7), (0.5, -0.5, 0.7)))
    return s


def camera(name):
    if name == "side":             # test_gpu_ids.py's _cam(0)
        return abi.make_camera((6.0 * math.cos(0.4), 6.0 * math.sin(0.4), 1.1), (0.0, 0.0, 0.4), fov=60.0)
    return abi.make_camera((0.5, 0.3, 9.0), (0.0, 0.0, 0.0), fov=60.0)      # looking down


def uniforms(r, cam_name, n_point=4):
    d, p, sp = _lights(1, n_point)
    r.update_uniforms(camera(cam_name), d, p, sp, 0.0, 0.0, 0.0)


def _flags(slots):
    f = np.zeros(N_SLOTS, dtype=np.uint8)
    f[list(slots)] = 1
    return f


ONE_SPHERE = 139                   # an instance that wins pixels under both cameras at every shape from 33 x 17 up (test_highlight_cpu.py holds that)
SETS = {
    "plane": _flags([0]),
    "spheres": _flags(range(1, 1 + N_SPHERES)),
    "odd_box": _flags(list(range(2, 1 + N_SPHERES, 2)) + [1 + N_SPHERES]),      # instances 1, 3, 5, ... and the box
    "one": _flags([1 + ONE_SPHERE]),
}


def apply_set(r, flags):
    """the set `flags` (a byte per slot) on a Renderer holding the scene, through zr_highlight_set object by object"""
    r.highlight_set(0, flags[0:1])
    r.highlight_set(1, flags[1:1 + N_SPHERES])
    r.highlight_set(2, flags[1 + N_SPHERES:])
