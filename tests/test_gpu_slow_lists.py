"""GPU parity of the camera pass's slow list when BOTH of its halves hold triangles in one two-round frame.

A triangle that needs the clipper, or has an edge of 64 px or more, is not drawn by k_tile's record walk: k_geom lists it (round 1's in the
first half of the list, round 2's in the second) and the frame's last k_tile<LAST> draws both halves through the clipper, reading the
records with the helper the shadow pass's k_shadow_slow reads its own with.  The scene puts one object into each half by construction:

  A  a thin slab under and around the camera in both frames: it has vertices behind the eye, so its triangles go the clipper's way; it
     wins pixels in frame 1, so frame 2 draws it in round 1;
  B  a wall that frame 1's camera has behind it by more than its bounding radius (frustum-culled, never marked visible) and that fills
     frame 2's view from a few units away: its triangles span 64 px or more, and frame 2 draws it in round 2.

The preconditions are established from the oracle and the cameras alone, before the GPU renders anything.
"""
import numpy as np
import pytest

from parity_util import compare_all
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

W, H, SD = 96, 64, 64
SLAB = ((12.0, 12.0, 0.05), (0.0, 0.0, 0.0))         # A: half extents, centre
WALL = ((4.0, 0.2, 2.5), (0.0, -9.0, 2.6))           # B
CAMERAS = [((0.0, -3.0, 1.5), (0.0, 3.0, 0.5)),      # frame 1: looks along +y, the wall 6 units behind it
           ((0.0, -5.0, 1.5), (0.0, -9.0, 0.8))]     # frame 2: turned round and moved towards the wall, 3.8 units from it
N_BOX_TRIS = 12                                      # scenes.box: one meshlet of 12 triangles


def _scene(r):
    r.set_cubemap(scenes.synthetic_cubemap(16))
    r.object_add(r.mesh_create(*scenes.box(*SLAB)))
    r.object_add(r.mesh_create(*scenes.box(*WALL)))
    r.object_add(r.mesh_create(*scenes.uv_sphere(12, 6, 0.5)), None, scenes.generate_instances(6, 1.0, 4.0, 0.4, 0.8, seed=5))


def _lights():
    w = scenes.sample_world()
    d, _, s = scenes.lights_from_world(w)
    w["PointLights"] = scenes.sample_point_lights(4)
    _, p, _ = scenes.lights_from_world(w)
    return d, p, s


def _depth_along_view(cam, point):
    eye, at = np.array(cam[0]), np.array(cam[1])
    fwd = (at - eye) / np.linalg.norm(at - eye)
    return float(np.dot(np.array(point) - eye, fwd))


def test_both_halves_of_the_slow_list_in_one_frame(oracle_lib, gpu_engine):
    o = oracle_lib.Oracle(W, H, SD)
    _scene(o)
    d, p, s = _lights()
    cams = [abi.make_camera(pos, at, fov=45.0) for pos, at in CAMERAS]
    a_prims, b_prims = np.arange(0, N_BOX_TRIS), np.arange(N_BOX_TRIS, 2 * N_BOX_TRIS)

    # ---- preconditions, from the cameras and the oracle alone
    (bh, bc), radius = WALL, float(np.linalg.norm(WALL[0]))
    assert _depth_along_view(CAMERAS[0], bc) < -radius, "frame 1: the wall must lie behind the eye by more than its radius"
    (ah, ac) = SLAB
    for cam in CAMERAS:        # the slab has corners behind the eye and corners in front of it: its triangles need the clipper
        depths = [_depth_along_view(cam, (ac[0] + sx * ah[0], ac[1] + sy * ah[1], ac[2])) for sx in (-1, 1) for sy in (-1, 1)]
        assert min(depths) < 0.0 < max(depths), depths
    vis = []
    for i, cam in enumerate(cams):
        o.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
        o.render(0)
        vis.append(o.visibility().copy())
    for i in range(2):
        assert np.isin(vis[i], a_prims).sum() >= 1, "frame %d: the slab wins no pixel" % (i + 1)
    assert np.isin(vis[0], b_prims).sum() == 0 and np.isin(vis[1], b_prims).sum() >= 1
    # one triangle of the wall owns more than 65 pixels of one row in frame 2: its snapped box is 64 px wide or more
    widest = max(int((vis[1] == t).sum(axis=1).max()) for t in b_prims)
    assert widest >= 66, widest

    # ---- the two frames on the GPU, each against the oracle
    g = gpu_engine.Renderer(W, H, SD)
    _scene(g)
    for i, cam in enumerate(cams):
        for r in (o, g):
            r.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
        o.render(0)
        g.render(); g.finish()
        assert np.array_equal(o.shadowmap().view(np.uint32), g.shadowmap().view(np.uint32)), "shadow map, frame %d" % (i + 1)
        bad = {k: v for k, v in compare_all(o, g).items() if v}
        assert not bad, "frame %d: HIP path differs from the oracle: %r" % (i + 1, bad)
        st = g.stats()
        assert st["overflow"] == 0, st
    # frame 2 ran in two rounds and its second round drew something: the wall.  (zr_stats adds the rounds up in survivors[1] and names
    # round 1's share; the difference is slot 2 of the device's statistics block, round 2's survivors.)
    assert st["round1_survivors"] > 0 and st["survivors"][1] - st["round1_survivors"] > 0, st
    g.close()
