"""The shadow map is kept while its light and its casters stand still (zr_render, include/zelda_render.h).

A frame whose shadow-pass block, caster epoch and map buffer equal those of the last drawn pass enqueues no shadow pipeline: it lights
from the map that pass left.  The observable is the pass time: a kept frame reports exactly 0.0 for "shadow" (the library stores 0, it does
not measure a gap), a drawn frame the time of at least one kernel.  Whatever is kept must be what would have been drawn: every frame
here is compared bit for bit - map, GBuffer targets, colour - with the CPU oracle (which draws every triangle every frame), or, where the
sequence is queued without a host synchronisation, with a ZR_FLAG_NO_LIST_REUSE context (which draws its map every frame).

Scenes: the small pile of test_gpu_shadow_occlusion.py (plane + box + 300 instanced spheres, 160 x 90, a 128^2 map, 4 point lights) and
one that takes the instance-level work lists (65 536 instances), as test_gpu_frames_in_flight.py builds it.  Timing interval 1.
"""
import numpy as np
import pytest

from parity_util import compare_all
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

W, H, SD = 160, 90, 128
CAM = (9.0, -7.0, 6.0), (0.0, 0.0, 1.0)
PLANE, BOX, SPHERES, EXTRA = 0, 1, 2, 3            # mesh ids = object indices, in add order


def _lights():
    w = scenes.sample_world()
    d, _, s = scenes.lights_from_world(w)
    w["PointLights"] = scenes.sample_point_lights(4)
    _, p, _ = scenes.lights_from_world(w)
    return d, p, s


class Stage:
    """Everything a frame depends on, so that the oracle can be given the same state from scratch."""

    def __init__(self, n=300, sphere=None, seed=3):
        self.light = (6.0, 0.0, 14.0)
        self.roll_stage = 0.0
        self.cam = CAM
        self.shadow_scale = None                    # set_frame: the shadow block's Proj[0] scaled, nothing else
        self.sphere = scenes.uv_sphere(*sphere) if sphere else scenes.uv_sphere()
        self.inst = scenes.generate_instances(n, 0.5, 7.0, 0.2, 0.6, seed=seed)
        self.extra = False
        self.empty = False
        self.version = 0                            # of the geometry: the oracle of a version is built once

    def populate(self, r):
        r.set_cubemap(scenes.synthetic_cubemap(16))
        if self.empty:
            return
        r.object_add(r.mesh_create(*scenes.grid_plane(60.0, 8, 0.0)))
        r.object_add(r.mesh_create(*scenes.box((4.0, 4.0, 0.1), (0.0, 0.0, 6.0))))
        r.object_add(r.mesh_create(*self.sphere), None, self.inst)
        if self.extra:
            r.object_add(r.mesh_create(*scenes.box((1.0, 1.0, 1.0), (2.0, 1.0, 3.0))))

    def uniforms(self, r, i, lights):
        d, p, s = lights
        d[0]["Position"][:3] = self.light; d[0]["Direction"][:3] = self.light
        r.update_uniforms(abi.make_camera(*self.cam, fov=50.0), d, p, s, self.roll_stage, 0.01 * i, 1.0 + 0.1 * i)     # roll_light and time advance
        if self.shadow_scale is not None:
            cam, sh, view = r.get_frame()
            sh["Proj"][0] *= np.float32(self.shadow_scale)
            r.set_frame(cam, sh, view)


class Checker:
    """The oracle for the stage's current state.  Geometry that did not change is not drawn again by the oracle either: a frame of the
    same geometry version, light and stage re-runs its lighting pass only (zo_render's pass mask)."""

    def __init__(self, oracle_lib, lights):
        self.lib, self.lights, self.o, self.key = oracle_lib, lights, None, None

    def frame(self, st, i):
        if self.o is None or self.key is None or self.key[0] != st.version:
            self.o = self.lib.Oracle(W, H, SD)
            st.populate(self.o)
            self.key = None
        key = (st.version, st.light, st.roll_stage, st.cam, st.shadow_scale)
        st.uniforms(self.o, i, self.lights)
        self.o.render(0, 7 if key != self.key else 4)
        self.key = key
        return self.o


def _render(g, st, i, lights, entry="render"):
    st.uniforms(g, i, lights)
    if entry == "staged":
        g.render_shadow(); g.render_gbuffer(); g.render_lighting()
    elif entry == "geometry":
        g.render_geometry(); g.render_lighting()
    else:
        g.render()
    g.finish()
    return g.pass_times(1)["shadow"]


def _same(o, g, what):
    bad = {k: v for k, v in compare_all(o, g).items() if v}
    assert not bad, "%s: HIP path differs from the oracle: %r" % (what, bad)


@pytest.mark.parametrize("scene", ["pile", "worklist"])
def test_still_light_keeps_the_map(oracle_lib, gpu_engine, scene):
    """Five frames, light, stage and scene still, the point lights riding their spiral: one drawn pass, four kept; every frame's map is the
    oracle's and every frame's colour (which differs from frame to frame) too; the statistics stay those of the drawn pass."""
    lights = _lights()
    st = Stage() if scene == "pile" else Stage(65536, (8, 5))
    g = gpu_engine.Renderer(W, H, SD)
    st.populate(g)
    chk = Checker(oracle_lib, lights)
    times, stats, colours = [], [], []
    for i in range(5):
        times.append(_render(g, st, i, lights))
        _same(chk.frame(st, i), g, "%s frame %d" % (scene, i))
        stats.append(g.stats()); colours.append(g.color().copy())
    print("shadow ms per frame:", times)
    assert times[0] > 0.0 and times[1:] == [0.0] * 4, times
    assert (stats[0]["work_items"][0] >= 65536) == (scene == "worklist")
    for k in ("survivors", "bin_entries"):
        assert stats[4][k][0] == stats[0][k][0] and stats[0][k][0] > 0, (k, stats[0], stats[4])
    assert stats[4]["covered_shadow_texels"] == stats[0]["covered_shadow_texels"] > 0 and stats[4]["overflow"] == 0
    assert not np.array_equal(colours[0], colours[4])          # the point lights did move
    g.close()


def _dev(a, width):
    import torch
    return torch.from_numpy(a.view(np.uint8).reshape(-1, width).copy()).to(torch.device("cuda", 0))


def test_every_change_of_the_casters_draws_the_map_again(oracle_lib, gpu_engine):
    """Still frame - change - drawn frame (the new state's map, by the oracle) - kept frame, for every way the shadow pass's result can change."""
    import torch
    lights = _lights()
    st = Stage()
    g = gpu_engine.Renderer(W, H, SD)
    st.populate(g)
    chk = Checker(oracle_lib, lights)
    ext = torch.ones(SD * SD, dtype=torch.float32, device=torch.device("cuda", 0))

    def light():
        st.light = (6.3, 0.4, 14.0)

    def roll_stage():
        st.roll_stage = 0.3

    def shadow_mvp():
        st.shadow_scale = 0.9

    def object_add():
        g.object_add(g.mesh_create(*scenes.box((1.0, 1.0, 1.0), (2.0, 1.0, 3.0))))
        st.extra = True; st.version += 1

    def clear_and_reload():
        st.inst = scenes.generate_instances(250, 0.5, 7.0, 0.2, 0.6, seed=8); st.version += 1
        g.scene_clear(); st.populate(g)

    def moved():
        new = st.inst.copy()
        new["InstancePosition"][:60, 2] += np.float32(2.5); new["InstancePScale"][:60] *= np.float32(1.5)
        st.inst = new; st.version += 1
        return new

    def set_instances():
        g.object_set_instances(SPHERES, moved()[:60])

    def update_instances_async():
        g.object_update_instances_async(SPHERES, _dev(moved()[:60], 32))

    def deformed():
        v, idx = st.sphere
        v = v.copy(); v["Position"][:, 2] *= np.float32(1.4)
        st.sphere = (v, idx); st.version += 1
        return v

    def set_vertices():
        g.mesh_set_vertices(SPHERES, deformed())

    def update_vertices_async():
        g.mesh_update_vertices_async(SPHERES, _dev(deformed(), 44))

    def shadow_buffer_on():
        g.set_shadow_buffer(ext.data_ptr())

    def shadow_buffer_off():
        g.set_shadow_buffer(0)

    def set_limits():
        g.set_limits(8192, 4096)

    i = 0
    assert _render(g, st, i, lights) > 0.0
    _same(chk.frame(st, i), g, "first frame")
    for change in (light, roll_stage, shadow_mvp, object_add, clear_and_reload, set_instances, update_instances_async, set_vertices,
                   update_vertices_async, shadow_buffer_on, shadow_buffer_off, set_limits):
        name = change.__name__
        i += 1
        t_still = _render(g, st, i, lights)
        if name != "shadow_buffer_off":              # (a caller-owned map is drawn every frame)
            assert t_still == 0.0, "%s: the still frame before it was drawn (%r ms)" % (name, t_still)
        _same(chk.frame(st, i), g, "still frame before " + name)
        change()
        i += 1
        t_drawn = _render(g, st, i, lights)
        assert t_drawn > 0.0, "%s: the next frame kept a stale map" % name
        _same(chk.frame(st, i), g, "frame after " + name)
        if name == "shadow_buffer_on":
            assert np.array_equal(ext.cpu().numpy().view(np.uint32).reshape(SD, SD), chk.o.shadowmap().view(np.uint32))
            continue
        i += 1
        t_kept = _render(g, st, i, lights)
        assert t_kept == 0.0, "%s: the second frame after it was drawn again (%r ms)" % (name, t_kept)
        _same(chk.frame(st, i), g, "second frame after " + name)
    g.close()


def test_what_the_shadow_pass_does_not_read_keeps_the_map(oracle_lib, gpu_engine):
    lights = _lights()
    d, p, s = lights
    st = Stage()
    g = gpu_engine.Renderer(W, H, SD)
    st.populate(g)
    chk = Checker(oracle_lib, lights)
    assert _render(g, st, 0, lights) > 0.0

    def camera():
        st.cam = (-8.0, 6.0, 5.0), (0.5, 0.0, 1.0)

    def point_lights():
        p[1]["Color"][:3] = (0.2, 0.9, 0.4); p[2]["Color"][:3] = (3.0, 0.1, 0.1)
        if len(s):
            s[0]["Color"][:3] = (0.1, 0.1, 2.0)

    def id_capture():
        g.set_id_capture(True)

    for i, change in enumerate((camera, point_lights, id_capture), start=1):
        change()
        t = _render(g, st, i, lights)                # (roll_light and time advance with i)
        assert t == 0.0, "%s drew the shadow map again (%r ms)" % (change.__name__, t)
        _same(chk.frame(st, i), g, "frame after " + change.__name__)
    for view in (1, 3):                              # debug views: the lighting pass's business
        st.uniforms(g, 9, lights)
        g.render(view); g.finish()
        assert g.pass_times(1)["shadow"] == 0.0, view
        o = chk.frame(st, 9)
        o.render(view, 4)
        assert np.array_equal(o.color(), g.color()), "debug view %d" % view
    g.close()


STEPS = [0, 0, 0, 1, 1, 1, 2, 3, 3, 3, 3, 3]         # still x3, step, still x2, step, step, still x4
DRAWN = [k == 0 or STEPS[k] != STEPS[k - 1] for k in range(len(STEPS))]


def test_twelve_frames_in_flight(gpu_engine):
    """No finish() between the frames: each frame's colour and map are copied out in stream order and compared with the same sequence on a
    context that draws its map every frame.  The work-list scene; the keep / draw pattern is read from the pass times afterwards."""
    import torch
    lights = _lights()
    sd = 256
    st = Stage(65536, (8, 5))
    ref = gpu_engine.Renderer(W, H, sd, flags=abi.FLAG_NO_LIST_REUSE)
    g = gpu_engine.Renderer(W, H, sd)
    dev = torch.device("cuda", 0)
    out = {}
    for r in (ref, g):
        st.populate(r)
        col = [torch.zeros(W * H, dtype=torch.int32, device=dev) for _ in STEPS]
        sha = [torch.zeros(sd * sd, dtype=torch.int32, device=dev) for _ in STEPS]
        torch.cuda.synchronize()
        for k, step in enumerate(STEPS):
            st.light = (6.0 + 0.4 * step, 0.3 * step, 14.0)
            st.uniforms(r, k, lights)
            r.render()
            r.copy_frame_async(col[k].data_ptr(), sha[k].data_ptr())
        r.finish()
        assert r.stats()["overflow"] == 0 and r.stats()["work_items"][0] >= 65536
        # per-frame shadow times from the means over the last n frames: S(n) = n * mean(n) is the sum over the last n
        sums = [n * r.pass_times(n)["shadow"] for n in range(0 + 1, len(STEPS) + 1)]
        per_frame = [sums[0]] + [sums[n] - sums[n - 1] for n in range(1, len(STEPS))]
        out[r] = ([c.cpu().numpy() for c in col], [x.cpu().numpy() for x in sha], per_frame[::-1], sums)
    for k in range(len(STEPS)):
        assert np.array_equal(out[g][1][k], out[ref][1][k]), "shadow map of queued frame %d" % k
        assert np.array_equal(out[g][0][k], out[ref][0][k]), "colour of queued frame %d" % k
    assert len(np.unique(out[g][1][-1])) > 50
    print("shadow ms per frame, keeping:", out[g][2], "drawing:", out[ref][2])
    # A drawn pass runs at least one kernel, > 1e-3 ms; a kept frame adds exactly 0 to the sum, which the float mean returns to within
    # 12 * 2^-24 of itself (< 1e-5 ms for sums below 10 ms): 1e-4 ms separates the two.
    assert out[g][3][3] == 0.0                                 # the last four frames: exactly nothing
    assert [t > 1e-4 for t in out[g][2]] == DRAWN, out[g][2]
    assert all(t > 1e-4 for t in out[ref][2]), out[ref][2]
    ref.close(); g.close()


@pytest.mark.parametrize("mode", ["staged", "geometry", "serial", "forward"])
def test_entry_points_and_modes_decide_alike(oracle_lib, gpu_engine, mode):
    lights = _lights()
    st = Stage()
    flags = abi.FLAG_SERIAL_PASSES if mode == "serial" else 0
    ref = gpu_engine.Renderer(W, H, SD)
    g = gpu_engine.Renderer(W, H, SD, flags=flags)
    for r in (ref, g):
        st.populate(r)
        r.set_shading(mode == "forward")
    entry = mode if mode in ("staged", "geometry") else "render"
    chk = Checker(oracle_lib, lights) if mode != "forward" else None
    pattern = []
    for k, step in enumerate((0, 0, 1, 1, 1)):
        st.light = (6.0 + 0.4 * step, 0.3 * step, 14.0)
        t_ref = _render(ref, st, k, lights)
        t = _render(g, st, k, lights, entry)
        pattern.append((t_ref > 0.0, t > 0.0, t == 0.0))
        assert np.array_equal(ref.shadowmap().view(np.uint32), g.shadowmap().view(np.uint32)), (mode, k)
        assert np.array_equal(ref.color(), g.color()), (mode, k)
        if chk:
            _same(chk.frame(st, k), g, "%s frame %d" % (mode, k))
    drawn = [True, False, True, False, False]
    assert pattern == [(x, x, not x) for x in drawn], pattern
    ref.close(); g.close()


@pytest.mark.parametrize("what", ["no_list_reuse", "shadow_occlusion", "tile_rank", "external_buffer"])
def test_contexts_that_draw_every_frame(gpu_engine, what):
    """The exceptions (zr_render): recompute-everything and forced-variant contexts, a rank of a tile-partitioned frame, a caller-owned map."""
    import torch
    lights = _lights()
    st = Stage()
    flags = {"no_list_reuse": abi.FLAG_NO_LIST_REUSE, "shadow_occlusion": abi.FLAG_SHADOW_OCCLUSION}.get(what, 0)
    g = gpu_engine.Renderer(W, H, SD, tile_rank=0, tile_world=2 if what == "tile_rank" else 1, flags=flags)
    st.populate(g)
    ext = torch.ones(SD * SD, dtype=torch.float32, device=torch.device("cuda", 0))
    if what == "external_buffer":
        g.set_shadow_buffer(ext.data_ptr())
    times = [_render(g, st, i, lights) for i in range(4)]
    assert all(t > 0.0 for t in times), (what, times)
    g.close()


def test_a_context_without_casters_keeps_its_cleared_map(oracle_lib, gpu_engine):
    lights = _lights()
    st = Stage()
    st.empty = True
    g = gpu_engine.Renderer(W, H, SD)
    st.populate(g)
    chk = Checker(oracle_lib, lights)
    for i in range(3):
        t = _render(g, st, i, lights)
        assert i == 0 or t == 0.0, (i, t)
        assert np.all(g.shadowmap().view(np.uint32) == 0x3F800000)
        _same(chk.frame(st, i), g, "empty scene, frame %d" % i)
    g.close()


def test_a_lane_frame_behind_a_staged_frame_with_nothing_between(oracle_lib, gpu_engine):
    """zr_render, the staged entry points, zr_render again, no finish() in between: with the map kept the third frame's camera lane is
    enqueued right behind the staged frame's deferred-scene pass, which ran on the host's stream and shares the key buffer, the triangle
    records and the plan with it.  The work-list scene (a camera pipeline long enough to still be running)."""
    lights = _lights()
    st = Stage(65536, (8, 5))
    g = gpu_engine.Renderer(W, H, SD)
    st.populate(g)
    st.uniforms(g, 0, lights); g.render()
    st.uniforms(g, 1, lights); g.render_shadow(); g.render_gbuffer(); g.render_lighting()
    st.uniforms(g, 2, lights); g.render()
    g.finish()
    assert g.pass_times(1)["shadow"] == 0.0
    _same(Checker(oracle_lib, lights).frame(st, 2), g, "lane frame behind a staged frame")
    g.close()
