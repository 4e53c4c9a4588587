"""The lighting pass keeps the per-pixel terms the moving point lights do not touch (csrc/zr_frame_plan.h: ZrFramePlan::light_keep /
light_fill; csrc/zr_lighting_host.cpp; csrc/zr_lighting.hip: k_lighting's FILL and KEPT modes).

A frame that keeps both its camera pass and its shadow map lights a GBuffer and a map that are the previous frame's bit for bit.  Its
ShadowFactor, the directional lights' share of Direct and RefC then depend on a few hundred bytes of uniforms and the cubemap besides:
the first such frame stores them (fill), the later ones load them (read) and compute the point lights, Indirect and the compose only.
The observable is zr_get_light_keep: what the last frame's pass did with the plane - "ignored", "filled" or "read".  Whatever is read
must be what would have been computed: every frame here is compared bit for bit with a ZR_FLAG_NO_LIST_REUSE twin, which keeps nothing
and computes everything every frame, and the still runs with the CPU oracle as well.

The empty-pixel shortcut (off in debug view 6) is handled by the key: a fill made with the shortcut on skipped the pixels that took it,
so the first frame whose shortcut is off fills again, every pixel this time, and that plane serves both kinds of frame afterwards.

Scenes and helpers are those of test_gpu_round2_keep.py: the pile (160 x 90, a 128^2 map; partial tiles on both axes) and the crowd
(384 x 216, a 256^2 map).  The point lights ride their spiral in every sequence.
"""
import copy
import json

import numpy as np
import pytest

from test_gpu_gbuffer_keep import ViewChecker, _whole
from test_gpu_round2_keep import BOX, SPHERES, Checker, Stage, _lights, _render, _same
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu


class LStage(Stage):
    """Stage with the directional lights under the test's hand: their number (0: LightsCount[0] set to 0 behind zr_update_uniforms, the
    map still drawn from light 0's matrices), light 0's colour and intensity."""

    def __init__(self, kind, n_point=None, n_dir=1):
        super().__init__(kind)
        if n_point is not None:
            self.lights = _lights(n_point)
        self.n_dir, self.dir_color, self.dir_intensity = n_dir, None, None
        # roll_light per frame: two lights of radius 1.5 light little of the scene, so they move fast enough to cross what the camera sees
        self.roll_rate = 0.01 if n_point is None or n_point > 2 else 0.2

    def uniforms(self, r, i):
        d, p, s = self.lights
        d = np.concatenate([d[:1]] * max(self.n_dir, 1))
        d[0]["Position"][:3] = self.light; d[0]["Direction"][:3] = self.light
        if self.n_dir == 2:
            d[1]["Direction"][:3] = (-3.0, 5.0, 8.0); d[1]["Color"][:3] = (0.2, 0.5, 0.9)
        if self.dir_color is not None:
            d[0]["Color"][:3] = self.dir_color
        if self.dir_intensity is not None:
            d[0]["Color"][3] = self.dir_intensity
        r.update_uniforms(abi.make_camera(*self.cam, fov=50.0), d, p, s, self.roll_stage, self.roll_rate * i, 1.0 + 0.1 * i)
        if self.view_ulps or self.n_dir == 0:
            cam, sh, view = r.get_frame()
            v = np.float32(cam["View"][12])
            for _ in range(self.view_ulps):
                v = np.nextafter(v, np.float32(np.inf))
            cam["View"][12] = v
            if self.n_dir == 0:
                view["LightsCount"][0] = 0
            r.set_frame(cam, sh, view)


def _last(g):
    return g.light_keep()["last"]


def _pair(g, twin, st, i, what, entry="render"):
    """one frame on both, compared; -> what g's lighting pass did with the plane"""
    _render(g, st, i, entry); _render(twin, st, i, entry)
    a, b = g.color(), twin.color()
    assert np.array_equal(a, b), "%s, frame %d: %d pixels differ from the twin's" % (what, i, int((a != b).any(axis=2).sum()))
    assert _last(twin) == "ignored"
    return _last(g)


# ------------------------------------------------------------------------------------------------ 1. a still run

@pytest.mark.parametrize("kind,n_point,n_dir,flags", [("pile", 16, 1, 0), ("crowd", 16, 1, 0), ("pile", 2, 1, 0), ("crowd", 2, 1, 0), ("pile", 16, 0, 0),
                                                      ("pile", 16, 2, 0), ("pile", 16, 1, abi.FLAG_SERIAL_PASSES), ("pile", 2, 2, abi.FLAG_SERIAL_PASSES)])
def test_still_run_fills_once_and_reads(oracle_lib, gpu_engine, kind, n_point, n_dir, flags):
    """Eight frames, everything still but the point lights (16: the tile lists are on; 2: the instantiation without them).  Frames 0 and 1
    draw, frame 2 keeps camera pass and map and fills, frames 3 - 7 read.  Every frame is the twin's and the oracle's."""
    st = LStage(kind, n_point, n_dir)
    g, twin = st.renderer(gpu_engine, flags), st.renderer(gpu_engine, flags | abi.FLAG_NO_LIST_REUSE)
    chk = Checker(oracle_lib)
    did, colours = [], []
    for i in range(8):
        did.append(_pair(g, twin, st, i, kind))
        _same(chk.frame(st, i), g, "%s frame %d" % (kind, i))
        colours.append(g.color().copy())
    print(did, g.light_keep())
    assert did == ["ignored", "ignored", "filled"] + ["read"] * 5, did
    k = g.light_keep()
    assert (k["ignored"], k["filled"], k["read"]) == (2, 1, 5) and k["plane_bytes"] == 32 * st.W * st.H, k
    assert twin.light_keep()["plane_bytes"] == 0
    # not vacuous: the point lights did move between two frames that read, pixels are covered, some of them in shadow
    assert len({c.tobytes() for c in colours[3:]}) >= 3, "the frames that read the plane are all alike"
    assert g.stats()["covered_pixels"] > 0
    g.set_debug_view(8); twin.set_debug_view(8)
    assert _pair(g, twin, st, 8, "view 8") == "read"
    v8 = g.color()
    assert (v8[..., 0] < 255).any() and (v8[..., 0] == 255).any(), "ShadowFactor is 1 everywhere"
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 2. every change ends it

def test_every_change_ends_the_keep(gpu_engine):
    """rest (read) - change - frames compared with the twin - rest again (read), for everything the standing terms depend on.  The frame
    after the change never reads; the plane is filled again before it is read again.  A directional light's colour or intensity alone
    leaves GBuffer and map standing: only the uniform comparison catches it, and the very next frame fills."""
    import torch
    st = LStage("pile", 16)
    st.box_image = np.random.default_rng(4).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    g, twin = st.renderer(gpu_engine), st.renderer(gpu_engine, abi.FLAG_NO_LIST_REUSE)
    both = (g, twin)
    ext = [torch.full((st.SD * st.SD,), 1.0, dtype=torch.float32, device=torch.device("cuda", 0)) for _ in both]
    torch.cuda.synchronize()

    def dir_colour():
        st.dir_color = (0.9, 0.4, 0.1)

    def dir_intensity():
        st.dir_intensity = 3.5

    def dir_direction():
        st.light = (5.0, 2.0, 13.0)

    def cubemap_levels():           # LightsCount[3] follows the cubemap's mip count
        for r in both:
            r.set_cubemap(scenes.synthetic_cubemap(8))

    def cubemap_texels():           # same size, other texels
        cube = [255 - f for f in scenes.synthetic_cubemap(8)]
        for r in both:
            r.set_cubemap(cube)

    def camera_one_ulp():
        st.view_ulps += 1

    def instance_transform():
        new = st.inst.copy()
        new["InstancePosition"][:60, 2] += np.float32(2.5)
        st.inst = new
        for r in both:
            r.object_set_instances(SPHERES, new[:60])

    def hidden_instance():
        shown = (np.arange(len(st.inst)) % 3) != 0
        for r in both:
            r.object_set_instance_visibility(SPHERES, shown)

    def deformed_mesh():
        v, idx = st.sphere
        v = v.copy(); v["Position"][:, 2] *= np.float32(1.3)
        st.sphere = (v, idx)
        for r in both:
            r.mesh_set_vertices(SPHERES, v)

    def texture_update():
        st.box_image = 255 - st.box_image
        for r in both:
            r.object_set_texture(BOX, 0, st.box_image)

    def shading_forward():
        for r in both:
            r.set_shading(True)

    def shading_back():
        for r in both:
            r.set_shading(False)

    def caller_owned_map():
        for r, t in zip(both, ext):
            r.set_shadow_buffer(t.data_ptr())

    def library_map_again():
        for r in both:
            r.set_shadow_buffer(None)

    never = ("shading_forward", "caller_owned_map")        # while these hold, no frame fills or reads
    uniforms_only = ("dir_colour", "dir_intensity", "cubemap_levels", "cubemap_texels")
    i = 0
    for _ in range(4):
        last = _pair(g, twin, st, i, "start"); i += 1
    assert last == "read"
    for change in (dir_colour, dir_intensity, dir_direction, cubemap_levels, cubemap_texels, camera_one_ulp, instance_transform, hidden_instance,
                   deformed_mesh, texture_update, shading_forward, shading_back, caller_owned_map, library_map_again):
        name = change.__name__
        filled = g.light_keep()["filled"]
        change()
        did = []
        for _ in range(5):
            did.append(_pair(g, twin, st, i, "after " + name)); i += 1
        print(name, did)
        assert did[0] != "read", "%s: the frame after it read a stale plane" % name
        if name in never:
            assert did == ["ignored"] * 5, (name, did)
            continue
        if name in uniforms_only:
            assert did == ["filled"] + ["read"] * 4, (name, did)
        assert did[-1] == "read" and did.count("filled") == 1 and g.light_keep()["filled"] == filled + 1, (name, did)
        assert did.index("filled") < did.index("read") and "ignored" not in did[did.index("filled"):], (name, did)
    assert g.stats()["overflow"] == 0
    g.close(); twin.close()


def test_a_world_reload_and_a_second_scene_end_the_keep(gpu_engine):
    """A world applied again with the same camera and lights but other objects, then a second scene loaded into the same context: the
    frames after either never read what the old objects left, and the rest that follows fills and reads again."""
    from test_gpu_tiles_world import _register_sample_profabs
    W, H, SD = 160, 120, 128
    pair = [gpu_engine.Renderer(W, H, SD, flags=f) for f in (0, abi.FLAG_NO_LIST_REUSE)]
    g, twin = pair
    w = copy.deepcopy(scenes.sample_world())
    w["Objects"][3]["InstanceCount"] = 700
    for r in pair:
        r.set_cubemap(scenes.synthetic_cubemap(16))
        _register_sample_profabs(r)
        r.world_load_json(json.dumps(w))
    n = [0]

    def frames(what, count):
        did = []
        for _ in range(count):
            for r in pair:
                r.world_update_uniforms(0.0, 0.01 * n[0], 1.0)
                r.render(); r.finish()
            n[0] += 1
            assert np.array_equal(g.color(), twin.color()), (what, n[0])
            did.append(_last(g))
        print(what, did)
        return did

    assert frames("the world", 5) == ["ignored", "ignored", "filled", "read", "read"]
    w["Objects"][2]["InstanceCount"] = 90
    for r in pair:
        assert r.world_update_json(json.dumps(w))["scene_changed"] == 1
    did = frames("the world with other objects", 5)
    assert did[0] == "ignored" and did[-1] == "read" and did.count("filled") == 1, did
    st = LStage("pile", 16)
    for r in pair:
        r.scene_clear(); st.populate(r)
    did = []
    for i in range(5):
        did.append(_pair(g, twin, st, i, "second scene"))
    assert did == ["ignored", "ignored", "filled", "read", "read"], did
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 3. views

def test_views_and_background_read_the_plane(oracle_lib, gpu_engine):
    """While resting, debug views 0 - 9 and back, and the background image on and off.  Every frame is the twin's (views 0 - 8: the
    oracle's too).  All of them read the plane - each derives from the decode plus the seven kept floats - but the first frame in view 6:
    its empty-pixel shortcut is off, the plane was filled with it on, so it fills again, every pixel; the views after it read that."""
    st = LStage("pile", 16)
    g, twin = st.renderer(gpu_engine), st.renderer(gpu_engine, abi.FLAG_NO_LIST_REUSE)
    chk = ViewChecker(oracle_lib)
    for i in range(4):
        last = _pair(g, twin, st, i, "start")
    assert last == "read"
    i, did = 4, {}
    bg = scenes.synthetic_sky_image(48, 32)
    for step, view in enumerate(list(range(10)) + [6, 0, 0, 0]):
        for r in (g, twin):
            r.set_debug_view(view)
            if step == 4:
                r.set_background(bg)
            if step == 12:
                r.set_sky_flags(True, False)
            if step == 13:
                r.set_sky_flags(True, True)
        if step == 4:
            chk.bg = bg
        chk.view = view
        did[step] = _pair(g, twin, st, i, "view %d" % view)
        assert _whole(g.pass_times(1)), view
        if view != 9 and step not in (12,):
            _same(chk.frame(st, i), g, "debug view %d" % view)
        i += 1
    print(did)
    assert [did[s] for s in range(14)] == ["read"] * 6 + ["filled"] + ["read"] * 7, did
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 4. in flight

@pytest.mark.parametrize("flags", [0, abi.FLAG_SERIAL_PASSES])
def test_frames_in_flight_with_a_light_change_in_the_middle(gpu_engine, flags):
    """Fourteen frames enqueued without a host synchronisation, each copied out in stream order; the directional light changes colour
    at frame 7.  One plane serves them all: every lighting pass runs on the host's stream, in frame order."""
    import torch
    dev = torch.device("cuda", 0)
    N, out = 14, {}
    for f in (abi.FLAG_NO_LIST_REUSE, 0):
        st = LStage("crowd", 16)
        r = st.renderer(gpu_engine, flags | f)
        col = [torch.zeros(st.W * st.H, dtype=torch.int32, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        did = []
        for k in range(N):
            if k == 7:
                st.dir_color = (0.2, 0.9, 0.3)
            st.uniforms(r, k)
            r.render()
            r.copy_frame_async(col[k].data_ptr(), None)
            did.append(_last(r))
        r.finish()
        assert r.stats()["overflow"] == 0
        out[f] = ([c.cpu().numpy() for c in col], did)
        r.close()
    got, ref = out[0], out[abi.FLAG_NO_LIST_REUSE]
    for k in range(N):
        assert np.array_equal(got[0][k], ref[0][k]), "queued frame %d: %d pixels differ" % (k, int((got[0][k] != ref[0][k]).sum()))
    assert got[1] == ["ignored", "ignored", "filled"] + ["read"] * 4 + ["filled"] + ["read"] * 6, got[1]
    assert ref[1] == ["ignored"] * N
    assert not np.array_equal(got[0][5], got[0][6]) and not np.array_equal(got[0][6], got[0][7])
