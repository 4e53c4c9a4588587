"""Round 2 of the camera pass is kept while camera and scene stand still (zr_render, csrc/zr_frame_plan.h: ZrFramePlan::rounds; csrc/zr_frame_host.cpp: gbuffer_pass).

Round 1 draws what owned a pixel of the previous frame; when this frame's camera-pass inputs are that frame's bit for bit, nothing else
can own one now, and the frame enqueues no Hi-Z build, no k_select and no second round.  The observable is the pass time: a frame that
kept round 2 reports exactly 0.0 for "hiz" and "gbuffer2" (the library stores 0, it does not measure a gap), a frame that drew it the
time of its kernels.  Whatever is kept must be what would have been drawn: every frame here is compared bit for bit - the six GBuffer
planes, the map, the colour - with the CPU oracle (which draws every triangle every frame), its statistics with those of a
ZR_FLAG_NO_LIST_REUSE context (which draws round 2 every frame); where a sequence is queued without a host synchronisation, the frames
are compared with that context's.

Scenes: the crowd behind a wall of test_gpu_hiz.py (384 x 216, a 256^2 map) and the pile of test_gpu_shadow_keep.py (160 x 90, a 128^2
map).  Timing interval 1.  The point lights ride their spiral in every sequence: every frame's colour differs from the one before.
"""
import copy
import json
import math

import numpy as np
import pytest

from parity_util import compare_all
from test_gpu_resolve_lane import STAT_KEYS
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

PLANE, BOX, SPHERES, EXTRA = 0, 1, 2, 3            # mesh ids = object indices, in add order


def _lights(n):
    w = scenes.sample_world()
    d, _, s = scenes.lights_from_world(w)
    w["PointLights"] = scenes.sample_point_lights(n)
    _, p, _ = scenes.lights_from_world(w)
    return d, p, s


class Stage:
    """Everything a frame depends on, so that the oracle can be given the same state from scratch (it knows no visibility: what is
    hidden is left out of its scene)."""

    def __init__(self, kind):
        self.kind = kind
        if kind == "crowd":
            self.W, self.H, self.SD = 384, 216, 256
            self.cam = (0.0, -6.0, 1.2), (0.0, 0.0, 1.0)
            self.box = scenes.box((3.0, 0.15, 1.6), (0.0, 0.0, 1.6))
            self.inst = scenes.generate_instances(600, 1.0, 14.0, 0.3, 0.7, seed=5)
            self.lights = _lights(8)
        else:
            self.W, self.H, self.SD = 160, 90, 128
            self.cam = (9.0, -7.0, 6.0), (0.0, 0.0, 1.0)
            self.box = scenes.box((4.0, 4.0, 0.1), (0.0, 0.0, 6.0))
            self.inst = scenes.generate_instances(300, 0.5, 7.0, 0.2, 0.6, seed=3)
            self.lights = _lights(4)
        self.sphere = scenes.uv_sphere()
        self.light = (6.0, 0.0, 14.0)
        self.roll_stage = 0.0
        self.view_ulps = 0                          # set_frame: one element of the camera's View moved by that many ulps
        self.shown = None                           # mask over the spheres' instances, or None: all of them
        self.box_shown = True
        self.extra = False
        self.sky = False
        self.box_image = None                       # slot 0 of the box's material
        self.version = 0                            # of everything but camera, stage and light: the oracle of a version is built once
        self._keep = []

    def populate(self, r, oracle=False):
        r.set_cubemap(scenes.synthetic_cubemap(16))
        r.object_add(r.mesh_create(*scenes.grid_plane(60.0, 8, 0.0)))
        if self.box_shown or not oracle:
            mat = None
            if self.box_image is not None:
                mat, keep = abi.make_material([self.box_image] + [None] * 6)
                self._keep.append(keep)
            r.object_add(r.mesh_create(*self.box), mat)
        inst = self.inst if (self.shown is None or not oracle) else self.inst[self.shown]
        r.object_add(r.mesh_create(*self.sphere), None, inst)
        if self.extra:
            r.object_add(r.mesh_create(*scenes.box((1.0, 1.0, 1.0), (2.0, 1.0, 3.0))))
        if self.sky:
            r.set_skydome(*scenes.sky_dome(20.48, 16, 8), scenes.synthetic_sky_image(64, 32))

    def renderer(self, eng, flags=0):
        g = eng.Renderer(self.W, self.H, self.SD, flags=flags)
        self.populate(g)
        return g

    def uniforms(self, r, i):
        d, p, s = self.lights
        d[0]["Position"][:3] = self.light; d[0]["Direction"][:3] = self.light
        r.update_uniforms(abi.make_camera(*self.cam, fov=50.0), d, p, s, self.roll_stage, 0.01 * i, 1.0 + 0.1 * i)     # roll_light and time advance
        if self.view_ulps:
            cam, sh, view = r.get_frame()
            v = np.float32(cam["View"][12])
            for _ in range(self.view_ulps):
                v = np.nextafter(v, np.float32(np.inf))
            cam["View"][12] = v
            r.set_frame(cam, sh, view)


class Checker:
    """The oracle for the stage's current state.  What did not change is not drawn again by the oracle either: a frame of the same
    version, camera, light and stage re-runs its lighting pass only (zo_render's pass mask)."""

    def __init__(self, oracle_lib):
        self.lib, self.o, self.key = oracle_lib, None, None

    def frame(self, st, i):
        if self.o is None or self.key is None or self.key[0] != st.version:
            self.o = self.lib.Oracle(st.W, st.H, st.SD)
            st.populate(self.o, oracle=True)
            self.key = None
        key = (st.version, st.light, st.roll_stage, st.cam, st.view_ulps)
        st.uniforms(self.o, i)
        self.o.render(0, 7 if key != self.key else 4)
        self.key = key
        return self.o


def _render(g, st, i, entry="render"):
    """-> the frame's pass times"""
    st.uniforms(g, i)
    if entry == "staged":
        g.render_shadow(); g.render_gbuffer(); g.render_lighting()
    else:
        g.render()
    g.finish()
    return g.pass_times(1)


def _same(o, g, what):
    bad = {k: v for k, v in compare_all(o, g).items() if v}
    assert not bad, "%s: HIP path differs from the oracle: %r" % (what, bad)


def _kept(t):
    return t["hiz"] == 0.0 and t["gbuffer2"] == 0.0


def _not_vacuous(st):
    """round 2 has something to draw and something to reject: keeping it is not keeping nothing"""
    assert st["round1_survivors"] > 0 and st["hiz_culled"] > 0 and st["survivors"][1] > st["round1_survivors"], st


def _dev(a, width):
    import torch
    return torch.from_numpy(a.view(np.uint8).reshape(-1, width).copy()).to(torch.device("cuda", 0))


# ------------------------------------------------------------------------------------------------ 1. a still run

@pytest.mark.parametrize("kind,flags", [("crowd", 0), ("pile", 0), ("pile", abi.FLAG_SERIAL_PASSES)])
def test_still_camera_keeps_round_two(oracle_lib, gpu_engine, kind, flags):
    """Six frames, camera and scene still, the point lights moving: one round, both rounds, four frames that keep round 2.  Every frame is
    the oracle's; every frame's statistics are those of a twin that draws round 2 every frame."""
    st = Stage(kind)
    # (The twin also draws its shadow map every frame, the context keeps it and reports the pass as last run.  The pile is dense enough
    # for the shadow pass's occlusion culling, whose second drawn pass bins fewer entries than its first: without it a drawn pass counts
    # what the kept one counted, and the shadow slots of `survivors` and `bin_entries` can be compared like the camera's.)
    if kind == "pile":
        flags |= abi.FLAG_NO_SHADOW_OCCLUSION
    g = st.renderer(gpu_engine, flags)
    twin = st.renderer(gpu_engine, flags | abi.FLAG_NO_LIST_REUSE)
    chk = Checker(oracle_lib)
    times, colours = [], []
    for i in range(6):
        t = _render(g, st, i)
        tt = _render(twin, st, i)
        _same(chk.frame(st, i), g, "%s frame %d" % (kind, i))
        sg, sw = g.stats(), twin.stats()
        print("frame", i, "hiz", t["hiz"], "gbuffer2", t["gbuffer2"], {k: sg[k] for k in STAT_KEYS})
        assert {k: sg[k] for k in STAT_KEYS} == {k: sw[k] for k in STAT_KEYS}, "statistics of frame %d" % i
        assert sg["overflow"] == 0
        if i == 0:
            assert sg["round1_survivors"] == 0             # no history yet: one round
        if i == 1:
            _not_vacuous(sg)
        if i >= 1:
            assert tt["gbuffer2"] > 0.0, "the twin kept round 2 on frame %d" % i
        times.append(t); colours.append(g.color().copy())
    assert times[1]["hiz"] > 0.0 and times[1]["gbuffer2"] > 0.0, times[1]
    assert [_kept(t) for t in times[2:]] == [True] * 4, times
    assert not np.array_equal(colours[2], colours[5])          # the point lights did move
    g.close(); twin.close()


def test_without_hiz_nothing_is_kept(oracle_lib, gpu_engine):
    st = Stage("pile")
    g = st.renderer(gpu_engine, abi.FLAG_NO_HIZ)
    chk = Checker(oracle_lib)
    for i in range(4):
        t = _render(g, st, i)
        assert t["gbuffer2"] > 0.0, (i, t)                    # (one round: the gap between two records, never the stored 0)
        assert g.stats()["round1_survivors"] == 0
        _same(chk.frame(st, i), g, "no Hi-Z, frame %d" % i)
    g.close()


# ------------------------------------------------------------------------------------------------ 2. every change draws round 2 again

def test_every_change_of_the_camera_pass_draws_round_two_again(oracle_lib, gpu_engine):
    """Still frame (kept) - change - two drawn frames (the new state's frame by the oracle; round 2's time above 0) - kept frame, for
    every way the camera pass's result can change.  Two drawn frames: the first one's round 1 goes by the history of the state before the
    change (or, where the change renumbers the work items, there is no history and it is one round), so what its round 2 counted is not
    what a round 2 of the standing state counts; the second one's is, and from then on round 2 is kept (test_gpu_hiz.py holds the
    statistics of the second frame after a camera cut to that)."""
    st = Stage("pile")
    g = st.renderer(gpu_engine)
    chk = Checker(oracle_lib)

    def camera_one_ulp():
        st.view_ulps += 1

    def roll_stage():
        st.roll_stage = 0.3

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
        v = v.copy(); v["Position"][:, 2] *= np.float32(1.3)
        st.sphere = (v, idx); st.version += 1
        return v

    def set_vertices():
        g.mesh_set_vertices(SPHERES, deformed())

    def update_vertices_async():
        g.mesh_update_vertices_async(SPHERES, _dev(deformed(), 44))

    def instance_visibility():
        st.shown = (np.arange(len(st.inst)) % 3) != 0; st.version += 1
        g.object_set_instance_visibility(SPHERES, st.shown)

    def object_visibility():
        st.box_shown = False; st.version += 1
        g.object_set_visible(BOX, False)

    def object_add():
        g.object_add(g.mesh_create(*scenes.box((1.0, 1.0, 1.0), (2.0, 1.0, 3.0))))
        st.extra = True; st.version += 1

    def clear_and_reload():
        st.inst = scenes.generate_instances(250, 0.5, 7.0, 0.2, 0.6, seed=8); st.shown = None; st.box_shown = True; st.version += 1
        g.scene_clear(); st.populate(g)

    def set_limits():
        g.set_limits(8192, 4096)

    def skydome_on():
        st.sky = True; st.version += 1
        g.set_skydome(*scenes.sky_dome(20.48, 16, 8), scenes.synthetic_sky_image(64, 32))

    i = 0
    _render(g, st, i)
    _same(chk.frame(st, i), g, "first frame")
    i += 1
    assert not _kept(_render(g, st, i))
    _not_vacuous(g.stats())
    for change in (camera_one_ulp, roll_stage, set_instances, update_instances_async, set_vertices, update_vertices_async,
                   instance_visibility, object_visibility, object_add, clear_and_reload, set_limits, skydome_on):
        name = change.__name__
        i += 1
        t = _render(g, st, i)
        assert _kept(t), "%s: the still frame before it drew round 2 (%r)" % (name, t)
        _same(chk.frame(st, i), g, "still frame before " + name)
        change()
        i += 1
        t = _render(g, st, i)
        if g.stats()["round1_survivors"] == 0:      # (a new work numbering or new pools: no history, the frame is one round)
            assert name in ("object_add", "clear_and_reload", "set_limits", "skydome_on"), name
        assert t["gbuffer2"] > 0.0, "%s: the next frame kept a stale round 2 (%r)" % (name, t)
        _same(chk.frame(st, i), g, "frame after " + name)
        i += 1
        t = _render(g, st, i)
        assert t["gbuffer2"] > 0.0 and t["hiz"] > 0.0 and g.stats()["round1_survivors"] > 0, "%s: the second frame after it kept round 2 (%r)" % (name, t)
        _same(chk.frame(st, i), g, "second frame after " + name)
        i += 1
        t = _render(g, st, i)
        assert _kept(t), "%s: the third frame after it drew round 2 again (%r)" % (name, t)
        _same(chk.frame(st, i), g, "third frame after " + name)
        assert g.stats()["overflow"] == 0
    g.close()


def test_a_world_update_draws_round_two_again(oracle_lib, gpu_engine):
    from test_gpu_tiles_world import _oracle_from_renderer, _register_sample_profabs
    W, H, SD = 160, 120, 128
    cube = scenes.synthetic_cubemap(16)
    g = gpu_engine.Renderer(W, H, SD)
    g.set_cubemap(cube)
    ids = _register_sample_profabs(g)
    meshes = {ids["terrain"]: scenes.grid_plane(20.0, 4, 0.0), ids["rock_01"]: scenes.box((0.5, 0.5, 0.5), (0, 0, 0.5)), ids["grass_01"]: scenes.uv_sphere()}
    w = copy.deepcopy(scenes.sample_world())
    w["Objects"][3]["InstanceCount"] = 700

    def frame(what, kept):
        g.render(); g.finish()
        t = g.pass_times(1)
        assert _kept(t) == kept, (what, t)
        o = _oracle_from_renderer(oracle_lib, g, meshes, W, H, SD, cube)
        o.render()
        _same(o, g, what)
        o.close()

    g.world_load_json(json.dumps(w))
    g.render(); g.finish()
    frame("second frame of the world", False)
    frame("still frame", True)
    w["Objects"][2]["InstanceCount"] = 90                   # a draw resized, later bases shifted: the history is carried
    d = g.world_update_json(json.dumps(w))
    assert d["scene_changed"] == 1 and d["history_items"] > 0, d
    frame("frame after the update", False)
    assert g.stats()["round1_survivors"] > 0
    frame("second frame after the update", False)        # (round 1 by the standing world's own history: the counts a kept round 2 reports)
    frame("third frame after the update", True)
    g.close()


def test_a_texture_update_keeps_the_frame_exact(oracle_lib, gpu_engine):
    """No key depends on a texel: whether round 2 is drawn again is left open, the frames are the oracle's."""
    st = Stage("pile")
    st.box_image = np.random.default_rng(4).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    g = st.renderer(gpu_engine)
    chk = Checker(oracle_lib)
    for i in range(3):
        _render(g, st, i)
    _same(chk.frame(st, 2), g, "still frame")
    st.box_image = 255 - st.box_image; st.version += 1
    g.object_set_texture(BOX, 0, st.box_image)
    for i in (3, 4):
        _render(g, st, i)
        _same(chk.frame(st, i), g, "frame %d after the texture update" % (i - 2))
    g.close()


# ------------------------------------------------------------------------------------------------ 3. further sequences

def test_rest_cut_rest(oracle_lib, gpu_engine):
    """A 30 degree camera cut out of a rest: the plan behind kept frames is no tighter than behind the last drawn round 2."""
    st = Stage("crowd")
    g = st.renderer(gpu_engine)
    chk = Checker(oracle_lib)
    for i in range(4):
        t = _render(g, st, i)
    assert _kept(t)
    _same(chk.frame(st, 3), g, "rest")
    (x, y, z), look = st.cam
    a = math.radians(30.0)
    st.cam = (x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z), look
    t = _render(g, st, 4)
    assert t["gbuffer2"] > 0.0 and g.stats()["overflow"] == 0, (t, g.stats())
    _same(chk.frame(st, 4), g, "the cut")
    cut = g.stats()
    t = _render(g, st, 5)
    settled = g.stats()
    assert t["gbuffer2"] > 0.0 and settled["overflow"] == 0, (t, settled)
    _same(chk.frame(st, 5), g, "the frame after the cut")
    t = _render(g, st, 6)
    assert _kept(t) and g.stats()["overflow"] == 0
    _same(chk.frame(st, 6), g, "the second frame after the cut")
    # a kept round 2 reports the settled frame's counts, not the cut frame's
    assert {k: g.stats()[k] for k in STAT_KEYS} == {k: settled[k] for k in STAT_KEYS}
    print("bin_entries: cut", cut["bin_entries"], "settled", settled["bin_entries"])
    g.close()


def test_kept_round_two_beside_drawn_shadow_maps(oracle_lib, gpu_engine):
    """The light moves every other frame: round 2 is kept on frames that draw their map and on frames that keep it, through zr_render
    (whose resolve changes lanes with the map) and through the staged entry points."""
    st = Stage("pile")
    g, s = st.renderer(gpu_engine), st.renderer(gpu_engine)
    chk = Checker(oracle_lib)
    for i in range(8):
        st.light = (6.0 + 0.4 * (i // 2), 0.3 * (i // 2), 14.0)
        t, ts = _render(g, st, i), _render(s, st, i, "staged")
        assert (t["shadow"] > 0.0) == (ts["shadow"] > 0.0) == (i % 2 == 0), (i, t, ts)
        assert _kept(t) == _kept(ts) == (i >= 2), (i, t, ts)
        _same(chk.frame(st, i), g, "zr_render, frame %d" % i)
        _same(chk.o, s, "staged, frame %d" % i)
        assert {k: g.stats()[k] for k in STAT_KEYS} == {k: s.stats()[k] for k in STAT_KEYS}, i
    g.close(); s.close()


def test_eight_frames_in_flight(gpu_engine):
    """No finish() between the frames: each frame's colour and map are copied out in stream order and compared with the same sequence on
    the twin; the keep / draw pattern is read from the pass times afterwards."""
    import torch
    st = Stage("crowd")
    dev = torch.device("cuda", 0)
    out = {}
    N = 8
    for flags in (abi.FLAG_NO_LIST_REUSE, 0):
        r = st.renderer(gpu_engine, flags)
        col = [torch.zeros(st.W * st.H, dtype=torch.int32, device=dev) for _ in range(N)]
        sha = [torch.zeros(st.SD * st.SD, dtype=torch.int32, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        for k in range(N):
            st.uniforms(r, k)
            r.render()
            r.copy_frame_async(col[k].data_ptr(), sha[k].data_ptr())
        r.finish()
        stats = r.stats()
        assert stats["overflow"] == 0
        sums = [n * r.pass_times(n)["gbuffer2"] for n in range(1, N + 1)]      # S(n) = n * mean(n): the sum over the last n frames
        out[flags] = ([c.cpu().numpy() for c in col], [x.cpu().numpy() for x in sha], sums, stats, [r.gbuffer(t).copy() for t in range(6)])
        r.close()
    got, ref = out[0], out[abi.FLAG_NO_LIST_REUSE]
    for k in range(N):
        assert np.array_equal(got[1][k], ref[1][k]), "shadow map of queued frame %d" % k
        assert np.array_equal(got[0][k], ref[0][k]), "colour of queued frame %d: %d pixels differ" % (k, int((got[0][k] != ref[0][k]).sum()))
    assert not np.array_equal(got[0][3], got[0][7])
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[4], ref[4])), "GBuffer of the last queued frame"
    assert {k: got[3][k] for k in STAT_KEYS} == {k: ref[3][k] for k in STAT_KEYS}
    _not_vacuous(got[3])
    print("gbuffer2 ms, sums over the last n frames, keeping:", got[2], "drawing:", ref[2])
    # the last six frames kept round 2: exactly nothing; the second frame drew it (a kernel: > 1e-3 ms); the twin drew it on every frame
    assert got[2][5] == 0.0 and got[2][6] > 1e-3, got[2]
    assert all(ref[2][n] - (ref[2][n - 1] if n else 0.0) > 1e-3 for n in range(N - 1)), ref[2]
