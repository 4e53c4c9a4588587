"""A resting frame is one kernel launch (csrc/zr_frame_plan.h: ZrFramePlan::light_args; csrc/zr_lighting.hip: k_lighting_rest;
csrc/zr_lighting_host.cpp).

A frame that reads the plane of standing terms takes what it reads of XkView - camera position, light counts, the point lights - as a
kernel argument, reads what the GBuffer decides (the tile light list's box, which pixels are empty) from records the fill wrote, and
computes the empty pixel's colour inside the launch: no uniform upload, no one-pixel launch, no event wait.  The observable is
zr_get_light_keep's read_by_arg: the passes that ran as that one launch.  Every case asserts it, and every frame is compared bit for
bit with a ZR_FLAG_NO_LIST_REUSE twin, which keeps nothing; the still runs with the CPU oracle as well.  No tolerances.

Scenes and helpers are those of test_gpu_lighting_keep.py.  The point lights here reach far (radius 8).  The cleared pixel - world
position 0, normal (-1, -1, -1) / sqrt 3, roughness 0.01, F0 0.04 - gets a specular term from every light that reaches the origin, so
its colour moves with them, which is why it is computed every frame; at that roughness the term shows only within a hundredth of a
radian of the mirror direction, so one test puts a light exactly there (RStage.mirror).
"""
import numpy as np
import pytest

from test_gpu_gbuffer_keep import ViewChecker
from test_gpu_lighting_keep import LStage, _last, _pair
from test_gpu_round2_keep import BOX, SPHERES, Checker, _lights, _render, _same
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

CAP = 64                                   # ZR_REST_ARG_LIGHTS
START = ["ignored", "ignored", "filled"]   # two drawn frames, the first resting frame fills


def _far_lights(n, radius=8.0):
    d, p, s = _lights(n)
    p["Direction"][:, 3] = radius
    return d, p, s


class RStage(LStage):
    """The pile at a size and from a camera of the test's choosing."""

    def __init__(self, n_point=16, size=(160, 120), cam=None, zfar=45.0):
        super().__init__("pile", n_point)
        self.W, self.H = size
        if cam is not None:
            self.cam = cam
        self.zfar = zfar
        self.lights = _far_lights(n_point)
        self.roll_rate = 0.01 if n_point > 2 else 0.2
        self.mirror = ()                   # frames in which point light 0 stands where the cleared pixel mirrors it into the camera

    def uniforms(self, r, i):
        d, p, s = self.lights
        d = np.concatenate([d[:1]])
        d[0]["Position"][:3] = self.light; d[0]["Direction"][:3] = self.light
        r.update_uniforms(abi.make_camera(*self.cam, fov=50.0, zfar=self.zfar), d, p, s, self.roll_stage, self.roll_rate * i, 1.0 + 0.1 * i)
        if i in self.mirror:
            v = np.array(self.cam[0], dtype=np.float64); v /= np.linalg.norm(v)            # from the pixel (the origin) to the camera
            n = -np.ones(3) / np.sqrt(3.0)
            cam, sh, view = r.get_frame()
            view["PointLights"][0]["Position"][:3] = 5.0 * (2.0 * n.dot(v) * n - v)        # the mirror direction, five units out
            r.set_frame(cam, sh, view)


def _by_arg(g):
    return g.light_keep()["read_by_arg"]


def _pairs(st, eng, flags=0):
    return st.renderer(eng, flags), st.renderer(eng, flags | abi.FLAG_NO_LIST_REUSE)


def _empty(g):
    """mask of the pixels nothing was drawn to"""
    return g.gbuffer(0) >= 1.0


# ------------------------------------------------------------------------------------------------ 1. light counts

@pytest.mark.parametrize("n_point", [0, 1, 3, 4, 16, CAP, CAP + 1])
def test_still_run_by_light_count(oracle_lib, gpu_engine, n_point):
    """Eight still frames at 160 x 120.  3 and 4 straddle the tile light list's threshold; 65 lights are one too many for the argument:
    those frames read the plane through XkView, as ever.  Every frame is the twin's and the oracle's."""
    st = RStage(n_point)
    g, twin = _pairs(st, gpu_engine)
    chk = Checker(oracle_lib)
    did, colours = [], []
    for i in range(8):
        did.append(_pair(g, twin, st, i, "%d lights" % n_point))
        _same(chk.frame(st, i), g, "%d lights, frame %d" % (n_point, i))
        colours.append(g.color().copy())
    k = g.light_keep()
    print(did, k)
    assert did == START + ["read"] * 5, did
    assert k["read_by_arg"] == (0 if n_point > CAP else 5) and k["read"] == 5 and k["plane_bytes"] == 32 * st.W * st.H, k
    assert twin.light_keep()["read_by_arg"] == 0
    e = _empty(g)
    assert e.any() and not e.all(), "the frame needs empty and covered pixels"
    if n_point >= 16:       # the lights moved
        assert len({c.tobytes() for c in colours[3:]}) >= 3
    g.close(); twin.close()


def test_the_empty_pixels_colour_moves_with_the_lights(oracle_lib, gpu_engine):
    """From a camera the cleared pixel's normal faces, point light 0 stands in the mirror direction on frames 4 and 6: the colour of every
    empty pixel differs on those frames - computed inside the launch, from the slot's standing terms - and is the twin's and the oracle's."""
    st = RStage(16, cam=((-9.0, -7.0, 6.0), (0.0, 0.0, 1.0)))
    st.mirror = (4, 6)
    g, twin = _pairs(st, gpu_engine)
    chk = Checker(oracle_lib)
    did, px = [], []
    for i in range(8):
        did.append(_pair(g, twin, st, i, "mirror"))
        _same(chk.frame(st, i), g, "mirror, frame %d" % i)
        e = _empty(g)
        assert e.any() and not e.all()
        c = g.color()[e]
        assert (c == c[0]).all(), "empty pixels of one frame differ"
        px.append(c[0].tolist())
    print(did, px, g.light_keep())
    assert did == START + ["read"] * 5 and _by_arg(g) == 5, (did, g.light_keep())
    assert px[3] == px[5] == px[7] and px[4] == px[6] and px[4] != px[3], px
    g.close(); twin.close()


def test_light_count_crosses_the_cap_in_flight(gpu_engine):
    """Twelve frames enqueued without a host synchronisation: 16 lights, 65 from frame 5, 16 again from frame 8.  The light count is no
    standing uniform: nothing is filled again, the three frames in the middle read through XkView - uploaded for them although the
    frames before uploaded nothing - and the frames after are one launch again."""
    import torch
    dev = torch.device("cuda", 0)
    N, out = 12, {}
    for f in (abi.FLAG_NO_LIST_REUSE, 0):
        st = RStage(16)
        r = st.renderer(gpu_engine, f)
        col = [torch.zeros(st.W * st.H, dtype=torch.int32, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        did, by_arg = [], []
        for k in range(N):
            st.lights = _far_lights(CAP + 1 if 5 <= k < 8 else 16)
            st.uniforms(r, k)
            r.render()
            r.copy_frame_async(col[k].data_ptr(), None)
            did.append(_last(r)); by_arg.append(_by_arg(r))
        r.finish()
        assert r.stats()["overflow"] == 0
        out[f] = ([c.cpu().numpy() for c in col], did, by_arg)
        r.close()
    got, ref = out[0], out[abi.FLAG_NO_LIST_REUSE]
    for k in range(N):
        assert np.array_equal(got[0][k], ref[0][k]), "queued frame %d: %d pixels differ" % (k, int((got[0][k] != ref[0][k]).sum()))
    print(got[1], got[2])
    assert got[1] == START + ["read"] * 9, got[1]
    assert got[2] == [0, 0, 0, 1, 2, 2, 2, 2, 3, 4, 5, 6], got[2]
    assert ref[2] == [0] * N


# ------------------------------------------------------------------------------------------------ 2. frame shapes

def _first_empty_per_workgroup(e):
    """per workgroup (512 consecutive pixels of a 32 x 32 tile: 16 rows of it) the index of its first empty pixel, or -1"""
    H, W = e.shape
    first = []
    for ty in range(0, H, 32):
        for tx in range(0, W, 32):
            for half in (0, 16):
                blk = np.zeros((16, 32), dtype=bool)
                sub = e[ty + half:ty + half + 16, tx:tx + 32]
                blk[:sub.shape[0], :sub.shape[1]] = sub
                idx = np.flatnonzero(blk.reshape(-1))
                first.append(int(idx[0]) if len(idx) else -1)
    return first


def _last_wave_camera(oracle_lib):
    """A camera from beyond the ground plane's near edge: the rows under the edge are empty.  Its height is chosen, with the oracle, so
    that in some workgroup the first empty pixel lies in the last wave (pixels 448 .. 511: its rows 14 and 15)."""
    for z in np.linspace(6.0, 14.0, 33):
        st = RStage(16, cam=((0.0, -45.0, float(z)), (0.0, 0.0, 0.0)))
        o = oracle_lib.Oracle(st.W, st.H, st.SD)
        st.populate(o, oracle=True)
        st.uniforms(o, 0)
        o.render(0, 7)
        if any(f >= 448 for f in _first_empty_per_workgroup(o.gbuffer(0) >= 1.0)):
            return st.cam
    raise AssertionError("no camera height puts a workgroup's first empty pixel into its last wave")


@pytest.mark.parametrize("shape", ["partial_on_both_edges", "one_partial_tile", "no_empty_pixel", "only_empty_pixels", "first_empty_in_last_wave"])
def test_frame_shapes(oracle_lib, gpu_engine, shape):
    """150 x 120 has partial tiles on both edges, in several rows and columns of tiles (160 = 5 x 32 has none on the right); 40 x 24 is one partial tile; inside the pile no pixel is empty; looking away every pixel is, and every workgroup holds nothing
    else; from beyond the plane's edge a workgroup's first empty pixel lies in its last wave.  (160 x 120, partial tiles on the lower
    edge, is the size of every other test here.)"""
    if shape == "partial_on_both_edges":
        st = RStage(16, size=(150, 120))
    elif shape == "one_partial_tile":
        st = RStage(16, size=(40, 24))
    elif shape == "no_empty_pixel":
        st = RStage(16, cam=((0.5, -0.5, 5.0), (0.0, 0.0, 0.0)))
    elif shape == "only_empty_pixels":
        st = RStage(16, cam=((9.0, -7.0, 6.0), (30.0, -25.0, 40.0)))
    else:
        st = RStage(16, cam=_last_wave_camera(oracle_lib))
    g, twin = _pairs(st, gpu_engine)
    chk = Checker(oracle_lib)
    did = []
    for i in range(6):
        did.append(_pair(g, twin, st, i, shape))
        _same(chk.frame(st, i), g, "%s, frame %d" % (shape, i))
    e = _empty(g)
    print(shape, did, g.light_keep(), int(e.sum()), "empty pixels")
    assert did == START + ["read"] * 3 and _by_arg(g) == 3, (did, g.light_keep())
    if shape == "no_empty_pixel":
        assert not e.any()
    elif shape == "only_empty_pixels":
        assert e.all()
    elif shape == "first_empty_in_last_wave":
        assert any(f >= 448 for f in _first_empty_per_workgroup(e))
    else:
        assert e.any() and not e.all()
    g.close(); twin.close()


def test_non_finite_position(gpu_engine):
    """An instance so far out that its world position is inf in the GBuffer's f16: the record of its pixels is -inf .. +inf, every light
    is listed for the tile, and the frame is the twin's."""
    st = RStage(16, cam=((9.0, -7.0, 6.0), (70000.0, 0.0, 0.0)), zfar=1.0e6)
    inst = st.inst.copy()
    inst["InstancePosition"][0] = (70000.0, 0.0, 0.0); inst["InstancePScale"][0] = 10000.0
    st.inst = inst
    g, twin = _pairs(st, gpu_engine)
    did = [_pair(g, twin, st, i, "non-finite position") for i in range(6)]
    d = g.gbuffer(5)
    pos = np.stack([(d >> (16 * k)) & 0xFFFF for k in range(3)]).astype(np.uint16).view(np.float16)
    print(did, g.light_keep(), int(np.isinf(pos).any(axis=0).sum()), "pixels at inf")
    assert np.isinf(pos).any(), "no pixel's position is inf"
    assert did == START + ["read"] * 3 and _by_arg(g) == 3, (did, g.light_keep())
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 3. the stale device copy of XkView

@pytest.mark.parametrize("change", ["instances", "texture", "view9", "forward"])
def test_the_next_reader_of_xkview_uploads_it(gpu_engine, change):
    """zr_update_uniforms, frames that are one launch and upload nothing, then - with NO further zr_update_uniforms - a frame that reads
    the device copy of XkView: a drawn frame (an instance moved, a texture changed), the GBufferVis mosaic, forward shading.  It finds the
    copy stale and uploads: the frame is the twin's."""
    st = RStage(16)
    st.box_image = np.random.default_rng(7).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    g, twin = _pairs(st, gpu_engine)
    for i in range(6):
        last = _pair(g, twin, st, i, "start")
    assert last == "read" and _by_arg(g) == 3
    for r in (g, twin):
        if change == "instances":
            new = st.inst.copy(); new["InstancePosition"][:60, 2] += np.float32(2.5)
            r.object_set_instances(SPHERES, new[:60])
        elif change == "texture":
            r.object_set_texture(BOX, 0, 255 - st.box_image)
        elif change == "view9":
            r.set_debug_view(9)
        else:
            r.set_shading(True)
    for n in range(3):      # (no st.uniforms: the uniforms of frame 5 stand)
        for r in (g, twin):
            r.render(); r.finish()
        a, b = g.color(), twin.color()
        assert np.array_equal(a, b), "%s, frame %d after: %d pixels differ from the twin's" % (change, n, int((a != b).any(axis=2).sum()))
        assert _last(g) != "read" or n > 0 or change == "view9"
    assert _by_arg(g) == 3
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 4. views, background, other modes

def test_debug_views(oracle_lib, gpu_engine):
    """Views 1 - 5, 7 and 8 are one launch like view 0: the colour parked for the empty pixels goes through the view switch.  View 6 has
    the shortcut off: it fills again, every pixel, and reads as ever; back in view 0 the frame is one launch again, from that fill."""
    st = RStage(16)
    g, twin = _pairs(st, gpu_engine)
    chk = ViewChecker(oracle_lib)
    for i in range(4):
        last = _pair(g, twin, st, i, "start")
    assert last == "read" and _by_arg(g) == 1
    i, did, by_arg = 4, [], []
    for view in (1, 2, 3, 4, 5, 7, 8, 6, 6, 0, 0):
        for r in (g, twin):
            r.set_debug_view(view)
        chk.view = view
        did.append(_pair(g, twin, st, i, "view %d" % view)); by_arg.append(_by_arg(g))
        _same(chk.frame(st, i), g, "debug view %d" % view)
        i += 1
    print(did, by_arg)
    assert did == ["read"] * 7 + ["filled", "read", "read", "read"], did
    assert by_arg == [2, 3, 4, 5, 6, 7, 8, 8, 8, 9, 10], by_arg
    g.close(); twin.close()


def test_background_behind_the_empty_pixels(oracle_lib, gpu_engine):
    st = RStage(16)
    g, twin = _pairs(st, gpu_engine)
    chk = ViewChecker(oracle_lib)
    bg = scenes.synthetic_sky_image(48, 32)
    for r in (g, twin):
        r.set_background(bg)
    chk.bg = bg
    did = []
    for i in range(6):
        did.append(_pair(g, twin, st, i, "background"))
        _same(chk.frame(st, i), g, "background, frame %d" % i)
    assert did == START + ["read"] * 3 and _by_arg(g) == 3, (did, g.light_keep())
    assert _empty(g).any()
    g.close(); twin.close()


@pytest.mark.parametrize("mode", ["packed_tiles", "id_capture", "timing_interval_1", "serial", "staged_view_change"])
def test_other_modes(gpu_engine, mode):
    st = RStage(16)
    flags = {"packed_tiles": abi.FLAG_PACKED_TILES, "serial": abi.FLAG_SERIAL_PASSES}.get(mode, 0)
    g, twin = _pairs(st, gpu_engine, flags)
    for r in (g, twin):
        if mode == "id_capture":
            r.set_id_capture(True)
        r.set_timing_interval(1)      # (pass events on every frame: the kept passes record theirs on the stream that lights the frame)
    entry = "staged" if mode == "staged_view_change" else "render"
    did = []
    for i in range(6):
        did.append(_pair(g, twin, st, i, mode, entry))
        if mode == "packed_tiles":
            assert np.array_equal(g.read_tiles(), twin.read_tiles()), i
    assert did == START + ["read"] * 3 and _by_arg(g) == 3, (did, g.light_keep())
    if mode == "staged_view_change":
        # the view changes between the stages: to 8, which the launch serves; then to 9, whose mosaic reads XkView - that frame shades
        # every pixel itself, with uniforms uploaded behind the plan, and the plane is filled again by the frame after it
        for view, want in ((8, 4), (9, 4), (0, 4), (0, 5), (0, 6)):
            for r in (g, twin):
                st.uniforms(r, 6)
                r.render_shadow(); r.render_gbuffer(); r.set_debug_view(view); r.render_lighting(); r.finish()
            assert np.array_equal(g.color(), twin.color()), view
            print(view, _last(g), _by_arg(g))
            assert _by_arg(g) == want, (view, g.light_keep())
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 5. the next map

def test_a_light_that_stops_and_moves_again(oracle_lib, gpu_engine):
    """The directional light moves for two frames in the middle of a rest.  The map drawn after the rest goes into the copy that stood
    cleared through the rest (by the lighting launch of the frame that drew the map before it); the frames are the twin's and the
    oracle's, the map included."""
    st = RStage(16)
    g, twin = _pairs(st, gpu_engine)
    chk = Checker(oracle_lib)
    did = []
    for i in range(14):
        if i in (6, 7):
            st.light = (6.0 - 0.5 * (i - 5), 0.5, 14.0)
        did.append(_pair(g, twin, st, i, "light stops and moves"))
        _same(chk.frame(st, i), g, "frame %d" % i)
    print(did, g.light_keep())
    assert did[:6] == START + ["read"] * 3 and did[6] == "ignored" and did[7] == "ignored" and did[-1] == "read", did
    assert did.count("filled") == 2 and _by_arg(g) == did.count("read"), (did, g.light_keep())
    g.close(); twin.close()


def test_the_map_drawn_after_a_rest_is_a_fresh_contexts(gpu_engine):
    """96 x 64 (3 x 2 tiles, partial on both edges), a 64^2 map.  A map is drawn, the frame rests - a fill, then three frames of one
    launch - then the directional light moves twice: each new map is rasterised, without a clear of its own, into the copy a lighting
    launch cleared slice by slice (light_clear_next_slice) since it was last drawn into.  Map and colour are, byte for byte, those of a
    fresh context given the final state directly, whose first map is cleared by a fill.  (The host hands the clear to the first
    lighting pass after a draw: here k_lighting's, before and after the rest.  A frame that is one launch keeps its map, so
    k_lighting_rest is handed a clear only where that pass could not take it; its call is the same helper.)"""
    st = RStage(16, size=(96, 64))
    st.SD = 64
    g = st.renderer(gpu_engine)
    did, maps = [], []
    for i in range(8):
        if i >= 6:
            st.light = (6.0 - 0.5 * (i - 5), 0.5, 14.0)
        _render(g, st, i)
        did.append(_last(g)); maps.append(g.shadowmap().view(np.uint32).copy())
    print(did, g.light_keep())
    assert did == START + ["read"] * 3 + ["ignored"] * 2 and _by_arg(g) == 3, (did, g.light_keep())
    assert (maps[7] != 0x3F800000).any() and not np.array_equal(maps[7], maps[6]) and not np.array_equal(maps[6], maps[5])
    fresh = st.renderer(gpu_engine)
    _render(fresh, st, 7)
    assert np.array_equal(maps[7], fresh.shadowmap().view(np.uint32)), "%d texels of the map differ" % int((maps[7] != fresh.shadowmap().view(np.uint32)).sum())
    assert g.color().tobytes() == fresh.color().tobytes(), "%d pixels differ" % int((g.color() != fresh.color()).any(axis=2).sum())
    g.close(); fresh.close()
