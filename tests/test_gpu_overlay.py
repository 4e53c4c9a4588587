"""Overlaying lines on the renderer (zr_overlay_set / _get, zr_set_overlay_style, zr_read_color_overlaid, zr_copy_frame_overlaid_async,
zr_set_frame_delta_overlay).

Every overlaid frame is held, byte for byte, to tests/overlay_reference.py applied to zr_read_color's frame, zr_read_gbuffer(0)'s depth
plane and the frame's PVM (from zr_get_frame, multiplied as the host multiplies it); scaled ones to tests/frame_scale_reference.py of
that; with a highlight underneath to tests/highlight_reference.py first; every delivery of changes to tests/frame_delta_reference.py of
two such frames.  Scene, cameras and shapes are tests/highlight_cases.py's, the lists tests/overlay_cases.py's, and
tests/test_overlay_cpu.py holds, on the CPU oracle, that they put visible, hidden and cleared-depth pixels where the kernels
(zr_overlay.hip) can go wrong.  The shapes: 66 x 34 (W % 4 == 2: the pixel-by-pixel loads; a two-pixel last tile both ways), 257 x 131
(a one-pixel last tile), 192 x 128 (everything aligned: the 16-byte loads and, by the destination, either store arm)."""
import numpy as np
import pytest

import frame_delta_reference as fdr
import frame_scale_reference as fsr
import highlight_cases as hc
import highlight_reference as hr
import overlay_cases as oc
import overlay_reference as ovr
import test_gpu_highlight as hl
from independent_scenes import _lights
from zeldaengine_amd import abi

pytestmark = pytest.mark.gpu

_Dest, _first, SENTINEL8 = hl._Dest, hl._first, hl.SENTINEL8


@pytest.fixture(scope="module")
def lights():
    return _lights(1, 4)


def _abi_style(st):
    return abi.make_overlay_style(st["depth_bias"], st["hidden_opacity"])


def _pvm(r):
    """the PVM of the uniforms as they stand (the frame's, while nothing was set after it)"""
    mvp = r.get_frame()[0]
    return ovr.pvm_of(mvp["Proj"], mvp["View"], mvp["Model"])


def _statement(h, pvm, seg, st, s=1, highlight=False):
    """what an overlaid delivery at scale s must hold"""
    base = h.r.color()
    if highlight:
        base = hr.highlight(base, h.mask(), h.style)
    out = ovr.overlay(base, h.r.gbuffer(0).astype(np.float32), pvm, seg, st)
    return out if s == 1 else fsr.downscale(out, s)


def _styled(h, st):
    h.r.overlay_style(_abi_style(st))
    h.ov_style = dict(st)


def _both_forms(h, want, s, highlight, k, what):
    got = h.r.read_color_overlaid(s, highlight)
    assert got.shape == want.shape and np.array_equal(got, want), "%s host form, scale %d: %s" % (what, s, _first(got, want))
    d = _Dest(want.shape[1], want.shape[0], offset=4 * ((k + s) % 2))
    h.r.copy_frame_overlaid_async(s, highlight, d.ptr())
    h.r.finish()
    got = d.read()
    assert np.array_equal(got, want), "%s device form, scale %d: %s" % (what, s, _first(got, want))


# ------------------------------------------------------------------------------------------------ rendered frames

MODES = ("deferred", "forward", "debug")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H", oc.SHAPES, ids=oc.SHAPE_IDS)
def test_rendered_frames_both_cameras_every_list(gpu_engine, lights, W, H, mode):
    """deferred shading runs every list, the forward variant and debug view 3 four of them; scales 2 and 3 and the highlight underneath
    on every third case; the frame, the ids and the GBuffer are untouched afterwards"""
    h = hl._Host(gpu_engine, lights, W, H, forward=mode == "forward")
    try:
        if mode == "debug":
            h.r.set_debug_view(3)
        h.styled(hr.style("fill", 2))
        h.select(hc.SETS["odd_box"])
        names = oc.GPU_LISTS if mode == "deferred" else ("slopes", "near_far", "guard", "many")
        k = 0
        for cam in oc.CAMERAS:
            h.frame(cam)
            before = hl._planes(h.r)
            pvm = _pvm(h.r)
            lists = oc.lists(pvm, W, H)
            for name in names:
                seg = lists[name]
                st = list(oc.STYLES.values())[k % 2]
                h.r.overlay_set(seg)
                _styled(h, st)
                assert h.r.overlay_get().tobytes() == seg.tobytes()
                want = _statement(h, pvm, seg, st)
                assert np.array_equal(gpu_engine.frame_overlay(before[0], before[3], pvm, seg, _abi_style(st)), want)
                assert not np.array_equal(want, before[0])
                _both_forms(h, want, 1, False, k, "%s/%s" % (cam, name))
                if k % 3 == 0:
                    for s in (2, 3):
                        _both_forms(h, fsr.downscale(want, s), s, False, k, "%s/%s" % (cam, name))
                    wh = _statement(h, pvm, seg, st, 1, True)
                    assert not np.array_equal(wh, want)
                    _both_forms(h, wh, 1, True, k, "%s/%s highlighted" % (cam, name))
                    _both_forms(h, fsr.downscale(wh, 2), 2, True, k, "%s/%s highlighted" % (cam, name))
                k += 1
            after = hl._planes(h.r)
            for a, b in zip(before, after):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "an overlaid delivery changed the frame, the ids or a GBuffer plane"
            assert np.array_equal(h.r.color_scaled(2), fsr.downscale(before[0], 2))                 # the scaled forms deliver the plain frame
            assert np.array_equal(h.r.color_highlighted(1), hr.highlight(before[0], h.mask(), h.style))
    finally:
        h.close()


def test_styles_and_xray(gpu_engine, lights):
    """hidden_opacity 0 and 96, depth_bias 0 and 1e-4, and the list's XRAY twin"""
    W, H = 66, 34
    h = hl._Host(gpu_engine, lights, W, H, capture=False)
    try:
        h.frame("side")
        pvm = _pvm(h.r)
        seg = oc.lists(pvm, W, H)["seams"]
        xr = seg.copy()
        xr["flags"] |= ovr.XRAY
        outs = []
        for k, (bias, hidden) in enumerate(((0.0, 0), (0.0, 96), (1e-4, 0), (1e-4, 96))):
            st = {"depth_bias": bias, "hidden_opacity": hidden}
            h.r.overlay_set(seg)
            _styled(h, st)
            got = h.r.overlay_style()
            assert (got.depth_bias, got.hidden_opacity) == (np.float32(bias), hidden)
            want = _statement(h, pvm, seg, st)
            _both_forms(h, want, 1, False, k, "bias %g hidden %d" % (bias, hidden))
            outs.append(want)
            h.r.overlay_set(xr)
            _both_forms(h, _statement(h, pvm, xr, st), 1, False, k, "xray")
        assert not np.array_equal(outs[0], outs[1]), "no pixel of the list is hidden"
    finally:
        h.close()


def test_an_empty_list_an_opacity_0_list_and_the_cap(gpu_engine, lights):
    W, H = 257, 131
    h = hl._Host(gpu_engine, lights, W, H, capture=False)
    try:
        h.frame("side")
        frame, pvm = h.r.color(), _pvm(h.r)
        assert len(h.r.overlay_get()) == 0
        st = h.r.overlay_style()
        assert (st.depth_bias, st.hidden_opacity, list(st.reserved)) == (0.0, 0, [0, 0])
        _both_forms(h, frame, 1, False, 0, "no list")
        _both_forms(h, fsr.downscale(frame, 2), 2, False, 0, "no list")
        lists = oc.lists(pvm, W, H)
        clear = lists["slopes"].copy()
        clear["rgba"][:, 3] = 0
        h.r.overlay_set(clear)
        _styled(h, {"depth_bias": 0.0, "hidden_opacity": 255})
        _both_forms(h, frame, 1, False, 1, "opacity 0")
        big = lists["max"]
        assert len(big) == abi.OVERLAY_MAX_SEGMENTS
        h.r.overlay_set(big)
        _styled(h, oc.STYLES["biased"])
        want = _statement(h, pvm, big, oc.STYLES["biased"])
        assert int((want != frame).any(axis=2).sum()) > W * H // 4
        _both_forms(h, want, 1, False, 0, "the cap")
        h.r.overlay_set(None)
        assert len(h.r.overlay_get()) == 0
        _both_forms(h, frame, 1, False, 1, "cleared")
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ frames in flight, the camera, a rest

FLIGHT = [(257, 131), (192, 128)]


@pytest.mark.parametrize("W,H", FLIGHT, ids=["%dx%d" % s for s in FLIGHT])
def test_device_form_four_frames_in_flight(gpu_engine, lights, W, H):
    """four frames in a row from alternating cameras, an instance moved and the list replaced between them, each delivered by the device
    form at scales 1, 2, 3, 1 into its own buffer (every other one off a 16-byte boundary) with no host synchronisation: every buffer
    equals the same frame rendered and overlaid alone - its list as of its enqueue, its depth as of its frame: the test of the wait for
    the apply's reads of the depth plane (ev_ids) and of the list's staging"""
    scales = (1, 2, 3, 1)
    cams = ("side", "top", "side", "top")
    names = ("slopes", "many", "edges", "seams")
    h = hl._Host(gpu_engine, lights, W, H, capture=False)
    try:
        _styled(h, oc.STYLES["biased"])
        segs, alone, was = [], [], None
        for k, s in enumerate(scales):       # each frame alone, read back
            if k:
                rec = h.move(0, 0.3)
                was = rec if was is None else was
            h.frame(cams[k])
            pvm = _pvm(h.r)
            segs.append(oc.lists(pvm, W, H)[names[k]])
            alone.append(_statement(h, pvm, segs[k], h.ov_style, s))
        h.put(0, was)
        dests = []
        for k, s in enumerate(scales):       # the same four in flight
            if k:
                h.move(0, 0.3)
            h.r.overlay_set(segs[k])
            h.frame(cams[k])
            dests.append(_Dest(alone[k].shape[1], alone[k].shape[0], offset=4 * (k % 2)))
            h.r.copy_frame_overlaid_async(s, False, dests[-1].ptr())
        h.r.overlay_set(segs[0])             # a change behind the last delivery: it keeps the list it was enqueued with
        h.r.finish()
        for k, d in enumerate(dests):
            got = d.read()
            assert np.array_equal(got, alone[k]), "frame %d of four in flight differs from the same frame overlaid alone: %s" % (k, _first(got, alone[k]))
    finally:
        h.close()


def test_uniforms_set_after_the_frame_do_not_move_the_lines(gpu_engine, lights):
    W, H = 66, 34
    h = hl._Host(gpu_engine, lights, W, H, capture=False)
    try:
        h.frame("side")
        pvm = _pvm(h.r)
        seg = oc.lists(pvm, W, H)["slopes"]
        h.r.overlay_set(seg)
        want = _statement(h, pvm, seg, ovr.DEFAULT_STYLE)
        d, p, sp = lights
        h.r.update_uniforms(hc.camera("top"), d, p, sp, 0.3, 0.0, 0.0)            # another camera and a rolled stage, no frame
        assert not np.array_equal(_pvm(h.r), pvm)
        _both_forms(h, want, 1, False, 0, "camera moved behind the frame")
        _both_forms(h, fsr.downscale(want, 2), 2, False, 1, "camera moved behind the frame")
        h.r.render()                                                              # the next frame takes the new camera
        assert not np.array_equal(h.r.read_color_overlaid(1), want)
        assert np.array_equal(h.r.read_color_overlaid(1), _statement(h, _pvm(h.r), seg, ovr.DEFAULT_STYLE))
    finally:
        h.close()


def test_a_resting_context_keeps_resting(gpu_engine):
    """camera and scene stand still, the point lights move: from the third frame of the rest on every frame is delivered overlaid, the
    list changed between two of them; every delivery equals the statement, and zr_get_light_keep and zr_get_stats count exactly as on a
    twin context that never overlays"""
    W, H = 192, 128
    far = _lights(1, 16)
    for l in far[1]:
        l["Direction"][3] = 8.0              # point lights that reach far
    h, twin = hl._Host(gpu_engine, far, W, H), hl._Host(gpu_engine, far, W, H)
    try:
        lists, seg = None, None
        _styled(h, oc.STYLES["biased"])
        for i in range(7):
            for x in (h, twin):
                x.frame("side", roll_light=0.01 * i)
            if lists is None:
                pvm = _pvm(h.r)
                lists = oc.lists(pvm, W, H)
            if i in (2, 5):
                seg = lists["slopes" if i == 2 else "seams"]
                h.r.overlay_set(seg)
            if i >= 3:
                want = _statement(h, pvm, seg, h.ov_style)
                _both_forms(h, want, 1, False, i, "frame %d" % i)
            a, b = h.r.light_keep(), twin.r.light_keep()
            assert (a["read"], a["read_by_arg"], a["filled"], a["last"]) == (b["read"], b["read_by_arg"], b["filled"], b["last"]), (i, a, b)
            assert h.r.stats() == twin.r.stats()
            assert np.array_equal(h.r.color(), twin.r.color())
        k = h.r.light_keep()
        assert k["read"] >= 4 and k["read_by_arg"] >= 4, k                       # the one-launch lighting path is the one running
    finally:
        h.close(); twin.close()


# ------------------------------------------------------------------------------------------------ deltas

DELTA_CASES = [(66, 34, 1), (66, 34, 2), (257, 131, 1), (257, 131, 2)]


def _delta_on(h, scale, mode, overlay=True, highlight=False):
    h.r.set_frame_delta_overlay(overlay)
    h.delta_on(scale, mode, highlight=highlight)


@pytest.mark.parametrize("W,H,s", DELTA_CASES, ids=["%dx%d-s%d" % c for c in DELTA_CASES])
def test_deltas_carry_the_overlaid_frame_in_the_four_forms(gpu_engine, lights, W, H, s):
    """move, change one segment, rest, change the style, clear the list: after every step the client holds exactly
    zr_read_color_overlaid(delta scale); a step that changed nothing lists 0 tiles; a step that changed only the list or the style lists
    exactly the tiles in which the two overlaid frames differ"""
    h = hl._Host(gpu_engine, lights, W, H, capture=False)
    try:
        _delta_on(h, s, abi.FRAME_DELTA_PACKED)
        h.frame()
        pvm = _pvm(h.r)
        seg = oc.lists(pvm, W, H)["slopes"].copy()
        h.r.overlay_set(seg)
        _styled(h, oc.STYLES["default"])
        steps = ["first", "move", "segment", "rest", "style", "rest", "clear", "move"]
        prev, counts = None, []
        for f, what in enumerate(steps):
            if what == "move":
                h.move(0, 0.3)
            elif what == "segment":
                seg["rgba"][3] = (0, 255, 255, 255)                               # one segment's colour
                h.r.overlay_set(seg)
            elif what == "style":
                _styled(h, oc.STYLES["biased"])
            elif what == "clear":
                seg = seg[:0]
                h.r.overlay_set(None)
            h.frame()
            tiles, hd = h.deliver_form(f % 4)
            want = _statement(h, pvm, seg, h.ov_style, s)
            assert hd["serial"] == f + 1 and hd["full"] == (1 if f == 0 else 0)
            assert np.array_equal(h.client, want), "step %d (%s): the client copy differs from the overlaid frame: %s" % (f, what, _first(h.client, want))
            assert np.array_equal(h.r.read_color_overlaid(s), want)
            if f:
                assert np.array_equal(tiles, fdr.delta(prev, want)[0]), "step %d (%s) lists other tiles than the two overlaid frames differ in" % (f, what)
            prev = want
            counts.append(hd["n_tiles"])
        assert counts[0] == h.total and counts[3] == 0 and counts[5] == 0 and min(counts[1], counts[2], counts[4], counts[6], counts[7]) > 0, counts
    finally:
        h.close()


def test_deltas_with_the_highlight_underneath_and_with_the_switch_off(gpu_engine, lights):
    W, H = 66, 34
    h = hl._Host(gpu_engine, lights, W, H)
    try:
        _delta_on(h, 1, abi.FRAME_DELTA_PACKED, overlay=True, highlight=True)
        h.styled(hr.style("fill", 2))
        h.select(hc.SETS["odd_box"])
        h.frame()
        pvm = _pvm(h.r)
        seg = oc.lists(pvm, W, H)["seams"]
        h.r.overlay_set(seg)
        _styled(h, oc.STYLES["biased"])
        for f in range(4):
            if f >= 2:
                h.move(0, 0.3)
            h.frame()
            tiles, hd = h.deliver_form(f)
            want = _statement(h, pvm, seg, h.ov_style, 1, True)
            assert np.array_equal(h.client, want), "form %d: %s" % (f, _first(h.client, want))
            assert (f == 1) == (hd["n_tiles"] == 0), (f, hd)
        h.r.set_frame_delta(False)
        _delta_on(h, 1, abi.FRAME_DELTA_PACKED, overlay=False, highlight=False)
        h.client[:] = 0
        for f, what in enumerate(["first", "move", "list", "rest"]):
            if what == "move":
                h.move(0, 0.3)
            elif what == "list":
                h.r.overlay_set(seg[:5])
            h.frame()
            tiles, hd = h.deliver_form(f % 4)
            assert np.array_equal(h.client, h.r.color()), "step %d (%s)" % (f, what)
            assert f in (0, 1) or hd["n_tiles"] == 0, (f, hd)                    # the list moves nothing
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ zr_resize, refusals

def test_resize_with_a_list_set(gpu_engine, lights):
    """the list and the style survive zr_resize; later deliveries equal a fresh context's at the new extent"""
    h = hl._Host(gpu_engine, lights, 66, 34, capture=False)
    fresh = hl._Host(gpu_engine, lights, 257, 131, capture=False)
    try:
        h.frame("side")
        seg = oc.lists(_pvm(h.r), 66, 34)["guard"]
        h.r.overlay_set(seg)
        _styled(h, oc.STYLES["biased"])
        assert not np.array_equal(h.r.read_color_overlaid(1), h.r.color())
        h.r.resize(257, 131)
        h.W, h.H = 257, 131
        assert h.r.overlay_get().tobytes() == seg.tobytes() and h.r.overlay_style().hidden_opacity == 96
        with pytest.raises(gpu_engine.ZeldaRenderError) as e:
            h.r.read_color_overlaid(1)
        assert e.value.code == abi.ERR_STATE                                      # no frame at the new extent yet
        fresh.r.overlay_set(seg)
        _styled(fresh, oc.STYLES["biased"])
        for x in (h, fresh):
            x.frame("side")
        pvm = _pvm(h.r)
        want = _statement(h, pvm, seg, h.ov_style)
        assert not np.array_equal(want, h.r.color())
        for s in (1, 2):
            got = h.r.read_color_overlaid(s)
            assert np.array_equal(got, fresh.r.read_color_overlaid(s)) and np.array_equal(got, want if s == 1 else fsr.downscale(want, s))
        _both_forms(h, want, 1, False, 1, "resized")
    finally:
        h.close(); fresh.close()


def test_refusals_change_nothing(gpu_engine, lights):
    W, H = 66, 34
    E = gpu_engine.ZeldaRenderError
    L = gpu_engine.lib()

    def refused(code, call, *args):
        with pytest.raises(E) as e:
            call(*args)
        assert e.value.code == code, e.value

    h = hl._Host(gpu_engine, lights, W, H, capture=False)
    try:
        r = h.r
        dest = _Dest(W, H)
        out = np.full((H, W, 4), SENTINEL8, dtype=np.uint8)
        # before the first frame
        refused(abi.ERR_STATE, r.read_color_overlaid, 1)
        refused(abi.ERR_STATE, r.copy_frame_overlaid_async, 1, False, dest.ptr())
        h.frame()
        pvm = _pvm(r)
        seg = oc.lists(pvm, W, H)["slopes"]
        r.overlay_set(seg)
        _styled(h, oc.STYLES["biased"])
        a = r.read_color_overlaid(1)
        assert np.array_equal(a, _statement(h, pvm, seg, h.ov_style)) and not np.array_equal(a, r.color())
        # highlight != 0 asks for a captured frame; highlight == 0 does not
        refused(abi.ERR_STATE, r.read_color_overlaid, 1, True)
        refused(abi.ERR_STATE, r.copy_frame_overlaid_async, 1, True, dest.ptr())
        assert "without id capture" in str(pytest.raises(E, r.read_color_overlaid, 1, True).value)

        def unchanged():
            assert np.array_equal(r.read_color_overlaid(1), a) and r.overlay_get().tobytes() == seg.tobytes()
            st = r.overlay_style()
            assert (st.depth_bias, st.hidden_opacity) == (np.float32(1e-4), 96)
        # arguments
        for s in (0, 9):
            refused(abi.ERR_ARG, r.read_color_overlaid, s)
            refused(abi.ERR_ARG, r.copy_frame_overlaid_async, s, False, dest.ptr())
        refused(abi.ERR_ARG, r.copy_frame_overlaid_async, 1, False, None)
        refused(abi.ERR_ARG, r.copy_frame_overlaid_async, 1, False, dest.ptr() + 2)
        assert L.zr_read_color_overlaid(r.h, 1, 0, None, out.nbytes) == abi.ERR_ARG
        assert L.zr_read_color_overlaid(r.h, 1, 0, gpu_engine._ptr(out), out.nbytes - 4) == abi.ERR_ARG
        assert L.zr_read_color_overlaid(r.h, 2, 0, gpu_engine._ptr(out), out.nbytes) == abi.ERR_ARG
        bad = seg.copy()
        bad["flags"][3] = 2                                                      # an unknown flag bit
        refused(abi.ERR_ARG, r.overlay_set, bad)
        over = np.zeros(abi.OVERLAY_MAX_SEGMENTS + 1, dtype=abi.OVERLAY_SEGMENT)
        refused(abi.ERR_ARG, r.overlay_set, over)
        assert L.zr_overlay_set(r.h, None, 3) == abi.ERR_ARG
        import ctypes as C
        n = C.c_uint32(len(seg) - 1)
        small = np.zeros(len(seg), dtype=abi.OVERLAY_SEGMENT)
        assert L.zr_overlay_get(r.h, gpu_engine._ptr(small), C.byref(n)) == abi.ERR_ARG and n.value == len(seg) and not small.view(np.uint8).any()
        assert L.zr_overlay_get(r.h, gpu_engine._ptr(small), None) == abi.ERR_ARG
        for st in (abi.make_overlay_style(-1.0), abi.make_overlay_style(float("nan")), abi.make_overlay_style(0.0, 256), abi.OverlayStyle(0.0, 0, (C.c_uint32 * 2)(1, 0))):
            refused(abi.ERR_ARG, r.overlay_style, st)
        ok = abi.make_overlay_style()
        assert L.zr_set_overlay_style(r.h, None, 16) == abi.ERR_ARG
        assert L.zr_set_overlay_style(r.h, ok, 12) == abi.ERR_ARG and L.zr_get_overlay_style(r.h, ok, 20) == abi.ERR_ARG
        assert (out == SENTINEL8).all()
        unchanged()
        # between the stages of a frame
        d, p, sp = lights
        r.update_uniforms(hc.camera("side"), d, p, sp, 0.0, 0.0, 0.0)
        r.render_shadow()
        refused(abi.ERR_STATE, r.read_color_overlaid, 1)
        refused(abi.ERR_STATE, r.copy_frame_overlaid_async, 1, False, dest.ptr())
        r.render_gbuffer(); r.render_lighting()
        r.finish()
        assert (dest.read() == SENTINEL8).all(), "a refused call wrote into the destination"
        unchanged()
        # zr_set_frame_delta_overlay only while delta is off; kept across the switch
        r.set_frame_delta_overlay(True)
        r.set_frame_delta(True)
        refused(abi.ERR_STATE, r.set_frame_delta_overlay, False)
        h.Wd, h.Hd, h.total, h.scale = r.frame_delta_extent()
        h.client = np.zeros((H, W, 4), dtype=np.uint8)
        _, hd = h.deliver_form(0)
        assert hd["full"] == 1 and hd["serial"] == 1 and np.array_equal(h.client, a)
        r.set_frame_delta(False)
        r.set_frame_delta(True)
        h.client[:] = 0
        h.deliver_form(0)
        assert np.array_equal(h.client, a), "overlay delivery was not kept across zr_set_frame_delta(0)"
        r.set_frame_delta(False)
        r.set_frame_delta_overlay(False)
        unchanged()
        # the list is no instance set: it survives zr_object_add
        box = hc.scene().items[2]
        r.object_add(r.mesh_create(box["verts"], box["idx"]), None, None)
        assert r.overlay_get().tobytes() == seg.tobytes()
        h.frame()
        assert np.array_equal(r.read_color_overlaid(1), _statement(h, pvm, seg, h.ov_style))
        assert (dest.read() == SENTINEL8).all()
    finally:
        h.close()
    # a context whose lighting pass writes packed tiles
    p = gpu_engine.Renderer(W, H, 256, flags=abi.FLAG_PACKED_TILES)
    try:
        hc.scene().load(p)
        d, pl, sp = lights
        p.update_uniforms(hc.camera("side"), d, pl, sp, 0.0, 0.0, 0.0)
        p.render()
        p.overlay_set(seg)
        refused(abi.ERR_UNSUPPORTED, p.read_color_overlaid, 1)
        refused(abi.ERR_UNSUPPORTED, p.copy_frame_overlaid_async, 1, False, dest.ptr())
        refused(abi.ERR_ARG, p.read_color_overlaid, 0)                           # arguments first
        p.finish()
        assert (dest.read() == SENTINEL8).all()
    finally:
        p.close()
