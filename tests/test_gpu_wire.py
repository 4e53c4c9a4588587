"""The wireframe on the renderer (zr_set_wire_style, zr_read_color_staged, zr_copy_frame_staged_async, zr_set_frame_delta_wire).

The scene is exact in float32: Model = View = identity and Proj = (x, y, -1.5 z - 1.5, -z) (entries 1, -1, -1.5), so a non-instanced
corner's clip (x, y, w) is (x, y, -z) bit for bit whatever float32 it is, and an instanced one's is p s + t with s a power of two and
dyadic p, t - which the test asserts is exact.  numpy therefore has the kernel's corners, and every wired frame is held, BYTE FOR BYTE, to
engine.frame_wire (csrc/zr_wire.h on the host; tests/test_wire_cpu.py holds that to exact rationals) of zr_read_color's frame and
zr_read_ids' winners.  Frames: 96 x 64 (3 x 2 tiles) and 70 x 45 (ragged tiles on both axes)."""
import numpy as np
import pytest

import frame_delta_reference as fdr
from independent_scenes import _lights
from zeldaengine_amd import abi

pytestmark = pytest.mark.gpu

SIZES = ((96, 64), (70, 45))
WIDTHS = (1, 256, 1024, 4096)
RGBA = (250, 40, 10, 200)
NONE = 0xFFFFFFFF
SENTINEL8 = 0xA5


def _mesh(tris):
    """a mesh of free triangles, each in both windings (the camera pass culls one): triangle 2 k and 2 k + 1 are tris[k]"""
    tris = np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    both = np.concatenate([tris[:, None], tris[:, None, [0, 2, 1]]], axis=1).reshape(-1, 3)
    v = np.zeros(len(both), dtype=abi.XkVertex)
    v["Position"] = both; v["Normal"] = (0.0, 0.0, 1.0); v["Color"] = (1.0, 1.0, 1.0)
    return v, np.arange(len(both), dtype=np.uint32)


def _instances(rows):
    inst = np.zeros(len(rows), dtype=abi.XkInstanceData)
    for k, (t, s) in enumerate(rows):
        inst[k]["InstancePosition"] = t; inst[k]["InstancePScale"] = s
    return inst


INSTANCES = [((-0.75, 0.5, -2.25), 0.5), ((0.5, -0.25, -1.75), 1.0), ((1.0, 0.75, -2.0), 0.25)]
QUAD = [[(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.125)], [(-0.5, -0.5, 0.0), (0.5, 0.5, 0.125), (-0.5, 0.5, 0.0)]]


def _free_triangles(W, H):
    """the non-instanced draw: a large triangle across the tile borders, one with a corner behind the eye (the clip path), one smaller
    than a pixel around the centre of pixel (60 W / 96, 40 H / 64) at w = 1.5, in front of everything"""
    sx, sy, w = (60 * W) // 96 + 0.5, (40 * H) // 64 + 0.5, 1.5
    X, Y = (2.0 * sx / W - 1.0) * w, (2.0 * sy / H - 1.0) * w
    e = 0.25 * 2.0 * w / W                                   # a quarter of a pixel at that depth
    return [[(-1.5, -1.0, -2.0), (1.25, -0.75, -2.0), (0.0, 1.5, -2.5)],
            [(-1.75, -1.0, -2.5), (-0.5, -1.25, -2.0), (-1.0, 0.5, 0.5)],
            [(X - e, Y - e, -w), (X + e, Y - e, -w), (X, Y + e, -w)]]


class _Host:
    def __init__(self, engine, W, H, instances=None, free=None, quad_verts=None):
        """free: the free triangles (None: those of W x H); quad_verts: the quad mesh's vertices as a vertex update left them"""
        self.engine, self.W, self.H = engine, W, H
        self.free = _mesh(free if free is not None else _free_triangles(W, H))
        self.quad = _mesh(QUAD)
        if quad_verts is not None:
            self.quad = (quad_verts, self.quad[1])
        self.inst = _instances(instances if instances is not None else INSTANCES)
        self.r = r = engine.Renderer(W, H, 64)
        self.m_free, self.m_quad = r.mesh_create(*self.free), r.mesh_create(*self.quad)
        r.object_add(self.m_free, None, None)              # object 0: primitives 0 .. 5
        r.object_add(self.m_quad, None, self.inst)         # object 1: primitives 6 .. 6 + 4 n
        r.set_id_capture(True)
        d, p, sp = _lights(1, 2)
        r.update_uniforms(abi.make_camera(), d, p, sp, 0.0, 0.0, 0.0)
        cam, sh, view = r.get_frame()
        ident = np.eye(4, dtype=np.float32).reshape(16)
        P = np.zeros((4, 4), np.float32)
        P[0, 0] = 1.0; P[1, 1] = 1.0; P[2, 2] = -1.5; P[2, 3] = -1.5; P[3, 2] = -1.0
        for m in (cam, sh):
            m["Model"] = ident; m["View"] = ident
        cam["Proj"] = P.T.reshape(16)
        self.pvm = P.T.reshape(16).copy()
        r.set_frame(cam, sh, view)

    def close(self):
        self.r.close()

    def corners(self, inst=None, free=None, quad=None):
        """(x, y, w) of every primitive's corners, in primitive-id order; asserts that the instanced ones are exact in float32"""
        inst = self.inst if inst is None else inst
        fv, qv = (self.free[0] if free is None else free)["Position"], (self.quad[0] if quad is None else quad)["Position"]
        out = [fv.reshape(-1, 3, 3)]
        for i in inst:
            p32 = qv * np.float32(i["InstancePScale"]) + i["InstancePosition"].astype(np.float32)
            p64 = qv.astype(np.float64) * float(i["InstancePScale"]) + i["InstancePosition"].astype(np.float64)
            assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), p64), "the scene is not exact in float32"
            out.append(p32.reshape(-1, 3, 3))
        c = np.concatenate(out).astype(np.float32)
        c[..., 2] = -c[..., 2]                              # w = -z
        return c

    def selected(self, flags):
        """per primitive: the instanced draw's instances flagged in `flags`, object 0 not"""
        return np.concatenate([np.zeros(len(self.free[1]) // 3, np.uint8), np.repeat(np.asarray(flags, np.uint8), len(self.quad[1]) // 3)])

    def statement(self, style, selected=None, corners=None):
        return self.engine.frame_wire(self.r.color(), self.r.read_ids(), self.corners() if corners is None else corners, style, selected)


class _Dest:
    """a device buffer with guard bytes round the frame"""

    def __init__(self, Wd, Hd, offset=0):
        import torch
        self.n, self.offset, self.shape = Wd * Hd * 4, offset, (Hd, Wd, 4)
        self.buf = torch.full((offset + self.n + 64,), SENTINEL8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def ptr(self):
        return self.buf.data_ptr() + self.offset

    def read(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.offset] == SENTINEL8).all() and (b[self.offset + self.n:] == SENTINEL8).all(), "written outside the destination"
        return b[self.offset:self.offset + self.n].reshape(self.shape)


def _first(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return "%d pixels differ, first (x %d, y %d): %s, the statement %s" % (len(bad), bad[0][1], bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else "equal"


# ---- D: every byte equals the host statement

@pytest.mark.parametrize("forward", [False, True], ids=["deferred", "forward"])
@pytest.mark.parametrize("W,H", SIZES)
def test_wire_equals_the_host_statement_in_every_byte(gpu_engine, W, H, forward):
    h = _Host(gpu_engine, W, H)
    try:
        r = h.r
        if forward:
            r.set_shading(True)
        r.render()
        prim, plain, corners = r.read_ids(), r.color(), h.corners()
        # what the scene must show: both draws, every instance, the clip-path triangle, the sub-pixel one, empty pixels, a tile border
        seen = set(np.unique(prim).tolist())
        assert NONE in seen and seen & {0, 1} and seen & {2, 3} and seen & {4, 5}, seen
        for i in range(3):
            assert seen & set(range(6 + 4 * i, 10 + 4 * i)), (i, seen)
        big = np.isin(prim, (0, 1))
        assert big[:, 31].any() and big[:, 32].any() and big[31].any() and big[32].any()
        assert 1 <= np.isin(prim, (4, 5)).sum() <= 2
        flags = [1, 0, 1]
        r.highlight_set(1, flags)
        for width in WIDTHS:
            for sel in (False, True):
                st = abi.make_wire_style(RGBA, width, abi.WIRE_SELECTED if sel else 0)
                r.set_wire_style(st)
                got = r.read_color_staged(abi.STAGE_WIRE)
                want = gpu_engine.frame_wire(plain, prim, corners, st, h.selected(flags) if sel else None)
                assert np.array_equal(got, want), "width %d selected %s: %s" % (width, sel, _first(got, want))
                on = (want != plain).any(axis=2)
                assert (on.any() or width == 1) and not on[prim == NONE].any() and (not sel or not on[prim < 6].any())
                if width == 256:
                    assert not on.all() and (sel or on[np.isin(prim, (2, 3))].any())
        r.highlight_clear()                                  # an empty set: no wire anywhere
        assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE), plain)
        assert np.array_equal(r.color(), plain), "the frame itself was drawn into"
    finally:
        h.close()


# ---- F: the path

def test_staged_deliveries_are_the_existing_ones_and_the_statements_in_order(gpu_engine):
    W, H = SIZES[1]
    h = _Host(gpu_engine, W, H)
    try:
        r = h.r
        r.render()
        r.highlight_set(1, [0, 1, 0])
        r.set_highlight_style(outline=(0, 255, 0, 255), fill=(0, 0, 255, 90), radius=2)
        seg = [(-1.0, -1.0, -2.0, 1.0, 1.0, -1.5, 255, 255, 0, 255), (-1.5, 0.5, -2.5, 1.5, 0.25, -1.25, 0, 255, 255, 160, abi.OVERLAY_XRAY)]
        r.overlay_set(seg)
        st = abi.make_wire_style(RGBA, 384)
        r.set_wire_style(st)
        plain, prim, depth, obj = r.color(), r.read_ids(), r.gbuffer(0), r.read_ids(abi.IDS_OBJECT)
        mask = (obj[..., 0] == 1) & (obj[..., 1] == 1)
        assert mask.any()
        wired = gpu_engine.frame_wire(plain, prim, h.corners(), st)
        marked = gpu_engine.frame_highlight(wired, mask, r.highlight_style())
        lined = gpu_engine.frame_overlay(marked, depth, h.pvm, seg, r.overlay_style())
        assert (wired != plain).any() and (marked != wired).any() and (lined != marked).any()
        ALL = abi.STAGE_WIRE | abi.STAGE_HIGHLIGHT | abi.STAGE_OVERLAY
        for s in (1, 2, 3):
            assert np.array_equal(r.read_color_staged(0, s), r.color_scaled(s))
            assert np.array_equal(r.read_color_staged(abi.STAGE_HIGHLIGHT, s), r.color_highlighted(s))
            assert np.array_equal(r.read_color_staged(abi.STAGE_OVERLAY, s), r.read_color_overlaid(s, False))
            assert np.array_equal(r.read_color_staged(abi.STAGE_HIGHLIGHT | abi.STAGE_OVERLAY, s), r.read_color_overlaid(s, True))
            want = gpu_engine.frame_downscale(lined, s)
            got = r.read_color_staged(ALL, s)
            assert np.array_equal(got, want), "all stages, scale %d: %s" % (s, _first(got, want))
            for k, stages in enumerate((0, abi.STAGE_WIRE, abi.STAGE_WIRE | abi.STAGE_HIGHLIGHT, abi.STAGE_WIRE | abi.STAGE_OVERLAY, ALL)):
                d = _Dest(want.shape[1], want.shape[0], offset=4 * ((k + s) % 2))
                r.copy_frame_staged_async(stages, s, d.ptr())
                r.finish()
                assert np.array_equal(d.read(), r.read_color_staged(stages, s)), "device form, stages %d scale %d" % (stages, s)
        assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE | abi.STAGE_HIGHLIGHT), marked)
        assert np.array_equal(r.color(), plain)
    finally:
        h.close()


def test_deliveries_of_changes_carry_the_wire(gpu_engine):
    W, H = SIZES[0]
    h = _Host(gpu_engine, W, H)
    try:
        r = h.r
        r.set_wire_style(rgba=RGBA, width_256=256)
        r.set_frame_delta_wire(True)
        r.set_frame_delta(True)
        with pytest.raises(gpu_engine.ZeldaRenderError) as e:
            r.set_frame_delta_wire(False)
        assert e.value.code == abi.ERR_STATE
        r.render()
        client = np.zeros((H, W, 4), dtype=np.uint8)
        t, px, hd = r.read_frame_delta()
        assert hd["full"] == 1 and len(t) == 6
        fdr.apply(client, t, px)
        first = r.read_color_staged(abi.STAGE_WIRE)
        assert np.array_equal(client, first) and (first != r.color()).any()
        t, px, hd = r.read_frame_delta()                     # at rest, the style unchanged: nothing
        assert hd["n_tiles"] == 0
        r.set_wire_style(rgba=RGBA, width_256=1024)          # a style change between two deliveries of a resting frame
        second = r.read_color_staged(abi.STAGE_WIRE)
        t, px, hd = r.read_frame_delta()
        want_t, want_px = fdr.delta(first, second)
        assert 0 < len(want_t) and np.array_equal(t, want_t) and np.array_equal(px, want_px)
        fdr.apply(client, t, px)
        assert np.array_equal(client, second)
    finally:
        h.close()


# ---- G: it follows the scene

MOVED = [((-0.5, 0.25, -2.25), 0.5), ((0.25, -0.5, -1.75), 1.0), ((1.0, 0.5, -2.0), 0.5)]


def _dev(a):
    """a numpy record array as a device tensor of its bytes (what the device forms of the updates take)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _squeezed(quad_verts):
    v = quad_verts.copy()
    v["Position"][:, 0] *= np.float32(0.5)                 # dyadic: the vertex stage stays exact
    return v


def _fresh_wire(engine, W, H, st, instances=None, quad_verts=None, hidden=None, free=None):
    """(winner plane, staged(WIRE)) of a context built from the data itself at W x H"""
    f = _Host(engine, W, H, instances=instances, free=free, quad_verts=quad_verts)
    try:
        if hidden is not None:
            f.r.object_set_instance_visibility(1, hidden)
        f.r.set_wire_style(st)
        f.r.render()
        return f.r.read_ids(), f.r.read_color_staged(abi.STAGE_WIRE)
    finally:
        f.close()


@pytest.mark.parametrize("device_form", [False, True], ids=["host_forms", "device_forms"])
def test_wire_follows_instances_vertices_visibility_rest_and_resize(gpu_engine, device_form):
    """After zr_object_set_instances / zr_mesh_set_vertices or their device forms (zr_object_update_instances_async,
    zr_mesh_update_vertices_async: the mesh sets and instance planes of the frame's parity, rewritten at the frame's head) the next
    frame's wire is the host statement of the new data AND the delivery of a context built from the new data, byte for byte."""
    W, H = SIZES[0]
    h = _Host(gpu_engine, W, H)
    st = abi.make_wire_style(RGBA, 512)
    keep = []
    try:
        r = h.r
        r.set_wire_style(st)
        r.render()
        before = r.read_color_staged(abi.STAGE_WIRE)
        assert np.array_equal(before, h.statement(st))
        # 5th frame of a rest equals the 1st
        for _ in range(4):
            r.render()
        assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE), before)
        # instances moved: the next frame's wire is the new data's
        moved = _instances(MOVED)
        if device_form:
            keep.append(_dev(moved))
            r.object_update_instances_async(1, keep[-1])
        else:
            r.object_set_instances(1, moved)
        assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE), before), "an update took effect before the next frame"
        r.render()
        got, want = r.read_color_staged(abi.STAGE_WIRE), h.statement(st, corners=h.corners(inst=moved))
        assert np.array_equal(got, want) and (got != before).any(), _first(got, want)
        f_prim, f_wire = _fresh_wire(gpu_engine, W, H, st, instances=MOVED)
        assert np.array_equal(f_prim, r.read_ids()) and np.array_equal(f_wire, got), _first(f_wire, got)
        # vertices moved
        quad2 = _squeezed(h.quad[0])
        if device_form:
            keep.append(_dev(quad2))
            r.mesh_update_vertices_async(h.m_quad, keep[-1])
        else:
            r.mesh_set_vertices(h.m_quad, quad2)
        assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE), got), "an update took effect before the next frame"
        r.render()
        got2, want = r.read_color_staged(abi.STAGE_WIRE), h.statement(st, corners=h.corners(inst=moved, quad=quad2))
        assert np.array_equal(got2, want) and (got2 != got).any(), _first(got2, want)
        f_prim, f_wire = _fresh_wire(gpu_engine, W, H, st, instances=MOVED, quad_verts=quad2)
        assert np.array_equal(f_prim, r.read_ids()) and np.array_equal(f_wire, got2), _first(f_wire, got2)
        for _ in range(3):                                   # and on the frames after it, both parities and a rest
            r.render()
            assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE), got2)
        # hidden instances draw none
        r.object_set_instance_visibility(1, [1, 0, 1])
        r.render()
        prim = r.read_ids()
        assert not np.isin(prim, range(10, 14)).any()
        got3, want = r.read_color_staged(abi.STAGE_WIRE), h.statement(st, corners=h.corners(inst=moved, quad=quad2))
        assert np.array_equal(got3, want), _first(got3, want)
        f_prim, f_wire = _fresh_wire(gpu_engine, W, H, st, instances=MOVED, quad_verts=quad2, hidden=[1, 0, 1])
        assert np.array_equal(f_prim, prim) and np.array_equal(f_wire, got3), _first(f_wire, got3)
        # a new extent: the wire is that of a context made at the new extent
        r.resize(70, 45)
        with pytest.raises(gpu_engine.ZeldaRenderError):
            r.read_color_staged(abi.STAGE_WIRE)
        r.render()
        got4, want = r.read_color_staged(abi.STAGE_WIRE), h.statement(st, corners=h.corners(inst=moved, quad=quad2))
        assert got4.shape == (45, 70, 4) and np.array_equal(got4, want) and (got4 != r.color()).any(), _first(got4, want)
        # (the resized context keeps the free triangles it was made with at 96 x 64: the fresh one takes the same mesh)
        f_prim, f_wire = _fresh_wire(gpu_engine, 70, 45, st, instances=MOVED, quad_verts=quad2, hidden=[1, 0, 1], free=_free_triangles(W, H))
        assert np.array_equal(f_prim, r.read_ids()), "the winner planes of the resized and the fresh context differ"
        assert np.array_equal(f_wire, got4), _first(f_wire, got4)
        assert r.wire_style().width_256 == 512              # kept across the resize
    finally:
        h.close()


@pytest.mark.parametrize("device_form", [False, True], ids=["host_forms", "device_forms"])
def test_a_delivery_in_flight_keeps_its_frames_wire(gpu_engine, device_form):
    """copy_frame_staged_async after frame N, then an instance and a vertex update and frames N + 1, N + 2: the delivery is frame N's
    wire (the frame after next waits before it rewrites what the launch reads)"""
    W, H = SIZES[0]
    h = _Host(gpu_engine, W, H)
    st = abi.make_wire_style(RGBA, 512)
    keep = []
    try:
        r = h.r
        r.set_wire_style(st)
        r.render()
        want = h.statement(st)
        r.render()                                           # frame N: the same scene, nothing read back in between
        d = _Dest(W, H)
        r.copy_frame_staged_async(abi.STAGE_WIRE, 1, d.ptr())
        moved, quad2 = _instances(MOVED), _squeezed(h.quad[0])
        if device_form:
            keep += [_dev(moved), _dev(quad2)]
            r.object_update_instances_async(1, keep[0])
            r.mesh_update_vertices_async(h.m_quad, keep[1])
        else:
            r.object_set_instances(1, moved)
            r.mesh_set_vertices(h.m_quad, quad2)
        r.render()
        d1 = _Dest(W, H)
        r.copy_frame_staged_async(abi.STAGE_WIRE, 1, d1.ptr())      # frame N + 1's, in flight behind frame N + 2
        r.render()
        r.finish()
        assert np.array_equal(d.read(), want), _first(d.read(), want)
        got, now = r.read_color_staged(abi.STAGE_WIRE), h.statement(st, corners=h.corners(inst=moved, quad=quad2))
        assert np.array_equal(got, now) and (now != want).any(), _first(got, now)
        assert np.array_equal(d1.read(), now), _first(d1.read(), now)
    finally:
        h.close()


# ---- H: refusals leave the context as it was

def test_refusals_leave_the_context_as_it_was(gpu_engine):
    W, H = SIZES[1]
    E = gpu_engine.ZeldaRenderError
    h = _Host(gpu_engine, W, H)
    try:
        r, L = h.r, gpu_engine.lib()
        dest = _Dest(W, H)
        out = np.zeros((H, W, 4), dtype=np.uint8)

        def refused(code, fn, *a):
            with pytest.raises(E) as e:
                fn(*a)
            assert e.value.code == code, (fn.__name__, a, e.value)
        # the style
        keep = abi.make_wire_style(RGBA, 640, abi.WIRE_SELECTED)
        r.set_wire_style(keep)
        for bad in (dict(width_256=0), dict(width_256=4097), dict(flags=2)):
            refused(abi.ERR_ARG, r.set_wire_style, abi.make_wire_style(**bad))
        st = abi.make_wire_style(); st.reserved = 7
        refused(abi.ERR_ARG, r.set_wire_style, st)
        assert L.zr_set_wire_style(r.h, keep, 12) == abi.ERR_ARG and L.zr_get_wire_style(r.h, keep, 20) == abi.ERR_ARG
        got = r.wire_style()
        assert (list(got.rgba), got.width_256, got.flags, got.reserved) == (list(RGBA), 640, abi.WIRE_SELECTED, 0)
        r.set_wire_style(rgba=RGBA, width_256=256)
        # before the first frame: arguments first, then the state
        refused(abi.ERR_ARG, r.read_color_staged, 8)
        refused(abi.ERR_ARG, r.read_color_staged, abi.STAGE_WIRE, 0)
        refused(abi.ERR_STATE, r.read_color_staged, abi.STAGE_WIRE)
        refused(abi.ERR_STATE, r.read_color_staged, 0)
        refused(abi.ERR_STATE, r.copy_frame_staged_async, abi.STAGE_WIRE, 1, dest.ptr())
        # the last frame rendered without capture: the wire is refused as the highlight is, the plain stages are not
        r.set_id_capture(False)
        r.render()
        refused(abi.ERR_STATE, r.read_color_staged, abi.STAGE_WIRE)
        refused(abi.ERR_STATE, r.copy_frame_staged_async, abi.STAGE_WIRE | abi.STAGE_OVERLAY, 2, dest.ptr())
        assert "without id capture" in str(pytest.raises(E, r.read_color_staged, abi.STAGE_WIRE).value)
        assert np.array_equal(r.read_color_staged(0), r.color())
        r.set_id_capture(True)
        r.render()
        want = r.read_color_staged(abi.STAGE_WIRE)
        # arguments
        for stages in (8, 16, 0x80000001):
            refused(abi.ERR_ARG, r.read_color_staged, stages)
            refused(abi.ERR_ARG, r.copy_frame_staged_async, stages, 1, dest.ptr())
        for s in (0, 9):
            refused(abi.ERR_ARG, r.read_color_staged, abi.STAGE_WIRE, s)
            refused(abi.ERR_ARG, r.copy_frame_staged_async, abi.STAGE_WIRE, s, dest.ptr())
        refused(abi.ERR_ARG, r.copy_frame_staged_async, abi.STAGE_WIRE, 1, None)
        refused(abi.ERR_ARG, r.copy_frame_staged_async, abi.STAGE_WIRE, 1, dest.ptr() + 2)
        assert L.zr_read_color_staged(r.h, 1, 1, None, out.nbytes) == abi.ERR_ARG
        assert L.zr_read_color_staged(r.h, 1, 1, gpu_engine._ptr(out), out.nbytes - 4) == abi.ERR_ARG
        assert L.zr_read_color_staged(r.h, 1, 2, gpu_engine._ptr(out), out.nbytes) == abi.ERR_ARG
        assert L.zr_read_color_staged(None, 1, 1, gpu_engine._ptr(out), out.nbytes) == abi.ERR_ARG
        # between the stages of a frame
        r.render_shadow()
        refused(abi.ERR_STATE, r.read_color_staged, abi.STAGE_WIRE)
        refused(abi.ERR_STATE, r.copy_frame_staged_async, abi.STAGE_WIRE, 1, dest.ptr())
        r.render_gbuffer(); r.render_lighting()
        r.finish()
        assert (dest.read() == SENTINEL8).all(), "a refused call wrote into the destination"
        assert np.array_equal(r.read_color_staged(abi.STAGE_WIRE), want)
        # the scene changed since the last frame
        r.object_add(h.m_free, None, None)
        refused(abi.ERR_STATE, r.read_color_staged, abi.STAGE_WIRE)
        assert "the scene changed" in str(pytest.raises(E, r.read_color_staged, abi.STAGE_WIRE).value)
        r.render()
        r.read_color_staged(abi.STAGE_WIRE)
    finally:
        h.close()
    # a context whose lighting pass writes packed tiles: arguments first, then unsupported
    p = gpu_engine.Renderer(W, H, 64, flags=abi.FLAG_PACKED_TILES)
    try:
        p.object_add(p.mesh_create(*_mesh(_free_triangles(W, H))), None, None)
        p.set_id_capture(True)
        d, pl, sp = _lights(1, 2)
        p.update_uniforms(abi.make_camera(), d, pl, sp, 0.0, 0.0, 0.0)
        p.render()
        with pytest.raises(E) as e:
            p.read_color_staged(abi.STAGE_WIRE)
        assert e.value.code == abi.ERR_UNSUPPORTED
        with pytest.raises(E) as e:
            p.read_color_staged(8)
        assert e.value.code == abi.ERR_ARG
    finally:
        p.close()


# ---- I: the native driver

def test_headless_wire_writes_what_the_renderer_delivers(gpu_engine, tmp_path):
    """tools/zelda_headless --wire=384: the written image is the one Renderer.read_color_staged returns, plain and with
    --pick .. --highlight --wire-selected through --delta --scale 2"""
    import json
    import os
    import subprocess
    from test_gpu_native_host import H, SD, W, _content_tree
    from zeldaengine_amd import build as zbuild
    root = str(tmp_path)
    _content_tree(root)
    exe = zbuild.build_headless()
    rect = (W // 4, H // 4, W // 2, H // 2)
    modes = {"plain": ["--wire=384"], "selected2": ["--wire=384", "--wire-selected", "--pick", "%d,%d,%d,%d" % rect, "--highlight", "--delta", "--scale", "2"]}
    images, printed = {}, {}
    for mode, extra in modes.items():
        ppm = os.path.join(root, mode + ".ppm")
        out = subprocess.run([exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (W, H), "--shadow", str(SD), "--frames", "2", "--out", ppm] + extra,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text
        printed[mode] = [json.loads(l) for l in text.splitlines() if l.startswith("{")]
        images[mode] = open(ppm, "rb").read()
        assert mode != "plain" or text.count("wired %dx%d" % (W, H)) == 2
    g = gpu_engine.Renderer(W, H, SD)
    try:
        g.set_asset_root(root)
        g.world_load_file("Content/World.json")
        g.set_id_capture(True)
        for f in range(2):
            g.world_update_uniforms(0.0, 0.0, 0.016 * f)
            g.render()
            if f == 0:
                hits, n = g.pick(*rect)
        g.set_wire_style(width_256=384)
        want = g.read_color_staged(abi.STAGE_WIRE)
        assert images["plain"] == ("P6\n%d %d\n255\n" % (W, H)).encode() + want[..., :3].tobytes()
        assert (want != g.color()).any()
        assert printed["selected2"] and [(p["object"], p["instance"]) for p in printed["selected2"]] == [(int(x["object"]), int(x["instance"])) for x in hits]
        for x in hits:
            g.highlight_set(int(x["object"]), 1, first=int(x["instance"]))
        g.set_wire_style(width_256=384, flags=abi.WIRE_SELECTED)
        want = g.read_color_staged(abi.STAGE_WIRE | abi.STAGE_HIGHLIGHT, 2)
        assert images["selected2"] == ("P6\n%d %d\n255\n" % (want.shape[1], want.shape[0])).encode() + want[..., :3].tobytes()
    finally:
        g.close()


# ---- E: perspective scenes against the independent statement

def _independent_verdicts(case, prim, width_256):
    """Per pixel of the winner plane: on the wire (1), off (0) or undecided (2) by the float64 statement over
    independent_geometry._triangles' corners, and `near`: within r + 1 pixels of an edge line of its winner.  A pixel is undecided
    when its distance to some edge line of its winner is within the propagated corner error + 2^-20 of r: the corner error is the
    statement's own float32 bound (K_EYE through |Proj|, plus K_PROJ), carried to the distance to first order - the change of the distance
    under each of the edge's six corner components moved by its bound, summed."""
    import independent_geometry as ig
    W, H = case.W, case.H
    fu = ig.frame_uniforms(case.cam, case.lights[0], case.lights[1], W, H, case.roll_stage, case.roll_light)
    ubo = fu["cam"]
    clip, e_eye, e_proj, ids = ig._triangles(case.scene.draws(), ubo)
    err = np.einsum("ij,tkj->tki", np.abs(ubo["Proj"])[:, :3], e_eye) + e_proj           # (T, 3, 4): per clip coordinate
    assert np.array_equal(ids, np.arange(len(ids)))
    r = width_256 / 512.0
    ys, xs = np.nonzero(prim < len(ids))
    t = prim[ys, xs].astype(np.int64)
    px, py = xs + 0.5, ys + 0.5
    c, e = clip[t][:, :, [0, 1, 3]], err[t][:, :, [0, 1, 3]]                             # (N, 3 corners, x y w)

    def dist(ca, cb):
        ha = np.stack([0.5 * W * (ca[:, 0] + ca[:, 2]), 0.5 * H * (ca[:, 1] + ca[:, 2]), ca[:, 2]], axis=1)
        hb = np.stack([0.5 * W * (cb[:, 0] + cb[:, 2]), 0.5 * H * (cb[:, 1] + cb[:, 2]), cb[:, 2]], axis=1)
        l = np.cross(ha, hb)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.abs(l[:, 0] * px + l[:, 1] * py + l[:, 2]) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)
    on = np.zeros(len(t), dtype=bool); unsure = np.zeros(len(t), dtype=bool); near = np.zeros(len(t), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        d0 = dist(c[:, a], c[:, b])
        tol = np.zeros(len(t))
        for which in (a, b):
            for comp in range(3):
                moved = c.copy()
                moved[:, which, comp] += e[:, which, comp]
                da, db = (moved[:, a], c[:, b]) if which == a else (c[:, a], moved[:, b])
                tol += np.abs(dist(da, db) - d0)
        tol = tol + 2.0 ** -20
        ok = np.isfinite(d0) & np.isfinite(tol)
        unsure |= ~ok | (np.abs(d0 - r) <= tol)
        on |= ok & (d0 < r - tol)
        near |= ok & (d0 <= r + 1.0)
    verdict = np.full(prim.shape, 0, dtype=np.uint8)
    verdict[ys, xs] = np.where(on, 1, np.where(unsure, 2, 0))
    near_plane = np.zeros(prim.shape, dtype=bool)
    near_plane[ys, xs] = near
    return verdict, near_plane


def _hold_to_the_independent_statement(case, prim, plain, got, width_256, rgba):
    import wire_reference as wr
    verdict, near = _independent_verdicts(case, prim, width_256)
    undecided, n_near = int((verdict == 2).sum()), int(near.sum())
    print("width %d: near %d, undecided %d, on %d, off-but-near %d" % (width_256, n_near, undecided, int((verdict == 1).sum()), int(((verdict == 0) & near).sum())))
    assert n_near > 200 and undecided <= 0.02 * n_near, (undecided, n_near)               # the reference's side alone
    assert (verdict == 1).sum() > 50 and ((verdict == 0) & near).sum() > 50                # both verdicts, and not trivially
    want_on = np.array([wr.blend_pixel(p, rgba) for p in plain.reshape(-1, 4)], dtype=np.uint8).reshape(plain.shape)
    bad_on = (verdict == 1) & (got != want_on).any(axis=2)
    bad_off = (verdict == 0) & (got != plain).any(axis=2)
    assert not bad_on.any() and not bad_off.any(), (np.argwhere(bad_on)[:4].tolist(), np.argwhere(bad_off)[:4].tolist())
    und = verdict == 2                                       # an undecided pixel is still one of the two
    assert ((got[und] == plain[und]).all(axis=1) | (got[und] == want_on[und]).all(axis=1)).all()


@pytest.mark.parametrize("name", ["mixed", "rolled_and_clipped", "low_camera"])
def test_perspective_scenes_against_the_independent_statement(gpu_engine, name):
    """The scenes of tests/independent_scenes.py under their perspective cameras: the winner plane as read back, corners and their
    float32 error bounds from independent_geometry._triangles; every pixel the statement decides is wire or not as it says"""
    import independent_scenes as isc
    case = isc.case(name)
    r = gpu_engine.Renderer(case.W, case.H, case.SD)
    try:
        case.scene.load(r)
        r.set_id_capture(True)
        d, p, sp = case.lights
        r.update_uniforms(case.cam, d, p, sp, case.roll_stage, case.roll_light, 0.0)
        r.render()
        prim, plain = r.read_ids(), r.color()
        for width in (256, 1024):
            r.set_wire_style(rgba=RGBA, width_256=width)
            _hold_to_the_independent_statement(case, prim, plain, r.read_color_staged(abi.STAGE_WIRE), width, RGBA)
    finally:
        r.close()
