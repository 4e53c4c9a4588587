"""A resting frame leaves the parts no point light reaches as they stand (csrc/zr_lighting.hip: k_lighting_stand; csrc/zr_settle.h;
csrc/zr_lighting_host.cpp).

On a resting frame only the point lights move, so a part (32 x 16 pixels, half a tile: a workgroup of the one launch) whose world-space
box lies outside every light's radius gets the colour the launch before wrote to the same addresses.  Once a launch of the current
generation has written it, the part returns after its set-up.  The observable is zr_get_rest_settled: how many parts stand settled after
the frame enqueued last.  Whatever is left alone must be what would have been computed: every frame of every case is compared byte for
byte with a ZR_FLAG_NO_LIST_REUSE twin, which keeps nothing and shades every pixel of every frame.  No tolerances.

The count is also predicted (numpy, float32): per part the box of the world positions of its pixels with Mask != 0, read back from the
GPU's own GBuffer (zr_read_gbuffer, target 5; bit-equal to the oracle's) - widened to the origin where the part holds an empty pixel -
tested against every point light of the frame as light_listed (csrc/zr_shade.h) tests it.  A part with a light within 1e-4 (relative,
squared distance against squared radius) of the boundary is left out as undecided; at most 5 % of the parts may be.  What is held to
the prediction is the SET (zr_get_rest_settled_parts: a byte per part): every decided part stands exactly where the prediction says, on
every frame at least two past the last change of generation - over sweeps in which the count rises and falls.

Scenes and helpers are those of test_gpu_rest_one_launch.py (the pile from a camera of the test's choosing), with point lights of a
small radius, which leave most of the frame alone.
"""
import re

import numpy as np
import pytest

from test_gpu_lighting_keep import _last, _pair
from test_gpu_rest_one_launch import CAP, RStage, _by_arg, _empty, _first_empty_per_workgroup, _last_wave_camera, _pairs
from test_gpu_round2_keep import BOX, SPHERES, _lights
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

RADIUS, RATE = 0.8, 0.1      # of the sweeps' point lights: chosen with the oracle's GBuffer D so that the settled count rises and falls
EXTENTS = [(160, 120), (33, 17), (100, 72)]


class SStage(RStage):
    """RStage with point lights of a small radius that roll fast."""

    def __init__(self, n_point=16, size=(160, 120), cam=None, zfar=45.0, radius=RADIUS, rate=RATE):
        super().__init__(n_point, size, cam, zfar)
        d, p, s = _lights(n_point)
        p["Direction"][:, 3] = radius
        self.lights = d, p, s
        self.roll_rate = rate


def predict(g, W, H):
    """-> per part (tile-major, the tile's upper half first: the launch's workgroups) 1 surely settled, 0 surely reached, 2 undecided,
    for the frame g holds: its GBuffer and its uniforms"""
    _, _, view = g.get_frame()
    n = int(view["LightsCount"][1])
    lp = np.array([view["PointLights"][k]["Position"][:3] for k in range(n)], dtype=np.float32).reshape(n, 3)
    rad = np.array([view["PointLights"][k]["Direction"][3] for k in range(n)], dtype=np.float32)
    col = np.array([view["PointLights"][k]["Color"] for k in range(n)], dtype=np.float32).reshape(n, 4)
    always = ~(np.isfinite(col).all(axis=1) & (rad > 0)) if n else np.zeros(0, dtype=bool)      # light_listed keeps such a light
    d = g.gbuffer(5)
    pos = np.stack([((d >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float32) for k in range(3)], axis=-1)
    mask = (g.gbuffer(1) >> 24) != 0
    empty = _empty(g)
    state = []
    with np.errstate(invalid="ignore", over="ignore"):
        for ty in range(0, H, 32):
            for tx in range(0, W, 32):
                for half in (0, 16):
                    sl = (slice(ty + half, min(ty + half + 16, H)), slice(tx, min(tx + 32, W)))
                    q = pos[sl][mask[sl]]
                    lo = np.full(3, np.inf, dtype=np.float32); hi = np.full(3, -np.inf, dtype=np.float32)
                    if len(q):
                        lo, hi = (q.min(axis=0), q.max(axis=0)) if np.isfinite(q).all() else (np.full(3, -np.inf, dtype=np.float32), np.full(3, np.inf, dtype=np.float32))
                    if empty[sl].any():
                        lo, hi = np.minimum(lo, np.float32(0)), np.maximum(hi, np.float32(0))
                    reached = near = False
                    for k in range(n):
                        if always[k]:
                            reached = True
                            continue
                        e = np.maximum(np.float32(0), np.maximum(lo - lp[k], lp[k] - hi)).astype(np.float32)
                        d2 = np.float32(e[2] * e[2] + np.float32(e[1] * e[1] + np.float32(e[0] * e[0])))
                        thr = np.float32(np.float32(rad[k] * rad[k]) * np.float32(1.000001))
                        if abs(float(d2) - float(thr)) <= 1e-4 * float(thr):
                            near = True
                        elif not d2 > thr:
                            reached = True
                    state.append(0 if reached else 2 if near else 1)
    return np.array(state, dtype=np.uint8)


def _held(g, st, what):
    """the parts that stand after g's last frame against the prediction, part by part -> (parts, settled, which)"""
    parts, settled = g.rest_settled()
    which = g.rest_settled_parts()
    want = predict(g, st.W, st.H)
    decided = want != 2
    print(what, "parts", parts, "settled", settled, "predicted", int((want == 1).sum()), "+", int((~decided).sum()))
    assert parts == len(want) == len(which) and settled == int(which.sum()) and (~decided).sum() <= 0.05 * parts, (what, parts, len(want))
    assert np.array_equal(which[decided], want[decided]), (what, np.flatnonzero(decided & (which != want)).tolist())
    return parts, settled, which


def _rest(g, twin, st, n=4, i0=0, what="start"):
    """frames i0 .. i0 + n - 1 on both, compared -> what g did on the last"""
    last = None
    for i in range(i0, i0 + n):
        last = _pair(g, twin, st, i, what)
    return last


# ------------------------------------------------------------------------------------------------ 1. a sweep, 2. the prediction

# radius and roll rate of the sweep per extent, chosen with the oracle's GBuffer D (bit-equal to the GPU's) so that the count moves
SWEEP = {(160, 120): (0.8, 0.1), (100, 72): (2.5, 0.5), (33, 17): (3.0, 0.7)}


@pytest.mark.parametrize("size", EXTENTS)
def test_sweep_settles_rises_and_falls_as_predicted(gpu_engine, size):
    """Lights roll through the pile for 21 frames.  Frames 0 and 1 draw, 2 fills, 3 is the first launch of a generation: from frame 4
    on the parts that stand are the prediction's, part by part.  At every extent the count rises, falls and rises again, and lies
    strictly between none and all on at least three frames: asserted, not assumed."""
    st = SStage(16, size=size, radius=SWEEP[size][0], rate=SWEEP[size][1])
    g, twin = _pairs(st, gpu_engine)
    counts = []
    for i in range(21):
        did = _pair(g, twin, st, i, "sweep %dx%d" % size)
        if i >= 4:
            assert did == "read"
            parts, settled, which = _held(g, st, "frame %d" % i)
            counts.append(settled)
    print(size, counts)
    assert _by_arg(g) == 18 and twin.rest_settled()[1] == 0 and not twin.rest_settled_parts().any()
    assert sum(0 < c < parts for c in counts) >= 3, counts
    s = np.sign(np.diff(counts)); s = s[s != 0]
    turns = "".join("+" if x > 0 else "-" for x in s)
    assert re.search(r"\+.*-.*\+", turns), (counts, turns)
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 3. light counts

@pytest.mark.parametrize("n_point", [0, 1, 3, 4, 16, CAP, CAP + 1])
def test_light_counts(gpu_engine, n_point):
    """3 and 4 straddle the threshold above which the other resting kernels build a tile list (this one always does).  With no light
    every part settles by the second resting launch.  65 lights are one too many for the argument: those frames go through XkView and
    write every pixel, nothing is settled behind them (asserted: the count reads 0), and with 16 lights again the frames are one launch.
    That the FIRST of those launches leaves nothing alone cannot be read off the marks: they are read after the frame, and a launch
    that shaded every part has by then marked the ones no light reaches - the count after it is the prediction's either way.  What holds
    it is the twin comparison of that frame (the lights moved through three frames meanwhile: a part wrongly left alone would hold
    stale pixels) and, without a GPU, tests/settle_check.cpp: a pass of another kernel always moves the generation on."""
    st = SStage(n_point)
    g, twin = _pairs(st, gpu_engine)
    for i in range(6):
        did = _pair(g, twin, st, i, "%d lights" % n_point)
        if i >= 4 and n_point <= CAP:
            parts, settled, which = _held(g, st, "%d lights, frame %d" % (n_point, i))
            if n_point == 0:
                assert settled == parts
    assert did == "read" and _by_arg(g) == (0 if n_point > CAP else 3)
    if n_point > CAP:
        assert g.rest_settled()[1] == 0
        st.lights = SStage(16).lights
        for i in range(6, 10):
            assert _pair(g, twin, st, i, "back to 16 lights") == "read"
            if i >= 8:
                _held(g, st, "back to 16 lights, frame %d" % i)
        assert _by_arg(g) == 4
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 4. the empty pixel

def test_no_part_with_an_empty_pixel_settles_while_a_light_reaches_the_origin(gpu_engine):
    """The mirror stage of test_the_empty_pixels_colour_moves_with_the_lights with lights of radius 0.8, which ride their spiral a unit
    above the origin and never reach it - except that on frames 5, 7, 10 and 11 light 0 has radius 8 and stands in the mirror
    direction, five units from the origin.  On exactly those frames the empty colour changes and no part that holds an empty pixel is
    settled (zr_get_rest_settled_parts, part by part); on the others parts that hold one do settle."""
    st = SStage(16, cam=((-9.0, -7.0, 6.0), (0.0, 0.0, 1.0)))
    mirror = (5, 7, 10, 11)
    g, twin = _pairs(st, gpu_engine)
    px, seen = [], []
    for i in range(13):
        st.mirror = mirror if i in mirror else ()
        st.lights[1]["Direction"][0, 3] = 8.0 if i in mirror else RADIUS
        did = _pair(g, twin, st, i, "mirror")
        e = _empty(g)
        assert e.any() and not e.all()
        c = g.color()[e]
        assert (c == c[0]).all(), "empty pixels of one frame differ"
        px.append(c[0].tolist())
        if i >= 4:
            assert did == "read"
            parts, settled, which = _held(g, st, "mirror, frame %d" % i)
            holds_empty = np.array([f >= 0 for f in _first_empty_per_workgroup(e)])
            assert len(holds_empty) == parts and holds_empty.any() and not holds_empty.all()
            seen.append((i in mirror, int(which[holds_empty].sum())))
    print(px, seen)
    for on, standing_with_empty in seen:
        assert standing_with_empty == 0 if on else standing_with_empty > 0, seen
    assert all(px[i] == px[5] for i in mirror) and all(px[i] == px[4] for i in range(3, 13) if i not in mirror) and px[5] != px[4], px
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 5. a change in the middle of a settled run

CHANGES = ["debug_view", "background_set", "background_toggled", "overlay", "highlight", "instances", "texture", "resize", "forward", "view9", "light_cap"]


@pytest.mark.parametrize("change,size", [(c, (160, 120)) for c in CHANGES] + [("debug_view", (33, 17)), ("background_set", (33, 17)), ("instances", (33, 17))])
def test_a_change_in_the_middle_of_a_settled_run(gpu_engine, change, size):
    """Six frames (parts stand settled), the change, and ten frames more: every one is the twin's.  Where the change is taken back
    (view, background flag, extent, shading, light count) the frames after that are too.  Whatever the change, the run settles again,
    and the parts that then stand are the prediction's.  (33 x 17: two tiles across, one of them a column wide, parts of sixteen rows
    and of one.)"""
    st = SStage(16, size=size)
    st.box_image = np.random.default_rng(7).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    g, twin = _pairs(st, gpu_engine)
    bg = scenes.synthetic_sky_image(48, 32)
    if change == "background_toggled":
        for r in (g, twin):
            r.set_background(bg)
    assert _rest(g, twin, st, 6) == "read"
    assert 0 < g.rest_settled()[1]

    def both(f):
        for r in (g, twin):
            f(r)

    back = None
    if change == "debug_view":
        both(lambda r: r.set_debug_view(1)); back = lambda r: r.set_debug_view(0)
    elif change == "background_set":
        both(lambda r: r.set_background(bg)); back = lambda r: r.set_background(255 - bg)
    elif change == "background_toggled":
        both(lambda r: r.set_sky_flags(True, False)); back = lambda r: r.set_sky_flags(True, True)
    elif change == "overlay":
        both(lambda r: r.overlay_set(SEGMENTS))
    elif change == "highlight":
        both(lambda r: (r.set_id_capture(True), r.highlight_set(SPHERES, np.ones(40, dtype=np.uint8))))      # (the highlight's mask reads the winners)
    elif change == "instances":
        new = st.inst.copy(); new["InstancePosition"][:60, 2] += np.float32(2.5)
        both(lambda r: r.object_set_instances(SPHERES, new[:60]))
    elif change == "texture":
        both(lambda r: r.object_set_texture(BOX, 0, 255 - st.box_image))
    elif change == "resize":
        both(lambda r: r.resize(100, 72)); back = lambda r: r.resize(st.W, st.H)
    elif change == "forward":
        both(lambda r: r.set_shading(True)); back = lambda r: r.set_shading(False)
    elif change == "view9":
        both(lambda r: r.set_debug_view(9)); back = lambda r: r.set_debug_view(0)
    else:
        keep = st.lights
        st.lights = SStage(CAP + 1).lights
        back = lambda r: None
    _rest(g, twin, st, 4, 6, change)
    if change in ("overlay", "highlight"):      # delivered forms: drawn over the frame elsewhere, the frame itself stays the library's
        a, b = _delivered(g, change), _delivered(twin, change)
        assert np.array_equal(a, b), change
    if back is not None:
        if change == "light_cap":
            st.lights = keep
        both(back)
    assert _rest(g, twin, st, 6, 10, change + ", after") in ("read", "filled")
    assert _rest(g, twin, st, 2, 16, change + ", settled again") == "read"
    assert _held(g, st, change + ", settled again")[1] > 0, change
    g.close(); twin.close()


SEGMENTS = [(-3.0, -3.0, 0.5, 3.0, 3.0, 2.5, 255, 255, 0, 255), (-3.0, 3.0, 1.0, 3.0, -3.0, 1.0, 0, 255, 255, 255)]


def _delivered(r, change):
    return r.read_color_overlaid(1, False) if change == "overlay" else r.color_highlighted(1)


# ------------------------------------------------------------------------------------------------ 6. frames in flight

def test_twelve_frames_enqueued_without_a_host_synchronisation(gpu_engine):
    import torch
    dev = torch.device("cuda", 0)
    N, out = 12, {}
    for f in (abi.FLAG_NO_LIST_REUSE, 0):
        st = SStage(16)
        r = st.renderer(gpu_engine, f)
        col = [torch.zeros(st.W * st.H, dtype=torch.int32, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        did = []
        for k in range(N):
            st.uniforms(r, k)
            r.render()
            r.copy_frame_async(col[k].data_ptr(), None)
            did.append(_last(r))
        r.finish()
        out[f] = ([c.cpu().numpy() for c in col], did, r.rest_settled(), _by_arg(r))
        r.close()
    got, ref = out[0], out[abi.FLAG_NO_LIST_REUSE]
    for k in range(N):
        assert np.array_equal(got[0][k], ref[0][k]), "queued frame %d: %d pixels differ" % (k, int((got[0][k] != ref[0][k]).sum()))
    print(got[1], got[2])
    assert got[1] == ["ignored", "ignored", "filled"] + ["read"] * 9 and got[3] == 9
    assert 0 < got[2][1] < got[2][0] and ref[2][1] == 0


# ------------------------------------------------------------------------------------------------ 7. frame shapes, 8. a non-finite position

@pytest.mark.parametrize("shape", ["one_partial_tile", "no_empty_pixel", "only_empty_pixels", "first_empty_in_last_wave"])
def test_frame_shapes(oracle_lib, gpu_engine, shape):
    if shape == "one_partial_tile":
        st = SStage(16, size=(40, 24))
    elif shape == "no_empty_pixel":
        st = SStage(16, cam=((0.5, -0.5, 5.0), (0.0, 0.0, 0.0)))
    elif shape == "only_empty_pixels":
        st = SStage(16, cam=((9.0, -7.0, 6.0), (30.0, -25.0, 40.0)))
    else:
        st = SStage(16, cam=_last_wave_camera(oracle_lib))
    g, twin = _pairs(st, gpu_engine)
    for i in range(8):
        did = _pair(g, twin, st, i, shape)
        if i >= 4:
            assert did == "read"
            _held(g, st, "%s, frame %d" % (shape, i))
    e = _empty(g)
    if shape == "no_empty_pixel":
        assert not e.any()
    elif shape == "only_empty_pixels":
        assert e.all()
    elif shape == "first_empty_in_last_wave":
        assert any(f >= 448 for f in _first_empty_per_workgroup(e))
    g.close(); twin.close()


def test_a_part_with_a_non_finite_position_never_settles(gpu_engine):
    """test_non_finite_position's stage: the record of a part that holds such a pixel is -inf .. +inf, every light reaches it."""
    st = SStage(16, cam=((9.0, -7.0, 6.0), (70000.0, 0.0, 0.0)), zfar=1.0e6)
    inst = st.inst.copy()
    inst["InstancePosition"][0] = (70000.0, 0.0, 0.0); inst["InstancePScale"][0] = 10000.0
    st.inst = inst
    g, twin = _pairs(st, gpu_engine)
    for i in range(7):
        _pair(g, twin, st, i, "non-finite position")
        if i >= 4:
            parts, settled, which = _held(g, st, "non-finite, frame %d" % i)
    d = g.gbuffer(5)
    pos = np.stack([(d >> (16 * k)) & 0xFFFF for k in range(3)]).astype(np.uint16).view(np.float16)
    bad = np.isinf(pos).any(axis=0)
    assert bad.any(), "no pixel's position is inf"
    n_bad = 0
    for ty in range(0, st.H, 32):
        for tx in range(0, st.W, 32):
            for half in (0, 16):
                n_bad += bool(bad[ty + half:ty + half + 16, tx:tx + 32].any())
    print(parts, settled, n_bad)
    assert n_bad > 0 and settled <= parts - n_bad
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 9. the switch, 10. packed tiles

def test_zr_no_rest_settle(gpu_engine, monkeypatch):
    """A context made with ZR_NO_REST_SETTLE in the environment rests through k_lighting_rest: nothing ever settles, and its frames are
    the default context's byte for byte (and the twin's)."""
    st = SStage(16)
    g, twin = _pairs(st, gpu_engine)
    monkeypatch.setenv("ZR_NO_REST_SETTLE", "1")
    off = st.renderer(gpu_engine)
    monkeypatch.delenv("ZR_NO_REST_SETTLE")
    for i in range(10):
        did = _pair(g, twin, st, i, "switch")
        assert _pair(off, twin, st, i, "switch, off") == did
        assert off.rest_settled()[1] == 0
        assert off.color().tobytes() == g.color().tobytes()
    assert g.rest_settled()[1] > 0 and _by_arg(off) == _by_arg(g) == 7
    g.close(); twin.close(); off.close()


def test_packed_tiles_on_one_gpu_settle_too(gpu_engine):
    st = SStage(16)
    g, twin = _pairs(st, gpu_engine, abi.FLAG_PACKED_TILES)
    for i in range(8):
        did = _pair(g, twin, st, i, "packed tiles")
        assert np.array_equal(g.read_tiles(), twin.read_tiles()), i
        if i >= 4:
            assert did == "read"
            _held(g, st, "packed tiles, frame %d" % i)
    assert 0 < g.rest_settled()[1]
    g.close(); twin.close()


def test_the_tiles_buffer_switched_in_the_middle_of_a_settled_run(gpu_engine):
    """Case 5's "packed tiles": a ZR_FLAG_PACKED_TILES context on one GPU settles in its own buffer; zr_set_tiles_buffer then points
    the frames at a caller's buffer - the library vouches for nothing there: nothing stands, every tile is written - and back at the
    internal one, whose bytes are four frames old by then: a new generation shades every part once before any stands again.  Every
    frame's tiles are the twin's."""
    import torch
    st = SStage(16)
    g, twin = _pairs(st, gpu_engine, abi.FLAG_PACKED_TILES)

    def frames(i0, n, what):
        for i in range(i0, i0 + n):
            did = _pair(g, twin, st, i, what)
            a, b = g.read_tiles(), twin.read_tiles()
            assert np.array_equal(a, b), "%s, frame %d: %d tile bytes differ" % (what, i, int((a != b).sum()))
        return did

    assert frames(0, 6, "own buffer") == "read" and g.rest_settled()[1] > 0
    nbytes = g.tiles_device_buffer()[1]
    mine = [torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in (g, twin)]
    torch.cuda.synchronize()
    for r, m in zip((g, twin), mine):
        r.set_tiles_buffer(m.data_ptr())
    for i in range(6, 10):
        assert frames(i, 1, "caller's buffer") == "read" and g.rest_settled()[1] == 0 and not g.rest_settled_parts().any()
    for r in (g, twin):
        r.set_tiles_buffer(None)
    assert frames(10, 1, "own buffer again") == "read"
    assert frames(11, 3, "own buffer again") == "read"
    assert _held(g, st, "own buffer again")[1] > 0 and _by_arg(g) == 11
    g.close(); twin.close()


def test_a_handed_out_frame_address_ends_it(gpu_engine):
    """zr_color_device_ptr lets the caller write through the address: from that call on nothing settles, every pixel is written again -
    a pixel the caller overwrote is the frame's again after the next resting frame."""
    import ctypes as C
    st = SStage(16)
    g, twin = _pairs(st, gpu_engine)
    assert _rest(g, twin, st, 6) == "read" and g.rest_settled()[1] > 0
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    junk = np.full(st.W * st.H, 0x00FF00FF, dtype=np.uint32)
    assert hip.hipMemcpy(C.c_void_p(g.color_device_ptr()), junk.ctypes.data_as(C.c_void_p), junk.nbytes, 1) == 0
    assert _rest(g, twin, st, 3, 6, "after the hand-out") == "read"
    assert g.rest_settled()[1] == 0
    g.close(); twin.close()
