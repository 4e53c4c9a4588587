"""The resting frame's launch decides a part once, in the workgroup's first wave (csrc/zr_lighting.hip: k_lighting_lead).

k_lighting_lead is k_lighting_stand with the decision - the part's box, its first empty pixel, the lights' ballot, settled or not - made
by wave 0 and handed to the other seven through LDS.  Nothing a frame holds and nothing zr_get_rest_settled reports may differ: a
context made with ZR_NO_LEAD_WAVE in the environment rests through k_lighting_stand, and the two are compared frame by frame, byte for
byte, with each other and with a ZR_FLAG_NO_LIST_REUSE twin - over a sweep in which the settled count moves, at the extents of
test_gpu_rest_settle.py (33 x 17: parts of sixteen rows and of one, a tile a column wide), with and without empty pixels, with the
empty pixel's colour moving, and with a background image (the other instantiation).  The settled set is also held to
test_gpu_rest_settle.py's prediction.  Every other resting case of that file and of test_gpu_rest_one_launch.py runs through this
kernel too: it is what a default context launches.
"""
import numpy as np
import pytest

from test_gpu_lighting_keep import _pair
from test_gpu_rest_one_launch import _by_arg, _pairs
from test_gpu_rest_settle import EXTENTS, RADIUS, SWEEP, SStage, _held
from zeldaengine_amd import scenes

pytestmark = pytest.mark.gpu


def _three(st, eng, monkeypatch):
    g, twin = _pairs(st, eng)
    monkeypatch.setenv("ZR_NO_LEAD_WAVE", "1")
    stand = st.renderer(eng)
    monkeypatch.delenv("ZR_NO_LEAD_WAVE")
    return g, stand, twin


def _frame(g, stand, twin, st, i, what):
    did = _pair(g, twin, st, i, what)
    assert _pair(stand, twin, st, i, what + ", k_lighting_stand") == did
    assert stand.color().tobytes() == g.color().tobytes()
    assert stand.rest_settled() == g.rest_settled() and np.array_equal(stand.rest_settled_parts(), g.rest_settled_parts()), (what, i)
    return did


@pytest.mark.parametrize("size", EXTENTS)
def test_sweep_is_k_lighting_stands_frame_for_frame(gpu_engine, monkeypatch, size):
    st = SStage(16, size=size, radius=SWEEP[size][0], rate=SWEEP[size][1])
    g, stand, twin = _three(st, gpu_engine, monkeypatch)
    counts = []
    for i in range(14):
        did = _frame(g, stand, twin, st, i, "sweep %dx%d" % size)
        if i >= 4:
            assert did == "read"
            counts.append(_held(g, st, "frame %d" % i)[1])
    print(size, counts)
    assert _by_arg(g) == _by_arg(stand) == 11 and len(set(counts)) > 1, counts
    for r in (g, stand, twin):
        r.close()


@pytest.mark.parametrize("shape", ["no_empty_pixel", "only_empty_pixels", "mirror", "background", "no_light"])
def test_frame_shapes_are_k_lighting_stands(gpu_engine, monkeypatch, shape):
    """mirror: test_gpu_rest_settle's stage in which light 0 reaches the origin on frames 5 and 7 - the empty pixel's colour, computed by
    its owner and parked in LDS, changes, and no part that holds one stands; background: the instantiation that samples the image."""
    cam = {"no_empty_pixel": ((0.5, -0.5, 5.0), (0.0, 0.0, 0.0)), "only_empty_pixels": ((9.0, -7.0, 6.0), (30.0, -25.0, 40.0)),
           "mirror": ((-9.0, -7.0, 6.0), (0.0, 0.0, 1.0))}.get(shape)
    st = SStage(0 if shape == "no_light" else 16, cam=cam)
    g, stand, twin = _three(st, gpu_engine, monkeypatch)
    if shape == "background":
        for r in (g, stand, twin):
            r.set_background(scenes.synthetic_sky_image(48, 32))
    mirror = (5, 7) if shape == "mirror" else ()
    settled = []
    for i in range(9):
        st.mirror = mirror if i in mirror else ()
        if shape == "mirror":
            st.lights[1]["Direction"][0, 3] = 8.0 if i in mirror else RADIUS
        did = _frame(g, stand, twin, st, i, shape)
        if i >= 4:
            assert did == "read"
            settled.append(_held(g, st, "%s, frame %d" % (shape, i))[1])
    print(shape, settled)
    if shape == "no_light":
        assert settled[-1] == g.rest_settled()[0]
    if shape == "mirror":
        assert settled[1] < settled[0] and settled[3] < settled[2], settled      # frames 5 and 7 against 4 and 6
    for r in (g, stand, twin):
        r.close()


@pytest.mark.parametrize("background", [False, True])
def test_the_three_resting_kernels_write_the_same_frame(gpu_engine, monkeypatch, background):
    """k_lighting_lead (a default context), k_lighting_stand (ZR_NO_LEAD_WAVE) and k_lighting_rest (ZR_NO_REST_SETTLE) run the same
    shared steps - the tables, the box, the first empty pixel, the pixel tail - and write the same bytes as each other and as the
    ZR_FLAG_NO_LIST_REUSE twin, at 33 x 17: parts of sixteen rows and of one, a tile a column wide, threads outside the frame; plain and
    with a background image (the tail's other instantiation).  The context that never settles reports nothing settled."""
    size = (33, 17)
    st = SStage(16, size=size, radius=SWEEP[size][0], rate=SWEEP[size][1])
    g, stand, twin = _three(st, gpu_engine, monkeypatch)
    monkeypatch.setenv("ZR_NO_REST_SETTLE", "1")
    rest = st.renderer(gpu_engine)
    monkeypatch.delenv("ZR_NO_REST_SETTLE")
    if background:
        for r in (g, stand, rest, twin):
            r.set_background(scenes.synthetic_sky_image(48, 32))
    for i in range(9):
        did = _frame(g, stand, twin, st, i, "three kernels")
        assert _pair(rest, twin, st, i, "three kernels, k_lighting_rest") == did
        assert rest.color().tobytes() == g.color().tobytes(), i
        assert rest.rest_settled()[1] == 0
        if i >= 4:
            assert did == "read"
    assert _by_arg(g) == _by_arg(stand) == _by_arg(rest) == 6
    for r in (g, stand, rest, twin):
        r.close()
