"""A timed frame records the events of the stages it runs, and no others (csrc/zr_timed.h; DESIGN.md section 5, "The schedule").

A stage the plan does not run records nothing: its figures read exactly 0.0, from the rule stored with the sample and not from events a
ring slot still holds from the frame that used it 64 samples earlier.  A frame that is one launch records its begin and its end.

The stage is test_gpu_rest_one_launch.py's at 96 x 64 with a 64^2 map: the smallest shapes here where a tile is partial on both edges
and a rest is reached.  The renderer under test samples every frame; its ZR_FLAG_NO_LIST_REUSE twin, which keeps nothing, samples none.
Every colour compared is byte-equal.  A read-out that left an error behind in the runtime's last-error state would fail the next frame,
whose passes check it: every read-out here is followed by a call that must succeed.
"""
import pytest

from test_gpu_lighting_keep import _last
from test_gpu_rest_one_launch import RStage, _by_arg, _pairs

pytestmark = pytest.mark.gpu

SHADOW = ("cull_shadow", "shadow")
CAMERA = ("cull_camera", "gbuffer", "hiz", "gbuffer2", "resolve")
ROUND2 = ("hiz", "gbuffer2")


def _stage():
    st = RStage(16, size=(96, 64))
    st.SD = 64
    return st


def _frame(g, twin, st, i):
    """frame i on both, compared; -> g's pass times and what its lighting pass did with the plane"""
    for r in (g, twin):
        st.uniforms(r, i)      # (on g: the first call behind the previous frame's read-out)
        r.render(); r.finish()
    a, b = g.color(), twin.color()
    assert a.tobytes() == b.tobytes(), "frame %d: %d pixels differ from the twin's" % (i, int((a != b).any(axis=2).sum()))
    t = g.pass_times(1)
    assert g.frame_latencies(1) == [t["total"]], (i, t)
    return t, _last(g)


def test_every_frame_shape(gpu_engine):
    """Drawn, drawn, the fill, three frames of one launch, a light move (the map drawn, the camera pass kept), a camera move."""
    st = _stage()
    g, twin = _pairs(st, gpu_engine)
    g.set_timing_interval(1); twin.set_timing_interval(0)
    # per frame: the stages that ran (every other figure is exactly 0.0).  Frame 0 draws one round and records EV_HIZ and EV_ROUND2 back to
    # back all the same: its two round-2 figures are the gap between two records, as before the rule, and are asserted neither way.
    ran = [SHADOW + CAMERA, CAMERA, (), (), (), (), SHADOW, CAMERA]
    did, by_arg = [], []
    for i in range(8):
        if i == 6:
            st.light = (5.5, 0.5, 14.0)
        if i == 7:
            st.cam = ((9.0, -7.0, 6.5), (0.0, 0.0, 1.0))
        t, last = _frame(g, twin, st, i)
        did.append(last); by_arg.append(_by_arg(g))
        print(i, last, {k: round(v, 5) for k, v in t.items()})
        for k in SHADOW + CAMERA:
            if i == 0 and k in ROUND2:
                continue
            if k in ran[i]:
                assert t[k] > 0.0, (i, k, t)
            else:
                assert t[k] == 0.0, (i, k, t)
        assert t["composite"] == 0.0 and t["total"] >= t["lighting"] > 0.0, (i, t)
    g.finish()      # (the call behind the last read-out)
    assert did == ["ignored", "ignored", "filled", "read", "read", "read", "ignored", "ignored"], did
    assert by_arg == [0, 0, 0, 1, 2, 3, 3, 3], by_arg
    with pytest.raises(gpu_engine.ZeldaRenderError):
        twin.pass_times(1)      # (it sampled nothing)
    g.close(); twin.close()


@pytest.mark.parametrize("every", [4, 8])
def test_sparse_ends_in_flight(gpu_engine, every):
    """ZR_REST_END_EVERY = 4 / 8 against a twin with 1 (every frame records its end, as before the rule), 46 frames enqueued without a host
    synchronisation: two drawn frames and the fill, ten frames of one launch, a texture update - its stream waits for the end of the frame
    enqueued last, which recorded none - and the three frames that follow it, seven of one launch, a camera cut with its three, a rest
    of twenty.  Every frame, copied out in stream order, is the twin's; every period is > 0; frames inside one sparse run report one
    value (csrc/zr_frame_end.h)."""
    import os
    import numpy as np
    import torch
    from test_gpu_round2_keep import BOX
    dev = torch.device("cuda", 0)
    N, out = 46, {}
    for r_every in (1, every):
        st = _stage()
        st.box_image = np.random.default_rng(7).integers(0, 256, (16, 16, 4), dtype=np.uint8)
        old = os.environ.get("ZR_REST_END_EVERY")
        os.environ["ZR_REST_END_EVERY"] = str(r_every)
        try:
            r = st.renderer(gpu_engine)
        finally:
            if old is None:
                del os.environ["ZR_REST_END_EVERY"]
            else:
                os.environ["ZR_REST_END_EVERY"] = old
        r.set_timing_interval(0)
        col = [torch.zeros(st.W * st.H, dtype=torch.int32, device=dev) for _ in range(N)]
        torch.cuda.synchronize()
        by_arg = []
        for k in range(N):
            if k == 13:
                r.object_set_texture(BOX, 0, 255 - st.box_image)
            if k == 23:
                st.cam = ((9.0, -7.0, 6.5), (0.0, 0.0, 1.0))
            st.uniforms(r, k)
            r.render()
            r.copy_frame_async(col[k].data_ptr(), None)
            by_arg.append(_by_arg(r))
        per = r.frame_periods(N - 1)      # (waits for the frames)
        assert r.stats()["overflow"] == 0
        out[r_every] = ([c.cpu().numpy() for c in col], by_arg, per)
        r.close()
    got, ref = out[every], out[1]
    for k in range(N):
        assert np.array_equal(got[0][k], ref[0][k]), "queued frame %d: %d pixels differ" % (k, int((got[0][k] != ref[0][k]).sum()))
    args = [b > a for a, b in zip([0] + got[1][:-1], got[1])]      # frame k ran as one launch
    print(every, "".join("1" if a else "." for a in args), [round(x, 4) for x in got[2]])
    assert args == [False] * 3 + [True] * 10 + [False] * 3 + [True] * 7 + [False] * 3 + [True] * 20 and got[1] == ref[1], args
    assert not np.array_equal(got[0][12], got[0][13]) and not np.array_equal(got[0][22], got[0][23])      # (the update and the cut show)
    for per in (got[2], ref[2]):
        assert len(per) == N - 1 and all(x > 0.0 for x in per), per
    # the last rest is frames 26 .. 45.  A frame behind a one-launch frame records its end where its number is a multiple of `every`, and
    # nobody asks for an end inside that rest: the frames from one multiple (exclusive) to the next (inclusive) are one run.
    period = {k: got[2][N - 1 - k] for k in range(1, N)}      # (newest first)
    m1 = (27 + every - 1) // every * every
    m2 = m1 + every
    assert 27 <= m1 and m2 <= N - 1
    run = [period[k] for k in range(m1 + 1, m2 + 1)]
    assert len(set(run)) == 1, (m1, m2, run)
    assert len(set(ref[2][:19])) > 1      # (the twin's frames each report their own)


def test_a_slot_a_drawn_frame_used_is_reused_by_a_frame_of_one_launch(gpu_engine):
    """77 sampled frames, more than the ring's 64, in cycles of six: the camera moves, two drawn frames, the fill, three frames of one
    launch.  64 is no multiple of 6, so the slots change hands: the last frame is one launch, and the sample 64 before it, whose events
    its slot still holds, was a drawn frame's.  The light stands from frame 0 on, so every sampled map of the last 64 was kept."""
    st = _stage()
    g = st.renderer(gpu_engine)
    g.set_timing_interval(1)
    N, did = 77, []
    for i in range(N):
        if i % 6 == 0:
            st.cam = ((9.0, -7.0, 6.0 + 0.05 * (i // 6)), (0.0, 0.0, 1.0))
        st.uniforms(g, i)
        g.render()
        did.append(_last(g))
    g.finish()
    assert did == ["ignored", "ignored", "filled", "read", "read", "read"] * 12 + ["ignored", "ignored", "filled", "read", "read"], did
    assert _by_arg(g) == 38 and did[N - 1] == "read" and did[N - 1 - 64] == "ignored"
    t1 = g.pass_times(1)
    g.finish()
    assert all(t1[k] == 0.0 for k in SHADOW + CAMERA) and t1["total"] >= t1["lighting"] > 0.0, t1
    t64 = g.pass_times(64)
    g.finish()
    assert all(t64[k] == 0.0 for k in SHADOW) and all(t64[k] > 0.0 for k in CAMERA + ("lighting", "total")), t64
    # S(n) = n * mean(n), the sum over the last n samples, never falls: every term is an elapsed time between two events of ONE sample, in
    # stream order.  The mean is a float32 of a double sum: S(n) carries a relative error of 2^-24, so 2^-23 S(n) bounds what a step may
    # lose to rounding.
    for k in SHADOW + CAMERA + ("lighting",):
        S = [n * g.pass_times(n)[k] for n in range(1, 65)]
        assert all(S[n] >= S[n - 1] - S[n] * 2.0 ** -23 for n in range(1, 64)), (k, S)
    # frames N-1 and N-2 are one launch, N-3 the fill, N-4 and N-5 drawn: the camera figures' sums stand, then rise
    S = [n * sum(g.pass_times(n)[k] for k in CAMERA) for n in range(1, 6)]
    assert S[0] == S[1] == S[2] == 0.0 and S[4] > S[3] > 0.0, S
    st.uniforms(g, N); g.render(); g.finish()      # (the frame behind the read-outs)
    g.close()
