"""Seeded sessions of updates, rests and deliveries on the renderer, every frame and every delivery held to its statement.

tests/session_model.py draws, per seed, 24 to 40 frames with 0 to 3 operations in the gap before each - every between-frames entry
point, at every rest depth, alone and beside an operation of another family - through zr_render, the staged calls or zr_render_geometry,
with the point lights moving or standing, and readers behind the frame.  tests/test_session_model.py holds that generator to its claims.
Here each script is played on a context of the seed's flavour (flags 0, ZR_FLAG_SERIAL_PASSES, ZR_FLAG_NO_LIST_REUSE, or created with a
skydome), timing interval 1:

  * after a synchronised frame colour, the six GBuffer planes and the shadow map are compared bit for bit with a fresh oracle of the
    model's state (which knows nothing of epochs, copies or keeps), and the step's readers with their own statements fed that frame;
  * inside a stretch without host synchronisation the frame goes through zr_copy_frame_async, and the device-form readers write, into
    buffers of that frame's own, all compared after the stretch;
  * zr_stats.overflow stays 0;
  * a frame of rest depth >= 3 on a default context (flags 0, no skydome, deferred shading) keeps its whole camera pass - the five camera
    pass times are exactly 0.0, the lighting time is above 0.0 ("The schedule") - and one whose predecessor was such a
    frame too, with sun and casters standing, the lights standing still and at most ZR_REST_ARG_LIGHTS of them, reads the plane of
    standing terms: a session cannot pass by never resting.

A failure names seed, flavour, frame and what differs by how much, says how session_model.run replays it (a session starts from
Model(seed)'s state, so the prefix up to the failing frame is played), and prints the steps since the last frame that passed as a
literal list; cut down by hand, such a list is pinned here as a named test (no default seed has failed so far).

ZR_SESSION_SEEDS / ZR_SESSION_BASE: more seeds, from another base, for a longer hunt (as ZR_FUZZ_SEEDS).

Measured on the MI355X, the 24 default seeds: wall time per seed, oracle included, median 0.48 s, maximum 1.14 s.  Census per seed
(frames in all, those of unsynchronised stretches included; of the synchronised ones: drawn / round 2 kept / camera pass kept; plane
filled / read / read by argument; parts settled after the last one-launch frame), as the test prints it:
  seed  0 skydome  : 28 in all,  8 /  9 /  0;  0 /  0 /  0; -       seed 12 flags   0: 27 in all,  9 /  0 /  8;  4 /  7 /  7; 0 of 30
  seed  1 flags 256: 27 in all, 16 /  0 /  0;  0 /  0 /  0; -       seed 13 skydome  : 30 in all, 13 / 17 /  0;  0 /  0 /  0; -
  seed  2 skydome  : 25 in all, 12 /  7 /  0;  0 /  0 /  0; -       seed 14 flags 256: 26 in all, 20 /  0 /  0;  0 /  0 /  0; -
  seed  3 flags   0: 24 in all, 13 /  4 /  7;  1 /  1 /  0; -       seed 15 flags   0: 24 in all, 12 /  2 /  5;  3 /  5 /  0; -
  seed  4 flags   0: 27 in all,  7 /  1 /  8;  3 /  3 /  3; 0 of 30 seed 16 skydome  : 24 in all,  6 /  7 /  0;  0 /  0 /  0; -
  seed  5 flags  16: 32 in all, 13 /  3 / 11;  6 /  7 /  7; 0 of 12 seed 17 flags   0: 24 in all, 10 /  4 /  5;  5 /  4 /  3; 0 of 4
  seed  6 flags   0: 26 in all, 15 /  3 /  8;  6 /  2 /  2; 0 of 12 seed 18 skydome  : 31 in all, 12 / 13 /  0;  0 /  0 /  0; -
  seed  7 skydome  : 24 in all, 14 / 10 /  0;  0 /  0 /  0; -       seed 19 flags   0: 32 in all, 14 /  0 / 18;  5 / 13 /  6; 0 of 12
  seed  8 flags  16: 26 in all,  9 /  7 /  4;  3 /  1 /  1; 0 of 30 seed 20 flags 256: 25 in all, 14 /  0 /  0;  0 /  0 /  0; -
  seed  9 flags   0: 25 in all, 11 /  7 /  7;  3 /  1 /  1; 0 of 12 seed 21 skydome  : 30 in all, 14 /  9 /  0;  0 /  0 /  0; -
  seed 10 flags   0: 24 in all, 11 /  4 /  4;  3 /  5 /  5; 0 of 30 seed 22 flags   0: 24 in all, 13 /  0 /  6;  5 /  3 /  2; 0 of 12
  seed 11 flags   0: 24 in all,  7 /  4 /  3;  3 /  2 /  2; 0 of 12 seed 23 flags   0: 29 in all, 11 /  5 / 13;  2 /  3 /  3; 0 of 30
The camera-pass keep was asserted on 39 frames of the default-flag seeds, the plane's read on 6.  Mutations of the library that the
default seeds catch: g_gen without its surface_epoch term (seeds 3, 5, 6, 8, 9, 10, 11, 15, 17), light_match without its cubemap
generation (seed 12).
"""
import os
import time

import numpy as np
import pytest

import session_model as sm
from parity_util import TARGET_NAMES
from zeldaengine_amd import abi

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("ZR_SESSION_SEEDS", sm.DEFAULT_SEEDS))
BASE = int(os.environ.get("ZR_SESSION_BASE", 0))
CAMERA_PASSES = ("cull_camera", "gbuffer", "hiz", "gbuffer2", "resolve")


def _whole(t):
    """the frame kept its whole camera pass (the predicate of test_gpu_gbuffer_keep.py)"""
    return all(t[k] == 0.0 for k in CAMERA_PASSES) and t["lighting"] > 0.0


def _diff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return "shape %r, expected %r" % (a.shape, b.shape)
    if a.dtype.names:
        bad = np.array([x.tobytes() != y.tobytes() for x, y in zip(a.reshape(-1), b.reshape(-1))])
        k = int(np.flatnonzero(bad)[0]) if bad.any() else -1
        return None if k < 0 else "%d of %d records differ, first %d: %r, expected %r" % (int(bad.sum()), bad.size, k, a.reshape(-1)[k], b.reshape(-1)[k])
    ne = a.view(np.uint8) != b.view(np.uint8) if a.dtype != np.uint8 else a != b
    if not ne.any():
        return None
    k = int(np.flatnonzero(ne.reshape(-1))[0])
    return "%d of %d bytes differ, the first at %r" % (int(ne.sum()), ne.size, tuple(int(x) for x in np.unravel_index(k, ne.shape)))


class Player(sm.Hooks):
    def __init__(self, seed, steps, g, engine, flags, sky):
        import torch
        self.torch, self.dev_ = torch, torch.device("cuda", 0)
        self.seed, self.steps, self.g, self.engine, self.flags, self.sky = seed, steps, g, engine, flags, sky
        self.side = torch.cuda.Stream(device=self.dev_)      # uploads go through a stream of their own: the session's streams are not drained
        self.keep, self.pending, self.last_ok, self.gclient, self.client_of = [], [], -1, None, None
        self.census = dict.fromkeys(("frames", "drawn", "round2_kept", "camera_kept", "keep_asserted", "read_asserted"), 0)
        self.default = flags == 0 and not sky

    # ---- plumbing
    def fail(self, i, what):
        raise AssertionError("seed %d, flags %d%s, frame %d: %s\nto replay (a session starts from Model(seed)'s state, so the whole prefix is played): "
                             "session_model.run(steps, upto=%d, seed=%d, ...) with steps = session_model.script(%d), or a list cut down from it\n"
                             "the steps since the last frame that passed (%d):\n%r"
                             % (self.seed, self.flags, ", skydome" if self.sky else "", i, what, i + 1, self.seed, self.seed, self.last_ok,
                                self.steps[self.last_ok + 1:i + 1]))

    def same(self, i, what, got, want):
        d = _diff(got, want)
        if d:
            self.fail(i, "%s: %s" % (what, d))

    def up(self, a):
        """an array -> a device tensor of its bytes, complete when this returns"""
        t = self.torch
        with t.cuda.stream(self.side):
            out = t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev_)
        self.side.synchronize()
        self.keep.append(out)
        return out

    def dev(self, a, row):
        t = self.up(a)
        return t.reshape(a.shape) if row is None else t.reshape(-1, row)

    def buffer(self, nbytes):
        t = self.torch
        with t.cuda.stream(self.side):
            out = t.zeros((nbytes + 15) // 16 * 16, dtype=t.uint8, device=self.dev_)
        self.side.synchronize()
        self.keep.append(out)
        return out

    def rays(self, reader, m):
        g = self.g
        cam = [g.camera_ray((x + 0.5) * m.W / 6.0, (y + 0.5) * m.H / 4.0) for y in range(4) for x in range(6)]
        return np.concatenate(cam + [m.free_rays(reader[1])])

    # ---- frames
    def flush(self, i):
        """what the frames of a stretch without synchronisation left in their buffers (the host has synchronised since)"""
        for j, what, buf, want in self.pending:
            got = buf.cpu().numpy()[:want.nbytes].view(want.dtype).reshape(want.shape)
            self.same(j, what + " (enqueued, compared at frame %d)" % i, got, want)
        self.pending = []

    def frame(self, i, step, m, rest, o):
        g = self.g
        self.census["frames"] += 1
        if not step["sync"]:
            c, s = self.buffer(m.W * m.H * 4), self.buffer(m.SD * m.SD * 4)
            g.copy_frame_async(c.data_ptr(), s.data_ptr())
            self.pending += [(i, "copy_frame_async colour", c, o.color()), (i, "copy_frame_async shadow map", s, o.shadowmap().view(np.uint32).copy())]
            return
        self.flush(i)
        self.same(i, "shadow map", g.shadowmap().view(np.uint32), o.shadowmap().view(np.uint32))
        for t, name in enumerate(TARGET_NAMES):
            self.same(i, "GBuffer " + name, g.gbuffer(t), o.gbuffer(t))
        self.same(i, "colour", g.color(), o.color())
        if g.stats()["overflow"] != 0:
            self.fail(i, "overflow %r" % (g.stats(),))
        t = g.pass_times(1)
        kept2 = t["hiz"] == 0.0 and t["gbuffer2"] == 0.0
        self.census["camera_kept" if _whole(t) else "round2_kept" if kept2 else "drawn"] += 1
        depth, sun, light = rest
        if self.default and depth >= 3 and not m.forward:
            self.census["keep_asserted"] += 1
            if not _whole(t):
                self.fail(i, "rest depth %d and the camera pass was not kept: %r" % (depth, t))
            if depth >= 4 and sun >= 4 and light >= 1 and m.n_point <= sm.REST_ARG_LIGHTS:
                self.census["read_asserted"] += 1
                if g.light_keep()["last"] != "read":
                    self.fail(i, "a second resting frame with standing lights did not read the plane: %r" % (g.light_keep(),))
        self.last_ok = i

    # ---- readers
    def reader(self, i, step, reader, m, o):
        g, kind = self.g, reader[0]
        s = sm.reader_scale(reader)
        if kind in ("raycast", "raycast_async"):
            rays = self.rays(reader, m)
            want = sm.expect(reader, m, o, self.engine, rays)
            if kind == "raycast":
                self.same(i, kind, g.raycast(rays), want)
            else:
                r, h = self.up(rays), self.buffer(want.nbytes)
                g.raycast_async(r.data_ptr(), h.data_ptr(), len(rays))
                self.pending.append((i, kind, h, want))
            return
        want = sm.expect(reader, m, o)
        if kind == "color_scaled":
            self.same(i, "%s %d" % (kind, s), g.color_scaled(s), want)
        elif kind == "copy_frame_scaled_async":
            b = self.buffer(want.nbytes)
            g.copy_frame_scaled_async(s, b.data_ptr())
            self.pending.append((i, "%s %d" % (kind, s), b, want))
        elif kind == "color_highlighted":
            self.same(i, "%s %d" % (kind, s), g.color_highlighted(s), want)
        elif kind == "read_color_overlaid":
            self.same(i, "%s %d" % (kind, s), g.read_color_overlaid(s, False), want)
        elif kind in ("read_frame_delta", "read_frame_delta_packed"):
            tiles, pixels, full, f = want
            if self.client_of is not m.client:               # (a new client: enabled, reset, rescaled or resized)
                self.client_of, self.gclient = m.client, np.zeros_like(m.client)
            if kind == "read_frame_delta":
                gt, gp, head = g.read_frame_delta()
                self.same(i, kind + " tiles", gt, tiles)
                self.same(i, kind + " pixels", gp, pixels)
                sm.fdr.apply(self.gclient, gt, gp)
            else:
                gt, offsets, stream, head = g.read_frame_delta_packed()
                self.same(i, kind + " tiles", gt, tiles)
                self.engine.frame_delta_decode(gt, offsets, stream, self.gclient)
            if (head["n_tiles"], head["full"]) != (len(tiles), int(full)):
                self.fail(i, "%s header %r, expected %d tiles, full %d" % (kind, head, len(tiles), full))
            self.same(i, kind + ": the client's copy", self.gclient, f)
        elif kind == "read_ids":
            self.same(i, kind, g.read_ids(abi.IDS_OBJECT), want)
        elif kind == "instance_coverage":
            self.same(i, kind, g.instance_coverage(), want)
        elif kind == "instance_coverage_async":
            b = self.buffer(want.nbytes)
            g.instance_coverage_async(b.data_ptr(), len(want))
            self.pending.append((i, kind, b, want))
        elif kind == "pick":
            rect = sm.pick_rect(reader, o.visibility())
            hits, total = g.pick(*rect)
            got = [(int(h["object"]), int(h["instance"]), int(h["pixels"]), int(h["triangle"]), int(h["x"]), int(h["y"]), float(h["depth"])) for h in hits]
            if (got, total) != want:
                self.fail(i, "pick%r: %r, expected %r" % (rect, (got, total), want))
        else:
            raise ValueError(kind)
        if step["sync"] and not self.pending:
            self.last_ok = i

    def end(self, m):
        self.g.finish()
        self.flush(len(self.steps))


def play(seed, steps, oracle_lib, gpu_engine, upto=None):
    """the session of `seed` (its starting state and flavour) over `steps` -> the census of the regimes it saw"""
    flags, sky = sm.flavour(seed)
    m0 = sm.Model(seed)
    g = gpu_engine.Renderer(m0.W, m0.H, m0.SD, flags=flags)
    g.set_timing_interval(1)
    p = Player(seed, steps, g, gpu_engine, flags, sky)
    try:
        sm.run(steps, upto, seed=seed, oracle_lib=oracle_lib, renderer=g, hooks=p)
        k = g.light_keep()
        p.census.update(plane_filled=k["filled"], plane_read=k["read"], read_by_argument=k["read_by_arg"])
        p.census["parts_settled"] = "%d of %d" % g.rest_settled()[::-1] if k["read_by_arg"] else "-"
    finally:
        g.close()
    return p.census


@pytest.mark.parametrize("seed", range(BASE, BASE + SEEDS))
def test_session(oracle_lib, gpu_engine, seed):
    t0 = time.time()
    census = play(seed, sm.script(seed), oracle_lib, gpu_engine)
    print("seed %d flavour %r: %s; %.2f s" % (seed, sm.flavour(seed), ", ".join("%s %s" % kv for kv in census.items()), time.time() - t0))
