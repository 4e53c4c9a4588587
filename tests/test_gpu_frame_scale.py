"""Delivering a scaled frame on the renderer (zr_read_color_scaled, zr_copy_frame_scaled_async, zr_set_frame_delta_scale,
zr_get_frame_delta_extent).

Every scaled frame is held, byte for byte, to tests/frame_scale_reference.py applied to zr_read_color's frame, and every delivery of a
scaled frame's changes to tests/frame_delta_reference.py applied to two such scaled frames.  Scene, cameras and the client's bookkeeping
are those of tests/test_gpu_frame_delta.py.  The shapes are the smallest at which the kernel (zr_scale.hip: k_frame_scale) can go wrong:
7 x 5 (at scale 8 the whole frame is one partial block of 35 pixels), 33 x 17 (W % 4 == 1; one-pixel-wide and one-pixel-high edge blocks at
scales 2, 4, 8), 66 x 34 (scaled to 33 x 17: Wd % 4 == 1 on the store side), 410 x 150 (W % 4 == 2), 257 x 131, and 192 x 128 (everything
aligned: the 16-byte loads and the arms compiled for scales 2 and 4); and, because a workgroup takes at most 1 024 frame columns of an
output row, 1100 x 9 and 1101 x 5: at every scale a row is split between two workgroups, on the aligned and on the pixel-by-pixel path.  Synthetic frames written over the finished frame put the kernel's
own input domain under it: random bytes, every threshold's tie block, constant levels.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import frame_delta_reference as fdr
import frame_scale_reference as fsr
import test_gpu_frame_delta as raw
import test_gpu_frame_delta_packed as pk
from independent_scenes import _lights
from zeldaengine_amd import abi, build as zbuild

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5), (33, 17), (66, 34), (410, 150), (257, 131), (192, 128), (1100, 9), (1101, 5)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
DELTA_CASES = [(257, 131, 2), (257, 131, 3), (66, 34, 2), (66, 34, 3)]
DELTA_IDS = ["%dx%d-s%d" % c for c in DELTA_CASES]
SENTINEL8 = raw.SENTINEL8
GUARD = 64                               # sentinel bytes behind a device destination


@pytest.fixture(scope="module")
def lights():
    return _lights(1, 4)


class _Host(pk._Host):
    """tests/test_gpu_frame_delta_packed.py's host and client, delivering at a delta scale: the client copy has the scaled extent"""

    def __init__(self, engine, lights, W, H, scale=None, mode=0):
        super().__init__(engine, lights, W, H, mode=0)
        if scale is not None:
            self.r.set_frame_delta_scale(scale)
        self.Wd, self.Hd, self.total, self.scale = self.r.frame_delta_extent()
        self.client = np.zeros((self.Hd, self.Wd, 4), dtype=np.uint8)
        if mode:
            self.r.set_frame_delta(mode)

    def scaled(self):
        """what the client must hold: the reference's filter of zr_read_color's frame"""
        return fsr.downscale(self.r.color(), self.scale)

    def deliver_packed_scaled(self):
        """one packed host-form delivery into sentinel buffers, applied to the client copy by the library's decoder -> (tiles, header)"""
        tiles = np.full(self.total, raw.SENTINEL32, dtype=np.uint32)
        offsets = np.full(self.total + 1, raw.SENTINEL32, dtype=np.uint32)
        stream = np.full(self.total * abi.RECORD_MAX_BYTES, SENTINEL8, dtype=np.uint8)
        t, o, s, h = self.r.read_frame_delta_packed(tiles, offsets, stream)
        n = h["n_tiles"]
        assert (tiles[n:] == raw.SENTINEL32).all() and (offsets[n + 1:] == raw.SENTINEL32).all() and (stream[h["bytes"]:] == SENTINEL8).all()
        self.engine.frame_delta_decode(t, o, s, self.client)
        return t.copy(), h

    def deliver_form(self, form):
        """one delivery through form 0 raw host, 1 raw device, 2 packed host, 3 packed device, applied to the client -> (tiles, header)"""
        if form == 0:
            t, _, h = self.deliver()
        elif form == 1:
            s = raw._DeviceSet(self.total)
            s.enqueue(self.r)
            self.r.finish()
            t, px, h = s.read()
            fdr.apply(self.client, t, px)
        elif form == 2:
            t, h = self.deliver_packed_scaled()
        else:
            s = pk._DeviceSet(self.total)
            s.enqueue(self.r)
            self.r.finish()
            t, o, st, h = s.read()
            self.engine.frame_delta_decode(t, o, st, self.client)
        assert h["total_tiles"] == self.total
        return np.asarray(t).copy(), h


class _Dest:
    """a device destination for zr_copy_frame_scaled_async: `offset` bytes into a sentinel-filled torch allocation, GUARD bytes behind it"""

    def __init__(self, Wd, Hd, offset=0):
        import torch
        self.n, self.offset, self.shape = Wd * Hd * 4, offset, (Hd, Wd, 4)
        self.buf = torch.full((offset + self.n + GUARD,), SENTINEL8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def ptr(self):
        return self.buf.data_ptr() + self.offset

    def read(self):
        """after a finish(): the scaled frame; every byte ahead of and behind it must still be the sentinel"""
        b = self.buf.cpu().numpy()
        assert (b[:self.offset] == SENTINEL8).all() and (b[self.offset + self.n:] == SENTINEL8).all(), "written outside the Wd*Hd*4 bytes"
        return b[self.offset:self.offset + self.n].reshape(self.shape).copy()


def _both_forms(h, frame, scales=fsr.SCALES):
    """the host form and the device form at every scale against the reference's filter of `frame`; the device destination is offset by 4
    bytes at every other scale, so it is not 16-byte aligned"""
    for s in scales:
        want = fsr.downscale(frame, s)
        got = h.r.color_scaled(s)
        assert got.shape == want.shape and np.array_equal(got, want), "host form, scale %d: first difference at %s" % (s, np.argwhere(got != want)[:1].tolist())
        d = _Dest(want.shape[1], want.shape[0], offset=4 * (s % 2))
        assert d.ptr() % 16 == 4 * (s % 2)
        h.r.copy_frame_scaled_async(s, d.ptr())
        h.r.finish()
        got = d.read()
        assert np.array_equal(got, want), "device form, scale %d: first difference at %s" % (s, np.argwhere(got != want)[:1].tolist())


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_rendered_frames_at_every_scale(gpu_engine, lights, W, H):
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame()
        c = h.r.color()
        assert np.array_equal(h.r.color_scaled(1), c)
        _both_forms(h, c)
        h.frame(cam=1)                       # another frame: the buffer made at first use is used again
        c1 = h.r.color()
        _both_forms(h, c1, scales=(2, 3))
        assert np.array_equal(h.r.color(), c1)
    finally:
        h.close()


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_synthetic_frames_over_the_kernels_own_input_domain(gpu_engine, lights, W, H):
    """independent of what the renderer draws: the finished frame overwritten in place with random bytes, with the 255 tie blocks tiled
    across it (every threshold on its tie at scale 2, and sums of tie blocks at the other scales), and with constant levels"""
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame()
        h.r.finish()
        rng = np.random.default_rng(W * 1000 + H)
        images = [rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8), fsr.tie_image(W, H), fsr.tie_image(W, H, shift=128)]
        for frame in images:
            h.put_frame(frame)
            assert np.array_equal(h.r.color(), frame)
            _both_forms(h, frame)
        for level in (0, 1, 127, 255):
            frame = np.full((H, W, 4), level, dtype=np.uint8)
            h.put_frame(frame)
            for s in fsr.SCALES:
                got = h.r.color_scaled(s)
                assert (got == level).all() and got.shape == fsr.downscale(frame, s).shape, (level, s)
        _both_forms(h, frame, scales=(2, 4, 7))
    finally:
        h.close()


def test_device_form_four_frames_in_flight(gpu_engine, lights):
    """four frames in a row, an instance moved between them, each filtered into its own buffer (scales 2, 3, 4, 2) with no host
    synchronisation in between: every buffer equals the reference's filter of that frame rendered alone"""
    W, H = 257, 131
    scales = (2, 3, 4, 2)
    h = _Host(gpu_engine, lights, W, H)
    try:
        was, alone = None, []
        for k, s in enumerate(scales):       # each frame alone, read back
            if k:
                rec = h.move(0, 0.3)
                was = rec if was is None else was
            h.frame()
            alone.append(fsr.downscale(h.r.color(), s))
        h.put(0, was)
        assert not np.array_equal(alone[0], alone[3])
        dests = []
        for k, s in enumerate(scales):       # the same four in flight
            if k:
                h.move(0, 0.3)
            h.frame()
            dests.append(_Dest(alone[k].shape[1], alone[k].shape[0], offset=4 * (k % 2)))
            h.r.copy_frame_scaled_async(s, dests[-1].ptr())
        h.r.finish()
        for k, d in enumerate(dests):
            assert np.array_equal(d.read(), alone[k]), "frame %d of four in flight differs from the same frame rendered alone" % k
    finally:
        h.close()


def _move_that_lists_some_tiles(h, a):
    """moves an instance so that the REFERENCE lists more than zero and at most half of the scaled frame's tiles (a frame of one tile: that
    one) against the scaled frame `a` -> (instance, its record as it was, the scaled frame after the move, the reference's delivery)"""
    most = max(1, h.total // 2)
    for inst in (0, 7, 5, 1, 2, 3):
        was = h.move(inst)
        h.frame()
        b = h.scaled()
        want = fdr.delta(a, b)
        if 0 < len(want[0]) <= most:
            return inst, was, b, want
        h.put(inst, was)
    raise AssertionError("no candidate instance makes the reference list between 1 and %d of %d tiles" % (most, h.total))


@pytest.mark.parametrize("W,H,s", DELTA_CASES, ids=DELTA_IDS)
def test_deltas_of_the_scaled_frame_in_the_four_forms(gpu_engine, lights, W, H, s):
    """the first delivery is full and untiles to the scaled frame; a rest delivers nothing; a moved instance delivers exactly the
    reference's delta of the two scaled frames, in the raw host and device forms and, through frame_delta_decode, in the packed ones"""
    h = _Host(gpu_engine, lights, W, H, scale=s, mode=abi.FRAME_DELTA_PACKED)
    try:
        Wd, Hd = fsr.extent(W, H, s)
        nx, ny = fdr.tile_grid(Wd, Hd)
        assert h.r.frame_delta_extent() == (Wd, Hd, nx * ny, s) and h.total == nx * ny == h.r.frame_delta_tiles()
        h.frame()
        tiles, pixels, hd = h.deliver()
        a = h.scaled()
        assert hd == {"n_tiles": h.total, "total_tiles": h.total, "full": 1, "serial": 1}
        assert np.array_equal(fdr.untile(tiles, pixels, Wd, Hd), a) and fdr.padding_is_zero(tiles, pixels, Wd, Hd)
        assert raw._same(tiles, pixels, fdr.delta(np.zeros_like(a), a, full=True))
        h.frame()                            # rest
        assert h.deliver()[2] == {"n_tiles": 0, "total_tiles": h.total, "full": 0, "serial": 2}
        inst, was, b, want = _move_that_lists_some_tiles(h, a)
        tiles, pixels, hd = h.deliver()      # raw host form
        assert hd == {"n_tiles": len(want[0]), "total_tiles": h.total, "full": 0, "serial": 3}
        assert raw._same(tiles, pixels, want) and fdr.padding_is_zero(tiles, pixels, Wd, Hd) and np.array_equal(h.client, b)
        frames = (a, b)
        for step, form in enumerate((1, 2, 3)):      # back and forth between the two frames: raw device, packed host, packed device
            if step % 2 == 0:
                h.put(inst, was)
            else:
                h.move(inst)
            h.frame()
            cur, prev = frames[step % 2], frames[(step + 1) % 2]
            assert np.array_equal(h.scaled(), cur)
            want = fdr.delta(prev, cur)
            if form == 1:
                dev = raw._DeviceSet(h.total)
                dev.enqueue(h.r)
                h.r.finish()
                tiles, pixels, hd = dev.read()
                assert raw._same(tiles, pixels, want)
                fdr.apply(h.client, tiles, pixels)
            else:
                tiles, hd = h.deliver_form(form)
            assert np.array_equal(tiles, want[0]) and 0 < len(tiles) <= max(1, h.total // 2)
            assert (hd["n_tiles"], hd["total_tiles"], hd["full"], hd["serial"]) == (len(want[0]), h.total, 0, 4 + step)
            assert np.array_equal(h.client, cur), "form %d: the client copy differs from the scaled frame" % form
    finally:
        h.close()


@pytest.mark.parametrize("W,H,s", DELTA_CASES, ids=DELTA_IDS)
def test_an_eight_step_sequence_keeps_the_client_at_the_scaled_frame(gpu_engine, lights, W, H, s):
    h = _Host(gpu_engine, lights, W, H, scale=s, mode=abi.FRAME_DELTA_PACKED)
    try:
        steps = [("cam", 0), ("rest", 0), ("inst", 0), ("cam", 1), ("rest", 1), ("inst", 5), ("inst", 0), ("cam", 0)]
        cam, counts = 0, []
        for f, (what, arg) in enumerate(steps):
            if what == "cam":
                cam = arg
            elif what == "inst":
                h.move(arg, 0.3)
            h.frame(cam)
            tiles, hd = h.deliver_form(f % 4)
            assert hd["serial"] == f + 1 and hd["full"] == (1 if f == 0 else 0)
            assert (np.diff(tiles.astype(np.int64)) > 0).all()
            assert np.array_equal(h.client, h.scaled()), "step %d (%s): the client copy differs from the scaled frame" % (f, what)
            counts.append(hd["n_tiles"])
        assert counts[0] == h.total and counts[1] == 0 and counts[4] == 0 and counts[3] > 0 and counts[7] > 0
    finally:
        h.close()


def test_refusals_change_nothing(gpu_engine, lights):
    W, H = 66, 34
    E = gpu_engine.ZeldaRenderError
    L = gpu_engine.lib()

    def refused(code, call, *args):
        with pytest.raises(E) as e:
            call(*args)
        assert e.value.code == code, e.value

    h = _Host(gpu_engine, lights, W, H)
    try:
        r = h.r
        dest = _Dest(33, 17)
        out = np.full((17, 33, 4), SENTINEL8, dtype=np.uint8)
        # before the first frame
        refused(abi.ERR_STATE, r.color_scaled, 2)
        refused(abi.ERR_STATE, r.copy_frame_scaled_async, 2, dest.ptr())
        h.frame()
        a = r.color()
        # arguments
        for s in (0, 9):
            refused(abi.ERR_ARG, r.color_scaled, s)
            refused(abi.ERR_ARG, r.copy_frame_scaled_async, s, dest.ptr())
            refused(abi.ERR_ARG, r.set_frame_delta_scale, s)
        refused(abi.ERR_ARG, r.copy_frame_scaled_async, 2, None)
        refused(abi.ERR_ARG, r.copy_frame_scaled_async, 2, dest.ptr() + 2)
        assert L.zr_read_color_scaled(r.h, 2, None, out.nbytes) == abi.ERR_ARG
        assert L.zr_read_color_scaled(r.h, 2, gpu_engine._ptr(out), out.nbytes - 4) == abi.ERR_ARG
        assert L.zr_read_color_scaled(r.h, 2, gpu_engine._ptr(out), W * H * 4) == abi.ERR_ARG
        assert L.zr_get_frame_delta_extent(r.h, None, None, None, None) == abi.ERR_ARG
        assert (out == SENTINEL8).all()
        # between the stages of a frame
        d, p, sp = lights
        r.update_uniforms(raw._cam(0), d, p, sp, 0.0, 0.0, 0.0)
        r.render_shadow()
        refused(abi.ERR_STATE, r.color_scaled, 2)
        refused(abi.ERR_STATE, r.copy_frame_scaled_async, 2, dest.ptr())
        r.render_gbuffer(); r.render_lighting()
        r.finish()
        assert (dest.read() == SENTINEL8).all(), "a refused call wrote into the destination"
        assert np.array_equal(r.color(), a) and np.array_equal(r.color_scaled(2), fsr.downscale(a, 2))
        # the delta scale: only while delta is off; kept across the switch; the extent answers on and off
        assert r.frame_delta_extent() == (66, 34, 6, 1)
        r.set_frame_delta_scale(2)
        assert r.frame_delta_extent() == (33, 17, 2, 2)
        r.set_frame_delta(True)
        refused(abi.ERR_STATE, r.set_frame_delta_scale, 3)
        assert r.frame_delta_extent() == (33, 17, 2, 2)
        h.total, h.client = 2, np.zeros((17, 33, 4), dtype=np.uint8)
        refused(abi.ERR_ARG, r.read_frame_delta, np.zeros(6, dtype=np.uint32), np.zeros((6, 32, 32, 4), dtype=np.uint8))      # (the frame's own tile count)
        tiles, pixels, hd = h.deliver()
        assert hd == {"n_tiles": 2, "total_tiles": 2, "full": 1, "serial": 1} and np.array_equal(h.client, fsr.downscale(a, 2))
        r.set_frame_delta(False)
        assert r.frame_delta_extent() == (33, 17, 2, 2)
        r.set_frame_delta_scale(3)
        assert r.frame_delta_extent() == (22, 12, 1, 3)
    finally:
        h.close()
    # contexts whose lighting pass does not write the row-major frame
    dest = _Dest(33, 17)
    for kw in ({"flags": abi.FLAG_PACKED_TILES}, {"tile_rank": 0, "tile_world": 2}):
        r = gpu_engine.Renderer(W, H, 256, **kw)
        try:
            refused(abi.ERR_UNSUPPORTED, r.color_scaled, 2)
            refused(abi.ERR_UNSUPPORTED, r.copy_frame_scaled_async, 2, dest.ptr())
        finally:
            r.close()


def test_native_headless_driver_delivers_scaled(gpu_engine, tmp_path):
    """tools/zelda_headless --scale 2: read with zr_read_color_scaled, and delivered through --delta and --delta-packed at delta scale 2
    into a client copy kept by the C++ driver; the three PPMs are the reference's filter of the PPM of the run without --scale"""
    import test_gpu_native_host as nh
    root = str(tmp_path)
    nh._content_tree(root)
    exe = zbuild.build_headless()
    Wd, Hd = fsr.extent(nh.W, nh.H, 2)
    total = fdr.tile_grid(Wd, Hd)[0] * fdr.tile_grid(Wd, Hd)[1]
    frames = {}
    for mode, extra in (("plain", []), ("scaled", ["--scale", "2"]), ("delta", ["--delta", "--scale", "2"]), ("packed", ["--delta-packed", "--scale", "2"])):
        ppm = os.path.join(root, mode + ".ppm")
        cmd = [exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (nh.W, nh.H), "--shadow", str(nh.SD), "--frames", "3", "--out", ppm]
        out = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text
        frames[mode] = open(ppm, "rb").read()
        if mode == "scaled":
            assert re.findall(r"^scaled (\d+)x(\d+)$", text, re.M) == [(str(Wd), str(Hd))] * 3, text
        elif mode == "delta":
            assert re.findall(r"^delta (\d+)/(\d+)$", text, re.M) == [(str(total), str(total))] + [("0", str(total))] * 2, text
        elif mode == "packed":
            assert [m[:2] for m in re.findall(r"^delta-packed (\d+)/(\d+) tiles (\d+) bytes", text, re.M)] == [(str(total), str(total))] + [("0", str(total))] * 2, text
    header = ("P6\n%d %d\n255\n" % (nh.W, nh.H)).encode()
    assert frames["plain"].startswith(header)
    rgb = np.frombuffer(frames["plain"][len(header):], dtype=np.uint8).reshape(nh.H, nh.W, 3)
    rgba = np.concatenate([rgb, np.full((nh.H, nh.W, 1), 255, dtype=np.uint8)], axis=2)
    want = ("P6\n%d %d\n255\n" % (Wd, Hd)).encode() + fsr.downscale(rgba, 2)[:, :, :3].tobytes()
    for mode in ("scaled", "delta", "packed"):
        assert frames[mode] == want, mode
    out = subprocess.run([exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (nh.W, nh.H), "--shadow", str(nh.SD), "--scale", "9"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 1 and b"--scale 1..8" in out.stdout


def test_delta_scale_1_is_the_delivery_of_the_frame_itself(gpu_engine, lights, monkeypatch):
    """a context whose delta scale was set to 1 explicitly delivers byte for byte what tests/test_gpu_frame_delta.py expects: one of its
    sequences run unchanged through its _Host"""
    class Scale1(raw._Host):
        def __init__(self, engine, lights, W, H, delta=True, flags=0):
            super().__init__(engine, lights, W, H, delta=False, flags=flags)
            self.r.set_frame_delta_scale(1)
            assert self.r.frame_delta_extent() == (W, H, self.total, 1)
            if delta:
                self.r.set_frame_delta(True)

    monkeypatch.setattr(raw, "_Host", Scale1)
    raw.test_first_delivery_rest_and_one_moved_instance(gpu_engine, lights, 257, 131)
    raw.test_a_sequence_of_frames_through_both_forms(gpu_engine, lights)
