"""The packed delivery on the renderer (zr_set_frame_delta(ctx, ZR_FRAME_DELTA_PACKED), zr_read_frame_delta_packed,
zr_copy_frame_delta_packed_async, zr_frame_delta_decode).

Every delivery - list, offsets, stream and header - is held byte for byte to tests/frame_delta_codec_reference.py applied to zr_read_color's
frame and the copy delivered so far; the buffers start as a sentinel so that "nothing behind the written part is touched" is checked too.
Scene, cameras and the client's bookkeeping are those of tests/test_gpu_frame_delta.py.  The shapes: 64 x 64 (whole tiles), 33 x 17
(W % 4 == 1, a one-pixel-wide and 17-pixel-high edge tile), 257 x 131 and 410 x 150 (W % 4 == 2): the smallest at which the edge guards
and both load paths of the kernels (zr_delta.hip: k_delta_measure, k_delta_encode) can go wrong.  Synthetic frames written over the
finished frame put every width 0..8, the longest coded record, the shortest raw one, noise and one colour under the device encoder.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_delta_codec_reference as cr
import frame_delta_reference as fdr
import test_gpu_frame_delta as raw
from independent_scenes import _lights
from zeldaengine_amd import abi, build as zbuild

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (33, 17), (257, 131), (410, 150)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
SENTINEL32, SENTINEL8 = raw.SENTINEL32, raw.SENTINEL8
PACKED = abi.FRAME_DELTA_PACKED


@pytest.fixture(scope="module")
def lights():
    return _lights(1, 4)


class _Host(raw._Host):
    """tests/test_gpu_frame_delta.py's host and client, with the packed host form beside the raw one"""

    def __init__(self, engine, lights, W, H, mode=PACKED):
        super().__init__(engine, lights, W, H, delta=False)
        self.engine = engine
        self.delivered = np.zeros((H, W, 4), dtype=np.uint8)      # what the library's delivered copy must hold (the reference's side)
        if mode:
            self.r.set_frame_delta(mode)

    def deliver_packed(self, want_full=False):
        """one packed host-form delivery into sentinel buffers, held to the reference's encoding of zr_read_color's frame against what
        was delivered so far, and applied to the client copy by the library's decoder -> (tiles, offsets, stream, header)"""
        tiles = np.full(self.total, SENTINEL32, dtype=np.uint32)
        offsets = np.full(self.total + 1, SENTINEL32, dtype=np.uint32)
        stream = np.full(self.total * abi.RECORD_MAX_BYTES, SENTINEL8, dtype=np.uint8)
        t, o, s, h = self.r.read_frame_delta_packed(tiles, offsets, stream)
        n = h["n_tiles"]
        assert h["total_tiles"] == self.total and len(t) == n and len(o) == n + 1 and len(s) == h["bytes"]
        assert (tiles[n:] == SENTINEL32).all() and (offsets[n + 1:] == SENTINEL32).all() and (stream[h["bytes"]:] == SENTINEL8).all(), \
            "written beyond the first n_tiles entries, n_tiles + 1 offsets or `bytes` bytes"
        self.check(t, o, s, h, want_full)
        return t.copy(), o.copy(), s.copy(), h

    def check(self, t, o, s, h, want_full=False):
        frame = self.r.color()
        wt, wo, ws, wraw = cr.delta(self.delivered, frame, full=want_full)
        assert np.array_equal(t, wt), "the list: %s, the reference's %s" % (t.tolist(), wt.tolist())
        assert np.array_equal(o, wo), "the offsets differ from the reference's"
        assert (h["n_tiles"], h["bytes"], h["raw_tiles"], h["full"]) == (len(wt), len(ws), wraw, 1 if want_full else 0), (h, len(wt), len(ws), wraw)
        bad = np.flatnonzero(s != ws)
        assert len(bad) == 0, "the stream differs from the reference's at byte %d (record %d)" % (bad[0], int(np.searchsorted(wo, bad[0], "right")) - 1)
        self.engine.frame_delta_decode(t, o, s, self.client)
        assert np.array_equal(self.client, frame), "the decoded client copy differs from zr_read_color"
        self.delivered = frame

    def put_frame(self, frame):
        """overwrite the finished frame on the device (the way tests/test_gpu_frame_delta.py overwrites a pixel)"""
        hip = raw._hip()
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        assert frame.shape == (self.H, self.W, 4)
        assert hip.hipMemcpy(C.c_void_p(self.r.color_device_ptr()), frame.ctypes.data_as(C.c_void_p), frame.nbytes, 1) == 0
        assert hip.hipDeviceSynchronize() == 0


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_rendered_frames_first_rest_instance_camera(gpu_engine, lights, W, H):
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame()
        tiles, offsets, stream, hd = h.deliver_packed(want_full=True)
        assert hd["serial"] == 1 and tiles.tolist() == list(range(h.total))
        assert hd["bytes"] < h.total * 4096, "a rendered frame that does not shrink at all"
        h.frame()                                              # rest
        _, offsets, _, hd = h.deliver_packed()
        assert (hd["n_tiles"], hd["bytes"], hd["raw_tiles"], hd["serial"]) == (0, 0, 0, 2) and offsets.tolist() == [0]
        h.move(0)                                              # one instance moved
        h.frame()
        _, _, _, hd = h.deliver_packed()
        assert hd["serial"] == 3 and (hd["n_tiles"] > 0 or W < 64)
        h.frame(cam=1)                                         # the camera moved
        _, _, _, hd = h.deliver_packed()
        assert hd["serial"] == 4 and hd["n_tiles"] > 0
    finally:
        h.close()


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_synthetic_frames_every_width_and_both_modes(gpu_engine, lights, W, H):
    """frames made of tiles of every kind (frame_delta_codec_reference.KINDS), each delivered against the one before: the device encoder
    meets every width, the longest coded and the shortest raw record, noise and one colour; raw_tiles is the reference's count"""
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame()
        h.deliver_packed(want_full=True)
        seen_widths, seen_lengths, raw_tiles = set(), set(), 0
        for step in range(cr.synthetic_steps(W, H)):
            frame = cr.synthetic_frame(W, H, step)
            h.put_frame(frame)
            tiles, offsets, stream, hd = h.deliver_packed()
            assert hd["n_tiles"] == h.total                    # (every tile is of another kind than before)
            raw_tiles += hd["raw_tiles"]
            for k in range(len(tiles)):
                rec = stream[offsets[k]:offsets[k + 1]]
                seen_lengths.add((len(rec), int(rec[6])))
                if rec[6] == cr.MODE_CODED:
                    seen_widths |= {int(v) for v in rec[8:40] & 15} | {int(v) for v in rec[8:40] >> 4}
        assert seen_widths == set(range(9))
        if W >= 64 and H >= 64:                                # whole tiles: the kinds arrive uncut
            assert {(4104, cr.MODE_CODED), (4104, cr.MODE_RAW)} <= seen_lengths and raw_tiles >= 3
            assert {(40 + 512 * b, cr.MODE_CODED) for b in range(8)} <= seen_lengths
    finally:
        h.close()


class _DeviceSet:
    """header, list, offsets and stream on the device, as torch tensors filled with the sentinel"""

    def __init__(self, total):
        import torch
        self.header = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.tiles = torch.full((total,), SENTINEL32 - (1 << 32), dtype=torch.int32, device="cuda")
        self.offsets = torch.full((total + 1,), SENTINEL32 - (1 << 32), dtype=torch.int32, device="cuda")
        self.stream = torch.full((total * abi.RECORD_MAX_BYTES,), SENTINEL8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def enqueue(self, r):
        r.copy_frame_delta_packed_async(self.header.data_ptr(), self.tiles.data_ptr(), self.offsets.data_ptr(), self.stream.data_ptr())

    def read(self):
        """after a finish(): (tiles, offsets, stream, header dict); what lies behind the written part must still be the sentinel"""
        hd = self.header.cpu().numpy().view(np.uint32)
        tiles, offsets, stream = self.tiles.cpu().numpy().view(np.uint32), self.offsets.cpu().numpy().view(np.uint32), self.stream.cpu().numpy()
        n, nbytes = int(hd[0]), int(hd[4])
        assert hd[6] == 0 and hd[7] == 0
        assert (tiles[n:] == SENTINEL32).all() and (offsets[n + 1:] == SENTINEL32).all() and (stream[nbytes:] == SENTINEL8).all(), \
            "written beyond the first n_tiles entries, n_tiles + 1 offsets or `bytes` bytes"
        return tiles[:n], offsets[:n + 1], stream[:nbytes], {"n_tiles": n, "total_tiles": int(hd[1]), "full": int(hd[2]), "serial": int(hd[3]),
                                                             "bytes": nbytes, "raw_tiles": int(hd[5])}


def _equals(got, want):
    """(tiles, offsets, stream, header) against the reference's (tiles, offsets, stream, raw_tiles)"""
    t, o, s, h = got
    return (np.array_equal(t, want[0]) and np.array_equal(o, want[1]) and np.array_equal(s, want[2]) and
            (h["n_tiles"], h["bytes"], h["raw_tiles"]) == (len(want[0]), len(want[2]), want[3]))


def test_device_form_two_frames_in_flight(gpu_engine, lights):
    """render, deliver into set 0, render moved, deliver into set 1, ONE finish: both sets equal the reference's, nothing behind their
    written parts is touched, and set 0 is not disturbed by the second frame"""
    W, H = 257, 131
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame(); a = h.r.color()
        was = h.move(0); h.frame(); b = h.r.color()
        h.put(0, was)
        assert not np.array_equal(a, b)
        sets = [_DeviceSet(h.total), _DeviceSet(h.total)]
        h.frame(); sets[0].enqueue(h.r)
        h.move(0); h.frame(); sets[1].enqueue(h.r)
        h.r.finish()
        got0, got1 = sets[0].read(), sets[1].read()
        assert np.array_equal(h.r.color(), b)
        assert (got0[3]["full"], got0[3]["serial"], got0[3]["total_tiles"]) == (1, 1, h.total)
        assert _equals(got0, cr.delta(np.zeros_like(a), a, full=True))
        want = cr.delta(a, b)
        assert (got1[3]["full"], got1[3]["serial"]) == (0, 2) and 0 < len(want[0]) < h.total
        assert _equals(got1, want)
        client = np.zeros_like(a)
        for t, o, s, _ in (got0, got1):
            gpu_engine.frame_delta_decode(t, o, s, client)
        assert np.array_equal(client, b)
    finally:
        h.close()


def test_the_four_forms_mixed_in_one_sequence(gpu_engine, lights):
    """8 frames delivered in turn through the raw host form, the packed host form, the raw device form and the packed device form: they
    share the delivered copy, the client copy equals zr_read_color after every delivery, and serial counts through all of them"""
    W, H = 410, 150
    h = _Host(gpu_engine, lights, W, H)
    try:
        steps = [("cam", 0), ("inst", 0), ("cam", 1), ("rest", 1), ("inst", 5), ("inst", 0), ("cam", 0), ("rest", 0)]
        cam = 0
        for f, (what, arg) in enumerate(steps):
            if what == "cam":
                cam = arg
            elif what == "inst":
                h.move(arg, 0.3)
            h.frame(cam)
            form = f % 4
            if form == 0:
                tiles, pixels, hd = h.deliver()                # (applies to the client copy itself)
                h.delivered = h.r.color()
            elif form == 1:
                tiles, _, _, hd = h.deliver_packed(want_full=(f == 0))
            elif form == 2:
                s = raw._DeviceSet(h.total)
                s.enqueue(h.r)
                h.r.finish()
                tiles, pixels, hd = s.read()
                fdr.apply(h.client, tiles, pixels)
                h.delivered = h.r.color()
            else:
                s = _DeviceSet(h.total)
                s.enqueue(h.r)
                h.r.finish()
                tiles, offsets, stream, hd = s.read()
                h.check(tiles, offsets, stream, hd)
            assert hd["serial"] == f + 1 and hd["full"] == (1 if f == 0 else 0) and hd["total_tiles"] == h.total
            assert np.array_equal(h.client, h.r.color()), "frame %d (%s, form %d): the client copy differs from zr_read_color" % (f, what, form)
            assert hd["n_tiles"] == 0 if what == "rest" else hd["n_tiles"] > 0 or what == "inst", (f, what, hd)
    finally:
        h.close()


def test_state_switching_and_refusals(gpu_engine, lights):
    W, H = 257, 131
    E = gpu_engine.ZeldaRenderError
    h = _Host(gpu_engine, lights, W, H, mode=1)
    dev = _DeviceSet(h.total)

    def refused(code, call, *args):
        with pytest.raises(E) as e:
            call(*args)
        assert e.value.code == code, e.value

    try:
        r = h.r
        h.frame()
        # raw delivery only: the packed forms are refused, the raw ones work
        refused(abi.ERR_STATE, r.read_frame_delta_packed)
        refused(abi.ERR_STATE, dev.enqueue, r)
        _, _, hd = h.deliver()
        assert (hd["full"], hd["serial"], hd["n_tiles"]) == (1, 1, h.total)
        h.delivered = r.color()
        # 1 -> 3 keeps the delivered copy, full and serial: the next delivery is not a full one
        r.set_frame_delta(PACKED)
        r.set_frame_delta(PACKED)                              # (already there: nothing changes)
        _, _, _, hd = h.deliver_packed()
        assert (hd["n_tiles"], hd["full"], hd["serial"]) == (0, 0, 2)
        h.move(0); h.frame()
        _, _, _, hd = h.deliver_packed()
        assert hd["n_tiles"] > 0 and hd["serial"] == 3
        # buffers of another size, a stream that is not 16-byte aligned
        total = h.total
        good = [np.zeros(total, np.uint32), np.zeros(total + 1, np.uint32), np.zeros(total * abi.RECORD_MAX_BYTES, np.uint8)]
        for k, short in enumerate((np.zeros(total - 1, np.uint32), np.zeros(total, np.uint32), np.zeros(total * 4096, np.uint8))):
            refused(abi.ERR_ARG, r.read_frame_delta_packed, *(good[:k] + [short] + good[k + 1:]))
        refused(abi.ERR_ARG, r.copy_frame_delta_packed_async, dev.header.data_ptr(), dev.tiles.data_ptr(), dev.offsets.data_ptr(), dev.stream.data_ptr() + 8)
        refused(abi.ERR_ARG, r.copy_frame_delta_packed_async, dev.header.data_ptr(), dev.tiles.data_ptr(), 0, dev.stream.data_ptr())
        # between the stages of a frame
        d, p, sp = lights
        r.update_uniforms(raw._cam(0), d, p, sp, 0.0, 0.0, 0.0)
        r.render_shadow()
        refused(abi.ERR_STATE, r.read_frame_delta_packed)
        refused(abi.ERR_STATE, dev.enqueue, r)
        refused(abi.ERR_STATE, r.set_frame_delta, 1)
        r.render_gbuffer(); r.render_lighting()
        _, _, _, hd = h.deliver_packed()
        assert (hd["n_tiles"], hd["serial"]) == (0, 4)
        # 3 -> 1 keeps them too; the packed forms are refused again
        h.move(0); h.frame()
        r.set_frame_delta(1)
        refused(abi.ERR_STATE, r.read_frame_delta_packed)
        tiles, pixels, hd = h.deliver()
        want = fdr.delta(h.delivered, r.color())
        assert (hd["full"], hd["serial"]) == (0, 5) and 0 < hd["n_tiles"] < h.total and raw._same(tiles, pixels, want)
        # a new client through the packed form; off and on again starts over
        r.set_frame_delta(PACKED)
        r.frame_delta_reset()
        h.client[:] = 0
        h.delivered = np.zeros_like(h.delivered)
        _, _, _, hd = h.deliver_packed(want_full=True)
        assert (hd["n_tiles"], hd["serial"]) == (h.total, 6)
        r.set_frame_delta(False)
        refused(abi.ERR_STATE, r.read_frame_delta_packed)
        refused(abi.ERR_STATE, r.read_frame_delta)
        r.set_frame_delta(PACKED)
        h.delivered = np.zeros_like(h.delivered)
        _, _, _, hd = h.deliver_packed(want_full=True)
        assert hd["serial"] == 1
    finally:
        h.close()
    # before the first frame
    r = gpu_engine.Renderer(W, H, 256)
    try:
        r.set_frame_delta(PACKED)
        refused(abi.ERR_STATE, r.read_frame_delta_packed)
        refused(abi.ERR_STATE, dev.enqueue, r)
    finally:
        r.close()


def test_nothing_else_moves(gpu_engine, lights):
    """colour, the six GBuffer planes, the shadow map and zr_stats of a three-frame sequence are the same with packed delivery on (and a
    delivery after every frame), with raw delivery on and with none; the raw context's deliveries are what they were - the reference's
    list and slots - beside a packed context"""
    W, H = 257, 131
    on, plain, off = _Host(gpu_engine, lights, W, H), _Host(gpu_engine, lights, W, H, mode=1), _Host(gpu_engine, lights, W, H, mode=0)
    try:
        before = np.zeros((H, W, 4), dtype=np.uint8)
        for f, (cam, inst) in enumerate([(0, None), (1, None), (1, 0)]):
            for h in (on, plain, off):
                if inst is not None:
                    h.move(inst)
                h.frame(cam)
            on.deliver_packed(want_full=(f == 0))
            tiles, pixels, hd = plain.deliver()
            planes = [[h.r.color()] + [h.r.gbuffer(t).copy() for t in range(6)] + [h.r.shadowmap().view(np.uint32).copy()] for h in (on, plain, off)]
            for k, (x, y, z) in enumerate(zip(*planes)):
                assert np.array_equal(x.view(np.uint8), z.view(np.uint8)) and np.array_equal(y.view(np.uint8), z.view(np.uint8)), \
                    "frame %d: plane %d differs with delivery on" % (f, k)
            assert on.r.stats() == off.r.stats() == plain.r.stats()
            assert raw._same(tiles, pixels, fdr.delta(before, planes[2][0], full=(f == 0))) and hd["serial"] == f + 1
            assert np.array_equal(on.client, planes[2][0]) and np.array_equal(plain.client, planes[2][0])
            before = planes[2][0]
    finally:
        on.close(); plain.close(); off.close()


def test_native_headless_driver_delivers_packed(gpu_engine, tmp_path):
    """tools/zelda_headless --delta-packed: every frame leaves through zr_read_frame_delta_packed and is decoded by zr_frame_delta_decode
    into the client copy kept by the C++ driver; its PPM is the one --delta writes, and bytes per frame are printed"""
    import test_gpu_native_host as nh
    root = str(tmp_path)
    nh._content_tree(root)
    exe = zbuild.build_headless()
    frames = {}
    total = fdr.tile_grid(nh.W, nh.H)[0] * fdr.tile_grid(nh.W, nh.H)[1]
    for mode in ("delta", "delta-packed"):
        ppm = os.path.join(root, mode + ".ppm")
        cmd = [exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (nh.W, nh.H), "--shadow", str(nh.SD), "--frames", "4", "--out", ppm,
               "--" + mode]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text
        frames[mode] = open(ppm, "rb").read()
        if mode == "delta-packed":
            rows = re.findall(r"^delta-packed (\d+)/(\d+) tiles (\d+) bytes \((\d+) raw\)$", text, re.M)
            assert [r[:2] for r in rows] == [(str(total), str(total))] + [("0", str(total))] * 3, text
            assert 40 * total <= int(rows[0][2]) < 4096 * total and [r[2] for r in rows[1:]] == ["0"] * 3
    header = ("P6\n%d %d\n255\n" % (nh.W, nh.H)).encode()
    assert frames["delta"].startswith(header) and len(frames["delta"]) == len(header) + nh.W * nh.H * 3
    assert frames["delta-packed"] == frames["delta"]
