"""Delivering changes on the renderer (zr_set_frame_delta, zr_frame_delta_reset, zr_read_frame_delta, zr_copy_frame_delta_async).

Every delivery is held, byte for byte, to tests/frame_delta_reference.py applied to two zr_read_color read-backs; host buffers start as a
sentinel so that "only the first n entries are written" is checked too.  The scene is the 400 spheres of tests/test_gpu_ids.py; the shapes
put one-pixel-wide and three-pixel-high edge tiles, widths that are no multiple of four, and one, two and three mask words under the
kernels (zr_delta.hip).
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import frame_delta_reference as fdr
from independent_scenes import Scene, _lights
from zeldaengine_amd import abi, build as zbuild, scenes

pytestmark = pytest.mark.gpu

SHAPES = [(192, 128), (257, 131), (33, 17), (410, 150), (420, 300)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
SENTINEL32, SENTINEL8 = 0xA5A5A5A5, 0xA5
SPHERES = 1                  # the instanced object's index (add order)


def _spheres():
    """400 instanced spheres over a plane that crosses the near plane (the scene of tests/test_gpu_ids.py)"""
    s = Scene()
    s.add(scenes.grid_plane(40.0, 3, 0.0), [(90, 140, 60, 255), (0, 0, 0, 255), (200, 200, 200, 255), (127, 127, 255, 255),
                                             (255, 255, 255, 255), (0, 0, 0, 255), (255, 255, 255, 255)])
    s.add(scenes.uv_sphere(10, 5, 0.5), None, scenes.generate_instances(400, 0.5, 7.0, 0.3, 0.9, seed=17))
    s.add(scenes.box((0.6, 0.5, 0.7), (0.5, -0.5, 0.7)))
    return s


def _cam(i):
    a = 0.4 + 0.05 * i
    return abi.make_camera((6.0 * math.cos(a), 6.0 * math.sin(a), 1.1 + 0.1 * i), (0.0, 0.0, 0.4), fov=60.0)


@pytest.fixture(scope="module")
def lights():
    return _lights(1, 4)


class _Host:
    """A renderer with the scene loaded, and a client: sentinel-filled host buffers and the copy the deliveries are applied to"""

    def __init__(self, engine, lights, W, H, delta=True, flags=0):
        self.r = engine.Renderer(W, H, 256, flags=flags)
        self.W, self.H, self.lights = W, H, lights
        self.scene = _spheres()
        self.scene.load(self.r)
        self.total = self.r.frame_delta_tiles()
        self.client = np.zeros((H, W, 4), dtype=np.uint8)
        if delta:
            self.r.set_frame_delta(True)

    def frame(self, cam=0):
        d, p, sp = self.lights
        self.r.update_uniforms(_cam(cam), d, p, sp, 0.0, 0.0, 0.0)
        self.r.render()

    def move(self, instance, dx=0.4):
        """-> the instance's record as it was (for put)"""
        _, inst = self.r.object_get_instances(SPHERES)
        one = inst[instance:instance + 1].copy()
        one["InstancePosition"][0][0] += dx
        self.r.object_set_instances(SPHERES, one, first=instance)
        return inst[instance:instance + 1].copy()

    def put(self, instance, record):
        self.r.object_set_instances(SPHERES, record, first=instance)

    def deliver(self):
        """one host-form delivery into sentinel buffers -> (tiles, pixels, header); what lies behind the first n entries must still be
        the sentinel; the delivery is applied to the client copy"""
        tiles = np.full(self.total, SENTINEL32, dtype=np.uint32)
        pixels = np.full((self.total, 32, 32, 4), SENTINEL8, dtype=np.uint8)
        t, px, h = self.r.read_frame_delta(tiles, pixels)
        n = h["n_tiles"]
        assert h["total_tiles"] == self.total and len(t) == n and len(px) == n
        assert (tiles[n:] == SENTINEL32).all() and (pixels[n:] == SENTINEL8).all(), "written beyond the first n_tiles entries"
        fdr.apply(self.client, t, px)
        return t.copy(), px.copy(), h

    def close(self):
        self.r.close()


def _same(got_tiles, got_pixels, want):
    return np.array_equal(got_tiles, want[0]) and np.array_equal(got_pixels, want[1])


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_first_delivery_rest_and_one_moved_instance(gpu_engine, lights, W, H):
    """the first delivery is the whole frame; the same inputs again deliver nothing; a hidden instance moved delivers nothing; instance 0
    moved delivers the reference's tiles of the two read-backs"""
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame()
        tiles, pixels, hd = h.deliver()
        a = h.r.color()
        assert hd == {"n_tiles": h.total, "total_tiles": h.total, "full": 1, "serial": 1}
        assert tiles.tolist() == list(range(h.total))
        assert np.array_equal(fdr.untile(tiles, pixels, W, H), a) and fdr.padding_is_zero(tiles, pixels, W, H)
        assert _same(tiles, pixels, fdr.delta(np.zeros_like(a), a, full=True))
        # rest
        h.frame()
        tiles, _, hd = h.deliver()
        assert hd == {"n_tiles": 0, "total_tiles": h.total, "full": 0, "serial": 2}
        # a hidden instance moved
        h.move(123)
        h.frame()
        assert h.deliver()[2]["n_tiles"] == 0
        assert np.array_equal(h.r.color(), a)
        serial = 3
        if (W, H) == (192, 128):              # a move that changes five pixels of one tile (so the CPU oracle has it)
            h.move(7)
            h.frame()
            tiles, pixels, hd = h.deliver()
            c = h.r.color()
            want = fdr.delta(a, c)
            assert len(want[0]) == 1 and int((a != c).any(axis=2).sum()) == 5
            assert _same(tiles, pixels, want) and np.array_equal(h.client, c)
            a, serial = c, 4
        # instance 0 moved
        h.move(0)
        h.frame()
        tiles, pixels, hd = h.deliver()
        b = h.r.color()
        want = fdr.delta(a, b)
        assert 0 < len(want[0]) <= h.total / 2, "the reference itself lists %d of %d tiles" % (len(want[0]), h.total)
        assert hd == {"n_tiles": len(want[0]), "total_tiles": h.total, "full": 0, "serial": serial + 1}
        assert _same(tiles, pixels, want) and fdr.padding_is_zero(tiles, pixels, W, H)
        assert np.array_equal(h.client, b)
    finally:
        h.close()


def _hip():
    """the HIP runtime this process has already loaded (the library's and torch's one copy)"""
    for line in open("/proc/self/maps"):
        m = re.search(r"(/\S*libamdhip64\.so[^\s]*)", line)
        if m:
            lib = C.CDLL(m.group(1))
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            lib.hipMemcpy.restype = C.c_int
            lib.hipDeviceSynchronize.restype = C.c_int
            return lib
    raise RuntimeError("no HIP runtime is loaded")


@pytest.mark.parametrize("W,H", [(257, 131), (410, 150)], ids=["257x131", "410x150"])
def test_one_byte_of_one_pixel_lists_exactly_its_tile(gpu_engine, lights, W, H):
    """independent of what the renderer draws: one byte of the finished frame overwritten in place, at the corners of tiles and of the
    frame; the old value poked back lists the same tile again"""
    hip = _hip()
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame()
        h.deliver()
        base = h.r.color()
        nx, ny = fdr.tile_grid(W, H)
        spots = [(0, 0), (31, 31), (32, 0), (W - 1, H - 1), ((nx - 1) * 32, (ny - 1) * 32)]
        for k, (x, y) in enumerate(spots):
            t = (y // 32) * nx + x // 32
            poked = base[y, x].copy()
            poked[k % 4] ^= 1 << (k % 8)         # a single byte, another channel and bit at every spot
            for value in (poked, base[y, x]):
                px = np.ascontiguousarray(value, dtype=np.uint8)
                assert hip.hipMemcpy(C.c_void_p(h.r.color_device_ptr() + 4 * (y * W + x)), px.ctypes.data_as(C.c_void_p), 4, 1) == 0
                assert hip.hipDeviceSynchronize() == 0
                tiles, pixels, hd = h.deliver()
                assert tiles.tolist() == [t], "pixel (%d, %d): tiles %s, expected [%d]" % (x, y, tiles.tolist(), t)
                want = base.copy()
                want[y, x] = px
                assert np.array_equal(pixels[0], fdr.tile_pixels(want, t)) and hd["full"] == 0
            assert np.array_equal(h.client, base)
        assert np.array_equal(h.r.color(), base)
    finally:
        h.close()


def test_frames_without_a_delivery_are_skipped_over(gpu_engine, lights):
    W, H = 257, 131
    h = _Host(gpu_engine, lights, W, H)
    try:
        h.frame(0)
        h.deliver()
        h.frame(1)                           # rendered, never delivered
        h.r.finish()
        assert not np.array_equal(h.r.color(), h.client)
        h.frame(0)
        _, _, hd = h.deliver()
        assert hd["n_tiles"] == 0 and hd["serial"] == 2 and np.array_equal(h.r.color(), h.client)
    finally:
        h.close()


class _DeviceSet:
    """header, list and slots on the device, as torch tensors filled with the sentinel"""

    def __init__(self, total):
        import torch
        self.torch = torch
        self.header = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.tiles = torch.full((total,), SENTINEL32 - (1 << 32), dtype=torch.int32, device="cuda")
        self.pixels = torch.full((total, 32, 32, 4), SENTINEL8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def enqueue(self, r):
        r.copy_frame_delta_async(self.header.data_ptr(), self.tiles.data_ptr(), self.pixels.data_ptr())

    def read(self):
        """after a finish(): (tiles, pixels, header dict); entries behind the first n must still be the sentinel"""
        hd = self.header.cpu().numpy().view(np.uint32)
        tiles, pixels = self.tiles.cpu().numpy().view(np.uint32), self.pixels.cpu().numpy()
        n = int(hd[0])
        assert (tiles[n:] == SENTINEL32).all() and (pixels[n:] == SENTINEL8).all(), "written beyond the first n_tiles entries"
        return tiles[:n], pixels[:n], {"n_tiles": n, "total_tiles": int(hd[1]), "full": int(hd[2]), "serial": int(hd[3])}


def test_a_sequence_of_frames_through_both_forms(gpu_engine, lights):
    """8 frames - the camera moves on some, an instance on others, some rest - delivered alternately through the host form and the
    device form: the client copy equals zr_read_color after every delivery, and serial counts up"""
    W, H = 410, 150
    h = _Host(gpu_engine, lights, W, H)
    try:
        steps = [("cam", 0), ("rest", 0), ("inst", 0), ("cam", 1), ("rest", 1), ("inst", 5), ("inst", 0), ("cam", 0)]
        counts = []
        cam = 0
        for f, (what, arg) in enumerate(steps):
            if what == "cam":
                cam = arg
            elif what == "inst":
                h.move(arg, 0.3)
            h.frame(cam)
            if f % 2 == 0:
                tiles, pixels, hd = h.deliver()
            else:
                s = _DeviceSet(h.total)
                s.enqueue(h.r)
                h.r.finish()
                tiles, pixels, hd = s.read()
                fdr.apply(h.client, tiles, pixels)
            assert hd["serial"] == f + 1 and hd["full"] == (1 if f == 0 else 0) and hd["total_tiles"] == h.total
            assert (np.diff(tiles.astype(np.int64)) > 0).all()
            assert np.array_equal(h.client, h.r.color()), "frame %d (%s): the client copy differs from zr_read_color" % (f, what)
            counts.append(hd["n_tiles"])
        assert counts[0] == h.total and counts[1] == 0 and counts[4] == 0 and all(c > 0 for k, c in enumerate(counts) if steps[k][0] == "cam")
    finally:
        h.close()


def test_two_frames_in_flight(gpu_engine, lights):
    """render, deliver into set 0, render moved, deliver into set 1, ONE finish: both sets equal the reference's, and set 0 is not
    disturbed by the second frame's lighting pass"""
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
        t0, p0, h0 = sets[0].read()
        t1, p1, h1 = sets[1].read()
        assert np.array_equal(h.r.color(), b)
        assert h0 == {"n_tiles": h.total, "total_tiles": h.total, "full": 1, "serial": 1}
        assert _same(t0, p0, fdr.delta(np.zeros_like(a), a, full=True))
        want = fdr.delta(a, b)
        assert h1 == {"n_tiles": len(want[0]), "total_tiles": h.total, "full": 0, "serial": 2} and len(want[0]) > 0
        assert _same(t1, p1, want)
    finally:
        h.close()


def test_reset_and_refusals(gpu_engine, lights):
    W, H = 192, 128
    E = gpu_engine.ZeldaRenderError
    h = _Host(gpu_engine, lights, W, H, delta=False)
    dev = _DeviceSet(h.total)

    def refused(code, call, *args):
        with pytest.raises(E) as e:
            call(*args)
        assert e.value.code == code, e.value

    try:
        r = h.r
        # off: every call but the switch is refused
        h.frame()
        refused(abi.ERR_STATE, r.read_frame_delta)
        refused(abi.ERR_STATE, dev.enqueue, r)
        refused(abi.ERR_STATE, r.frame_delta_reset)
        r.finish()
        a = r.color()
        r.set_frame_delta(True)
        r.set_frame_delta(True)              # (already on: nothing changes)
        _, _, hd = h.deliver()
        assert hd["full"] == 1 and hd["serial"] == 1 and np.array_equal(h.client, a)
        assert h.deliver()[2] == {"n_tiles": 0, "total_tiles": h.total, "full": 0, "serial": 2}
        # a new client
        r.frame_delta_reset()
        h.client[:] = 0
        tiles, pixels, hd = h.deliver()
        assert hd == {"n_tiles": h.total, "total_tiles": h.total, "full": 1, "serial": 3} and np.array_equal(h.client, a)
        # buffers of another size
        refused(abi.ERR_ARG, r.read_frame_delta, np.zeros(h.total - 1, dtype=np.uint32), np.zeros((h.total, 32, 32, 4), dtype=np.uint8))
        refused(abi.ERR_ARG, r.read_frame_delta, np.zeros(h.total, dtype=np.uint32), np.zeros((h.total + 1, 32, 32, 4), dtype=np.uint8))
        refused(abi.ERR_ARG, r.copy_frame_delta_async, dev.header.data_ptr(), dev.tiles.data_ptr(), dev.pixels.data_ptr() + 4)
        # between the stages of a frame
        d, p, sp = lights
        r.update_uniforms(_cam(0), d, p, sp, 0.0, 0.0, 0.0)
        r.render_shadow()
        refused(abi.ERR_STATE, r.read_frame_delta)
        refused(abi.ERR_STATE, dev.enqueue, r)
        refused(abi.ERR_STATE, r.set_frame_delta, False)
        r.render_gbuffer(); r.render_lighting()
        assert h.deliver()[2] == {"n_tiles": 0, "total_tiles": h.total, "full": 0, "serial": 4}
        # off and on again starts over
        r.set_frame_delta(False)
        refused(abi.ERR_STATE, r.read_frame_delta)
        r.set_frame_delta(True)
        assert h.deliver()[2] == {"n_tiles": h.total, "total_tiles": h.total, "full": 1, "serial": 1}
    finally:
        h.close()
    # before the first frame; contexts whose lighting pass does not write the row-major frame
    r = gpu_engine.Renderer(W, H, 256)
    try:
        r.set_frame_delta(True)
        refused(abi.ERR_STATE, r.read_frame_delta)
        refused(abi.ERR_STATE, dev.enqueue, r)
    finally:
        r.close()
    for kw in ({"flags": abi.FLAG_PACKED_TILES}, {"tile_rank": 0, "tile_world": 2}):
        r = gpu_engine.Renderer(W, H, 256, **kw)
        try:
            refused(abi.ERR_UNSUPPORTED, r.set_frame_delta, True)
        finally:
            r.close()


def test_nothing_else_moves(gpu_engine, lights):
    """colour, the six GBuffer planes, the shadow map and zr_stats of a three-frame sequence are the same with delta on (and a delivery
    after every frame) and off"""
    W, H = 257, 131
    on, off = _Host(gpu_engine, lights, W, H), _Host(gpu_engine, lights, W, H, delta=False)
    try:
        for f, (cam, inst) in enumerate([(0, None), (1, None), (1, 0)]):
            for h in (on, off):
                if inst is not None:
                    h.move(inst)
                h.frame(cam)
            on.deliver()
            planes = [[h.r.color()] + [h.r.gbuffer(t).copy() for t in range(6)] + [h.r.shadowmap().view(np.uint32).copy()] for h in (on, off)]
            for k, (x, y) in enumerate(zip(*planes)):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "frame %d: plane %d differs with delta on" % (f, k)
            assert on.r.stats() == off.r.stats()
            assert np.array_equal(on.client, planes[1][0])
    finally:
        on.close(); off.close()


def test_native_headless_driver_delivers_through_the_delta(gpu_engine, tmp_path):
    """tools/zelda_headless --delta: every frame leaves through zr_read_frame_delta into a client copy kept by the C++ driver; its PPM is
    written from that copy and equals the run without --delta, and the frames at rest deliver nothing"""
    import test_gpu_native_host as nh
    root = str(tmp_path)
    nh._content_tree(root)
    exe = zbuild.build_headless()
    frames = {}
    for mode in ("plain", "delta"):
        ppm = os.path.join(root, mode + ".ppm")
        cmd = [exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (nh.W, nh.H), "--shadow", str(nh.SD), "--frames", "4", "--out", ppm]
        out = subprocess.run(cmd + (["--delta"] if mode == "delta" else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text
        frames[mode] = open(ppm, "rb").read()
        if mode == "delta":
            total = fdr.tile_grid(nh.W, nh.H)[0] * fdr.tile_grid(nh.W, nh.H)[1]
            assert re.findall(r"^delta (\d+)/(\d+)$", text, re.M) == [(str(total), str(total))] + [("0", str(total))] * 3, text
        else:
            assert "delta " not in text
    header = ("P6\n%d %d\n255\n" % (nh.W, nh.H)).encode()
    assert frames["plain"].startswith(header) and len(frames["plain"]) == len(header) + nh.W * nh.H * 3
    assert frames["delta"] == frames["plain"]
