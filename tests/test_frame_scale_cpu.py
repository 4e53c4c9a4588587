"""Delivering a scaled frame without a GPU: the table of csrc/zr_scale.h is the float64 formula's, the library's host statement of the
filter (zr_frame_downscale, context-free host code) equals the numpy statement (tests/frame_scale_reference.py) byte for byte - random
images at the edge shapes and every scale, constant images, the identity, every threshold's tie block and the block just below it - a
stand-alone program runs the shared header under the sanitizers from and into exactly-sized heap buffers, and the C-ABI carries the six
entry points in the public header, the ctypes binding and the built library alike."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_scale_reference as fsr
from zeldaengine_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
SHAPES = [(1, 1), (7, 5), (33, 17), (66, 34), (257, 131)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
ENTRY_POINTS = ("zr_frame_scaled_extent", "zr_frame_downscale", "zr_read_color_scaled", "zr_copy_frame_scaled_async", "zr_set_frame_delta_scale",
                "zr_get_frame_delta_extent")


def _random(W, H, seed=0):
    return np.random.default_rng(1000 * W + H + seed).integers(0, 256, size=(H, W, 4), dtype=np.uint8)


# ---- the table

def _header_table():
    text = open(os.path.join(CSRC, "zr_scale.h")).read()
    body = text.split("#define ZR_SCALE_TABLE_LITERALS", 1)[1].split("\n\n", 1)[0]
    return np.array([int(v) for v in re.findall(r"\d+", body)], dtype=np.int64)


def test_the_headers_literals_are_the_float64_formulas():
    got = _header_table()
    assert got.shape == (256,) and np.array_equal(got, fsr.table())
    assert got[:6].tolist() == [0, 20, 40, 60, 80, 99] and got[253:].tolist() == [64372, 64952, 65535]


def test_the_table_ascends_and_no_entry_is_near_a_rounding_tie():
    t = fsr.table()
    assert (np.diff(t) > 0).all() and int(np.diff(t).min()) == 19
    x = fsr.table_real()
    assert float(np.abs((x - np.floor(x)) - 0.5).min()) > 1e-3


def test_every_intermediate_is_below_two_to_the_24():
    assert 2 * 64 * int(fsr.T[255]) == 8388480 < 1 << 24 and int(fsr.MID.max()) * 64 == 8351168 < 1 << 24


# ---- zr_frame_downscale against the reference

@pytest.mark.parametrize("s", fsr.SCALES)
@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_random_images_equal_the_reference(W, H, s):
    img = _random(W, H)
    got = engine.frame_downscale(img, s)
    want = fsr.downscale(img, s)
    assert got.shape == want.shape == (-(-H // s), -(-W // s), 4)
    assert np.array_equal(got, want), "first difference at %s" % (np.argwhere(got != want)[0].tolist(),)


def test_constant_images_return_themselves():
    for c in range(256):
        img = np.full((5, 7, 4), c, dtype=np.uint8)
        for s in fsr.SCALES:
            out = engine.frame_downscale(img, s)
            assert (out == c).all(), (c, s)
            assert np.array_equal(out, fsr.downscale(img, s))


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
def test_scale_1_is_the_identity(W, H):
    img = _random(W, H, seed=1)
    assert np.array_equal(engine.frame_downscale(img, 1), img) and np.array_equal(fsr.downscale(img, 1), img)


def test_every_thresholds_tie_block_goes_upward():
    """{k - 1, k - 1, k, k} sits exactly on threshold k and yields k, in colour and in alpha"""
    for k in range(1, 256):
        blk = fsr.tie_block(k)
        assert 2 * int(fsr.T[blk[:, :, 0]].sum()) == int(fsr.MID[k - 1]) * 4
        out = engine.frame_downscale(blk, 2)
        assert out.shape == (1, 1, 4) and out.reshape(4).tolist() == [k] * 4, (k, out.tolist())
        assert np.array_equal(fsr.downscale(blk, 2), out)


def test_just_below_the_tie_is_what_the_sums_say():
    """the tie block with one pixel lowered by one: the expected byte is the reference's, never the library's"""
    below = 0
    for k in range(1, 256):
        for y, x in ((0, 0), (1, 1)):
            blk = fsr.tie_block(k)
            if blk[y, x, 0] == 0:
                continue
            blk[y, x] -= 1
            want = fsr.downscale(blk, 2)
            assert np.array_equal(engine.frame_downscale(blk, 2), want), (k, y, x)
            below += int(want[0, 0, 0] == k - 1)
            assert want[0, 0, 3] == k - 1                      # floor((2 (4 k - 3) + 4) / 8) = floor(k - 1/4)
    assert below == 509                                        # every one of them: the sum fell below threshold k and not below k - 1
    img = fsr.tie_image(66, 34)
    assert np.array_equal(engine.frame_downscale(img, 2), fsr.downscale(img, 2))


# ---- zr_frame_scaled_extent and the refusals of the context-free calls

def test_scaled_extent_and_refusals():
    L = engine.lib()
    for W, H in SHAPES:
        for s in fsr.SCALES:
            assert engine.frame_scaled_extent(W, H, s) == fsr.extent(W, H, s) == (-(-W // s), -(-H // s))
    w, h = C.c_uint32(77), C.c_uint32(77)
    for args in ((33, 17, 0), (33, 17, 9), (0, 17, 2), (33, 0, 2)):
        assert L.zr_frame_scaled_extent(*args, C.byref(w), C.byref(h)) == abi.ERR_ARG
    assert L.zr_frame_scaled_extent(33, 17, 2, None, C.byref(h)) == abi.ERR_ARG
    assert L.zr_frame_scaled_extent(33, 17, 2, C.byref(w), None) == abi.ERR_ARG
    assert (w.value, h.value) == (77, 77)
    img = _random(33, 17)
    out = np.full((9, 17, 4), 0xA5, dtype=np.uint8)
    src, dst = img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.zr_frame_downscale(src, 33, 17, 0, dst, out.nbytes) == abi.ERR_ARG
    assert L.zr_frame_downscale(src, 33, 17, 9, dst, out.nbytes) == abi.ERR_ARG
    assert L.zr_frame_downscale(None, 33, 17, 2, dst, out.nbytes) == abi.ERR_ARG
    assert L.zr_frame_downscale(src, 33, 17, 2, None, out.nbytes) == abi.ERR_ARG
    assert L.zr_frame_downscale(src, 33, 17, 2, dst, out.nbytes - 4) == abi.ERR_ARG
    assert L.zr_frame_downscale(src, 33, 17, 2, dst, out.nbytes + 4) == abi.ERR_ARG
    assert L.zr_frame_downscale(src, 0, 17, 2, dst, out.nbytes) == abi.ERR_ARG
    assert (out == 0xA5).all(), "a refused call wrote into the destination"
    assert L.zr_frame_downscale(src, 33, 17, 2, dst, out.nbytes) == 0 and np.array_equal(out, fsr.downscale(img, 2))
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.frame_downscale(img, 9)
    assert e.value.code == abi.ERR_ARG


# ---- the shared header as a stand-alone program under the sanitizers

def test_the_shared_header_under_the_sanitizers(tmp_path):
    """tests/frame_scale_check.cpp includes csrc/zr_scale.h alone and is compiled with g++, under the address and undefined-behaviour
    sanitizers where this machine links them for a stand-alone program (as tests/test_frame_delta_codec_cpu.py does), and run on the CPU:
    the edge shapes at every scale, from and into exactly-sized heap buffers; its digests are the reference's."""
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hello = tmp_path / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp_path / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp_path / "hello")]) == 0):
        sanitize = []
    exe = tmp_path / "frame_scale_check"
    subprocess.check_call(["g++"] + flags + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "frame_scale_check.cpp"), "-o", str(exe)])
    cases = [(_random(W, H, seed=2), s) for W, H in SHAPES for s in fsr.SCALES]
    cases += [(fsr.tie_image(66, 34), 2), (fsr.tie_image(33, 17, shift=100), 2), (np.full((5, 7, 4), 255, dtype=np.uint8), 8)]
    blob = [np.array([len(cases)], dtype="<u4").tobytes()]
    for img, s in cases:
        blob += [np.array([img.shape[1], img.shape[0], s], dtype="<u4").tobytes(), img.tobytes()]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    run = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "cases %d failed 0" % len(cases) and len(lines) == len(cases) + 1
    for line, (img, s) in zip(lines, cases):
        row = dict(w.split("=") for w in line.split()[2:])
        want = fsr.downscale(img, s)
        assert (int(row["wd"]), int(row["hd"])) == (want.shape[1], want.shape[0])
        assert int(row["fnv"], 16) == fsr.digest(want), line


# ---- the C-ABI

def test_the_six_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert hasattr(L, name), name
        assert name in abi.FRAME_SCALE_SIGNATURES and getattr(L, name).argtypes == abi.FRAME_SCALE_SIGNATURES[name]
    for m in ("color_scaled", "copy_frame_scaled_async", "set_frame_delta_scale", "frame_delta_extent"):
        assert callable(getattr(engine.Renderer, m))
    assert callable(engine.frame_downscale) and callable(engine.frame_scaled_extent)


def test_header_binding_and_library_agree_on_the_version():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == abi.ABI_VERSION == engine.lib().zr_abi_version()
