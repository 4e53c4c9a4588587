"""Delivering changes without a GPU: the numpy statement of a delivery (tests/frame_delta_reference.py) holds its own rules, and the C-ABI
carries the four entry points and the 16-byte header in the public header, the ctypes binding and the built library alike."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_delta_reference as fdr
from zeldaengine_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(33, 17), (257, 131), (410, 150)]
ENTRY_POINTS = ("zr_set_frame_delta", "zr_frame_delta_reset", "zr_read_frame_delta", "zr_copy_frame_delta_async")


def _frames(W, H, seed):
    """a random frame, and the same with a few scattered pixels changed in one byte (most tiles stay equal)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    b = a.copy()
    for x, y in ((0, 0), (W - 1, H - 1), (W // 2, H // 2), (min(32, W - 1), 0)):
        b[y, x, int(rng.integers(0, 4))] ^= 0x10
    return a, b


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_reference_round_trips(W, H):
    a, b = _frames(W, H, W)
    nx, ny = fdr.tile_grid(W, H)
    tiles, pixels = fdr.delta(np.zeros_like(a), a, full=True)
    assert tiles.tolist() == list(range(nx * ny)) and pixels.shape == (nx * ny, 32, 32, 4)
    assert np.array_equal(fdr.untile(tiles, pixels, W, H), a)
    client = a.copy()
    tiles, pixels = fdr.delta(a, b)
    assert 0 < len(tiles) <= 4                                 # (four pixels were touched)
    assert np.array_equal(fdr.apply(client, tiles, pixels), b)
    none, _ = fdr.delta(b, b)
    assert len(none) == 0
    # a delivery straight from a stale copy (frames skipped over) still lands on the frame
    c, _ = _frames(W, H, W + 1)
    assert np.array_equal(fdr.apply(c.copy(), *fdr.delta(c, b)), b)


@pytest.mark.parametrize("W,H", SHAPES)
def test_edge_slots_are_padded_with_zero_and_the_list_ascends(W, H):
    a, _ = _frames(W, H, 7 * W)
    a[a == 0] = 1                                              # so that a zero in a slot can only be padding
    tiles, pixels = fdr.delta(np.zeros_like(a), a, full=True)
    assert (np.diff(tiles.astype(np.int64)) > 0).all()
    assert fdr.padding_is_zero(tiles, pixels, W, H)
    nx, ny = fdr.tile_grid(W, H)
    last = pixels[-1]
    h, w = H - (ny - 1) * 32, W - (nx - 1) * 32
    assert last[:h, :w].all() and int((last != 0).any(axis=2).sum()) == h * w
    # one byte of one pixel: exactly that pixel's tile
    b = a.copy(); b[H - 1, W - 1, 3] ^= 1
    assert fdr.delta(a, b)[0].tolist() == [nx * ny - 1]


def test_the_four_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert hasattr(L, name), name
        assert name in abi.FRAME_DELTA_SIGNATURES and getattr(L, name).argtypes == abi.FRAME_DELTA_SIGNATURES[name]
    for m in ("set_frame_delta", "frame_delta_reset", "read_frame_delta", "copy_frame_delta_async"):
        assert callable(getattr(engine.Renderer, m))


def test_header_binding_and_library_agree_on_the_version():
    """The entry points are additive (no struct of an older host changed), and the suite pins ZR_ABI_VERSION at 7 in four places: the number
    stays, and the three places that carry it agree."""
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == abi.ABI_VERSION == engine.lib().zr_abi_version()


def test_the_delivery_header_is_16_bytes_as_c_and_as_ctypes(tmp_path):
    assert C.sizeof(abi.FrameDelta) == 16
    assert [n for n, _ in abi.FrameDelta._fields_] == ["n_tiles", "total_tiles", "full", "serial"]
    src = tmp_path / "t.c"
    src.write_text('#include "zelda_render.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu", sizeof(zr_frame_delta), offsetof(zr_frame_delta, n_tiles), '
                   'offsetof(zr_frame_delta, total_tiles), offsetof(zr_frame_delta, full), offsetof(zr_frame_delta, serial));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["16", "0", "4", "8", "12"]
    assert abi.TILE_BYTES == 4096
