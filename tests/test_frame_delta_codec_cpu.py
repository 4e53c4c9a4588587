"""The tile codec of the packed delivery without a GPU: the numpy statement of the format (tests/frame_delta_codec_reference.py) holds its
own rules - round trips at every width, the sizes the format promises, zero padding at a frame's edge - the library's decoder
(zr_frame_delta_decode: host code, context-free) reads what the reference writes and refuses what is malformed without writing, a
stand-alone program runs the decoder's header under the sanitizers over valid, truncated and mutated streams, and the C-ABI carries the
entry points and the 32-byte header in the public header, the ctypes binding and the built library alike."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_delta_codec_reference as cr
import frame_delta_reference as fdr
from zeldaengine_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
SHAPES = [(33, 17), (257, 131), (410, 150)]
ENTRY_POINTS = ("zr_read_frame_delta_packed", "zr_copy_frame_delta_packed_async", "zr_frame_delta_decode")
SENTINEL = 0xA5


def _round_trip(tile):
    rec = cr.encode_tile(tile)
    back, mode = cr.decode_record(rec)
    assert np.array_equal(back, tile)
    assert len(rec) % 8 == 0 and len(rec) <= cr.RAW_BYTES
    return rec, mode


@pytest.mark.parametrize("b", range(9))
def test_every_width_round_trips(b):
    rng = np.random.default_rng(b)
    for _ in range(3):
        rec, mode = _round_trip(cr.tile_of_widths(rng, b))
        if 40 + 8 * 64 * b <= cr.RAW_BYTES:
            assert mode == cr.MODE_CODED and len(rec) == 40 + 8 * 64 * b
        else:                                                  # width 8 everywhere: 4 136 bytes coded, so it goes raw
            assert mode == cr.MODE_RAW and len(rec) == cr.RAW_BYTES
    mixed = [int(v) for v in rng.integers(0, b + 1, size=64)]
    rec, mode = _round_trip(cr.tile_of_widths(rng, mixed))
    assert mode == cr.MODE_CODED and len(rec) == 40 + 8 * sum(mixed)
    nib = np.frombuffer(rec, dtype=np.uint8, count=32, offset=8)
    assert [int(n & 15) for n in nib] == mixed[0::2] and [int(n >> 4) for n in nib] == mixed[1::2]


def test_the_sizes_the_format_promises():
    rng = np.random.default_rng(99)
    rec, mode = _round_trip(cr.tile_of_kind(rng, "constant"))
    assert (len(rec), mode) == (40, cr.MODE_CODED)
    rec, mode = _round_trip(cr.tile_of_kind(rng, "sum508"))
    assert (len(rec), mode) == (4104, cr.MODE_CODED)
    tile = cr.tile_of_kind(rng, "sum509")
    rec, mode = _round_trip(tile)
    assert (len(rec), mode) == (4104, cr.MODE_RAW) and rec[8:] == tile.tobytes() and rec[:4] == tile[0, 0].tobytes()
    rec, mode = _round_trip(cr.tile_of_kind(rng, "random"))
    assert (len(rec), mode) == (4104, cr.MODE_RAW)
    # one record, spelled out: a tile of one colour but for pixel (1, 0), whose red is one more - residual 1 there (z = 2) and 255 at
    # pixel (2, 0) (z = 1): group 0 (block 0, red) is two bits wide, every other group 0
    tile = np.full((32, 32, 4), 7, dtype=np.uint8)
    tile[0, 1, 0] = 8
    rec = cr.encode_tile(tile)
    assert rec[:8] == bytes([7, 7, 7, 7, 7, 0, 0, 0])          # pixel (0, 0); (40 + 2 * 8) / 8 words; coded
    assert rec[8] == 2 and not any(rec[9:40])
    assert rec[40:48] == (0b100).to_bytes(8, "little")         # bit 0 of every value: value 2 has it
    assert rec[48:56] == (0b010).to_bytes(8, "little")         # bit 1: value 1
    assert len(rec) == 56


@pytest.mark.parametrize("W,H", SHAPES)
def test_edge_tiles_round_trip_with_zero_padding(W, H):
    nx, ny = fdr.tile_grid(W, H)
    for step in range(cr.synthetic_steps(W, H)):
        frame = cr.synthetic_frame(W, H, step)
        frame[frame == 0] = 1                                  # so that a zero in a decoded tile can only be padding
        for t in sorted({nx - 1, nx * ny - nx, nx * ny - 1}):
            tile = fdr.tile_pixels(frame, t)
            h, w = min(32, H - t // nx * 32), min(32, W - t % nx * 32)
            back, _ = cr.decode_record(cr.encode_tile(tile))
            assert np.array_equal(back, tile) and back[:h, :w].all() and not back[h:].any() and not back[:, w:].any()
        tiles, offsets, stream, _ = cr.delta(np.zeros_like(frame), frame, full=True)
        assert offsets[0] == 0 and offsets[-1] == len(stream) and len(offsets) == nx * ny + 1 and (offsets % 8 == 0).all()
        assert np.array_equal(cr.apply(np.zeros_like(frame), tiles, offsets, stream), frame)


def _deliveries(W, H):
    """[(tiles, offsets, stream, frame)]: every synthetic frame in full, and the last against the one before (which lists every tile too)
    cut down to every other listed tile"""
    out = []
    steps = cr.synthetic_steps(W, H)
    for step in range(steps):
        frame = cr.synthetic_frame(W, H, step)
        out.append(cr.delta(np.zeros_like(frame), frame, full=True)[:3] + (frame,))
    tiles = out[-1][0][::2]
    out.append((tiles,) + cr.encode_stream(out[-1][3], tiles)[:2] + (out[-1][3],))
    return out


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_library_decodes_what_the_reference_encodes(W, H):
    nx, _ = fdr.tile_grid(W, H)
    kinds = set()
    for tiles, offsets, stream, frame in _deliveries(W, H):
        client = np.full_like(frame, SENTINEL)
        assert engine.frame_delta_decode(tiles, offsets, stream, client) is client
        listed = np.zeros((H, W), dtype=bool)
        for t in tiles.tolist():
            listed[t // nx * 32:t // nx * 32 + 32, t % nx * 32:t % nx * 32 + 32] = True
        assert np.array_equal(client[listed], frame[listed]) and (client[~listed] == SENTINEL).all()
        kinds |= {stream[int(o) + 6] for o in offsets[:-1]}
    assert kinds == ({cr.MODE_CODED, cr.MODE_RAW} if H >= 64 else {cr.MODE_CODED})      # (half a tile of noise still codes shorter than raw)
    # an empty delivery is one
    client = np.full((H, W, 4), SENTINEL, dtype=np.uint8)
    engine.frame_delta_decode(np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint8), client)
    assert (client == SENTINEL).all()


def _refused(tiles, offsets, stream, W, H):
    client = np.full((H, W, 4), SENTINEL, dtype=np.uint8)
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.frame_delta_decode(tiles, offsets, stream, client)
    assert e.value.code == abi.ERR_PARSE
    assert (client == SENTINEL).all(), "a refused delivery wrote into the client copy"
    with pytest.raises(cr.Malformed):                          # the reference refuses the same
        cr.apply(client.copy(), tiles, offsets, stream)


def test_malformed_deliveries_are_refused_and_write_nothing():
    W, H = 257, 131
    nx, ny = fdr.tile_grid(W, H)
    frame = cr.synthetic_frame(W, H, 0)
    tiles, offsets, stream, raw = cr.delta(np.zeros_like(frame), frame, full=True)
    assert raw > 0
    engine.frame_delta_decode(tiles, offsets, stream, np.zeros_like(frame))      # (it is a good one to begin with)
    coded = next(k for k in range(len(tiles)) if stream[offsets[k] + 6] == cr.MODE_CODED and offsets[k + 1] - offsets[k] > 48)
    rawk = next(k for k in range(len(tiles)) if stream[offsets[k] + 6] == cr.MODE_RAW)

    def changed(what, k, value):
        t, o, s = tiles.copy(), offsets.copy(), stream.copy()
        {"tile": t, "offset": o, "byte": s}[what][k] = value
        return t, o, s

    # the list: an index beyond the frame, one repeated, one out of order
    _refused(*changed("tile", len(tiles) - 1, nx * ny), W, H)
    _refused(*changed("tile", 3, 2), W, H)
    _refused(*changed("tile", 3, 5), W, H)
    # the offsets: not from 0, not ascending, past the stream
    _refused(*changed("offset", 0, 8), W, H)
    _refused(*changed("offset", 2, int(offsets[1])), W, H)
    _refused(*changed("offset", 2, int(offsets[3]) + 8), W, H)
    _refused(tiles, offsets, stream[:-8], W, H)
    _refused(*changed("offset", len(tiles), len(stream) + 8), W, H)
    # a record's length word against its offsets (a record boundary moved by one word, both length words left alone)
    _refused(*changed("offset", coded + 1, int(offsets[coded + 1]) - 8), W, H)
    _refused(*changed("byte", int(offsets[coded]) + 4, int(stream[offsets[coded] + 4]) ^ 1), W, H)
    _refused(*changed("byte", int(offsets[rawk]) + 4, 0), W, H)
    # ... and against 40 + 8 * sum(b): one width one more or one less
    nib = int(offsets[coded]) + 8
    at = next(a for a in range(nib, nib + 32) if 0 < (stream[a] & 15) < 8)
    _refused(*changed("byte", at, int(stream[at]) + 1), W, H)
    _refused(*changed("byte", at, int(stream[at]) - 1), W, H)
    # a width above 8, with the length made to agree: the record is one word longer on paper and the next one starts later
    t, o, s = tiles[:coded + 1].copy(), offsets[:coded + 2].copy(), stream[:offsets[coded + 1]].copy()
    engine.frame_delta_decode(t, o, s, np.zeros_like(frame))
    more = 9 - int(s[nib] & 15)                                # group 0's width becomes 9: `more` words more
    words = int(s[offsets[coded] + 4]) + 256 * int(s[offsets[coded] + 5]) + more
    assert words * 8 <= cr.RAW_BYTES
    s = np.concatenate([s, np.zeros(8 * more, np.uint8)])
    s[nib] = (s[nib] & 0xF0) | 9; s[offsets[coded] + 4] = words & 255; s[offsets[coded] + 5] = words >> 8; o[-1] += 8 * more
    _refused(t, o, s, W, H)
    # an unknown mode
    _refused(*changed("byte", int(offsets[coded]) + 6, 2), W, H)
    _refused(*changed("byte", int(offsets[rawk]) + 7, 1), W, H)
    # a coded record that says it is raw, a raw one that says it is coded
    _refused(*changed("byte", int(offsets[coded]) + 6, 1), W, H)
    _refused(*changed("byte", int(offsets[rawk]) + 6, 0), W, H)


def test_the_decoder_header_under_the_sanitizers(tmp_path):
    """tests/frame_delta_codec_check.cpp includes csrc/zr_delta_codec.h alone and is compiled with g++, under the address and
    undefined-behaviour sanitizers where this machine links them for a stand-alone program (as tests/test_frame_plan.py does), and run on
    the CPU over reference-encoded deliveries: valid, truncated, and with every byte of a record's header mutated."""
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hello = tmp_path / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp_path / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp_path / "hello")]) == 0):
        sanitize = []
    exe = tmp_path / "frame_delta_codec_check"
    subprocess.check_call(["g++"] + flags + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "frame_delta_codec_check.cpp"), "-o", str(exe)])
    cases = _deliveries(33, 17)[-2:] + _deliveries(64, 64)[::3] + _deliveries(257, 131)[-2:] + _deliveries(410, 150)[-1:]
    cases.append((np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(0, np.uint8), np.zeros((17, 33, 4), np.uint8)))
    blob = [np.array([len(cases)], dtype="<u4").tobytes()]
    for tiles, offsets, stream, frame in cases:
        H, W = frame.shape[:2]
        blob += [np.array([W, H, len(tiles), len(stream)], dtype="<u4").tobytes(), tiles.astype("<u4").tobytes(), offsets.astype("<u4").tobytes(),
                 stream.tobytes() + bytes(-len(stream) % 4), frame.tobytes()]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    run = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    rows = [dict(w.split("=") for w in line.split()[2:]) for line in run.stdout.splitlines() if line.startswith("case ")]
    assert len(rows) == len(cases) and run.stdout.splitlines()[-1] == "cases %d failed 0" % len(cases)
    for row, (tiles, _, _, _) in zip(rows, cases):
        assert row["valid"] == "1" and row["broken"] == "0" and int(row["n"]) == len(tiles)
        assert row["truncated"] == row["truncated_refused"] and row["length"] == row["length_refused"]
        if len(tiles):
            assert int(row["truncated"]) >= 6 and int(row["refused"]) >= int(row["applied"]) > 0 and int(row["length"]) >= 16


def test_the_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert hasattr(L, name), name
        assert name in abi.FRAME_DELTA_SIGNATURES and getattr(L, name).argtypes == abi.FRAME_DELTA_SIGNATURES[name]
    for m in ("read_frame_delta_packed", "copy_frame_delta_packed_async"):
        assert callable(getattr(engine.Renderer, m))
    assert callable(engine.frame_delta_decode)
    assert "#define ZR_FRAME_DELTA_PACKED 3" in hdr and abi.FRAME_DELTA_PACKED == 3
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == 7 == abi.ABI_VERSION == L.zr_abi_version()


def test_the_packed_header_is_32_bytes_as_c_and_as_ctypes(tmp_path):
    assert C.sizeof(abi.FrameDeltaPacked) == 32
    assert [n for n, _ in abi.FrameDeltaPacked._fields_] == ["n_tiles", "total_tiles", "full", "serial", "bytes", "raw_tiles", "reserved"]
    src = tmp_path / "t.c"
    src.write_text('#include "zelda_render.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %u", sizeof(zr_frame_delta_packed), offsetof(zr_frame_delta_packed, serial), '
                   'offsetof(zr_frame_delta_packed, bytes), offsetof(zr_frame_delta_packed, raw_tiles), offsetof(zr_frame_delta_packed, reserved), '
                   'ZR_FRAME_DELTA_RECORD_MAX);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["32", "12", "16", "20", "24", "4104"]
    assert abi.RECORD_MAX_BYTES == 4104 == cr.RAW_BYTES
