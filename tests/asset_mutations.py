"""Damaged PNG and OBJ files for the loaders' tests: one generator, drawn from by tests/test_assets.py (in process, through the
library) and tests/test_host_readers_cpu.py (the same readers in a stand-alone program under the sanitizers).  Every draw comes from the
caller's numpy Generator, so a seed names a corpus."""
import struct
import zlib

import numpy as np

OBJ = """# two triangles sharing an edge, a quad face, per-corner uv and normal indices
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 0.25
vn 0 0 1
vn 0 1 0
vn 1 0 0
vn 0.6 0 0.8
f 1/1/4 2/2/4 3/3/4 4/4/4
f 1/5/1 3/3/2 -1/4/3
"""


def write_adam7_rgb(path, rgb):
    """PIL cannot write Adam7: an interlaced 8-bit RGB PNG assembled by hand"""
    h, w, _ = rgb.shape
    raw = b""
    for x0, y0, dx, dy in [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]:
        sub = rgb[y0::dy, x0::dx]
        if sub.size == 0:
            continue
        for row in sub:
            raw += b"\x00" + row.tobytes()

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    return path


def png_fix_crcs(data):
    """recompute every chunk's CRC after a mutation, so that the damage reaches the decoder instead of dying at the checksum"""
    out, pos = bytearray(data[:8]), 8
    while pos + 12 <= len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        if pos + 12 + n > len(data):
            break
        t, d = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        out += data[pos:pos + 8] + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
        pos += 12 + n
    return bytes(out + data[pos:])


def png_seeds(tmp_path, rng):
    """Well-formed files to damage: every colour type the loader reads at 31 x 19, and an interlaced one at 17 x 13."""
    from PIL import Image
    seeds = []
    for mode in ("RGBA", "RGB", "L", "LA", "P", "1"):
        im = Image.fromarray(rng.integers(0, 256, size=(19, 31, 4), dtype=np.uint8), "RGBA")
        im = im.convert("RGB").quantize(16) if mode == "P" else im.convert(mode)
        p = str(tmp_path / ("s_%s.png" % mode)); im.save(p)
        seeds.append(open(p, "rb").read())
    seeds.append(open(write_adam7_rgb(str(tmp_path / "s_a7.png"), rng.integers(0, 256, size=(13, 17, 3), dtype=np.uint8)), "rb").read())
    return seeds


def mutated_png(rng, seeds, k):
    """The k-th damaged file: byte flips, truncations, length / dimension fields blown up, chunks duplicated; CRCs repaired for odd k."""
    data = bytearray(seeds[k % len(seeds)])
    kind = int(rng.integers(0, 5))
    if kind == 0:
        for _ in range(int(rng.integers(1, 6))):
            data[int(rng.integers(8, len(data)))] ^= int(rng.integers(1, 256))
    elif kind == 1:
        data = data[:int(rng.integers(0, len(data)))]
    elif kind == 2:                                            # IHDR fields: width, height, depth, colour type, interlace
        off = 16 + int(rng.integers(0, 13))
        data[off] = int(rng.choice([0, 1, 3, 7, 16, 64, 255]))
    elif kind == 3:                                            # a chunk length blown up
        pos = 8
        lens = []
        while pos + 12 <= len(data):
            lens.append(pos); pos += 12 + struct.unpack(">I", data[pos:pos + 4])[0]
        at = lens[int(rng.integers(0, len(lens)))]
        data[at:at + 4] = struct.pack(">I", int(rng.choice([0, 1, 0x7FFFFFFF, 0xFFFFFFFF, 100000])))
    else:                                                      # IDAT duplicated / IEND moved
        i = bytes(data).find(b"IDAT")
        if i > 4:
            n = struct.unpack(">I", data[i - 4:i])[0]
            data = data[:i + 8 + n] + data[i - 4:i + 8 + n] + data[i + 8 + n:]
    blob = bytes(data)
    if k % 2 and len(blob) > 8:
        blob = png_fix_crcs(blob)
    return blob


def mutated_obj(rng, text):
    """A damaged copy of an OBJ text: numbers replaced by junk, indices out of range / negative / huge, lines cut."""
    lines = text.split("\n")
    for _ in range(int(rng.integers(1, 5))):
        i = int(rng.integers(0, len(lines)))
        toks = lines[i].split(" ")
        if len(toks) > 1:
            j = int(rng.integers(1, len(toks)))
            toks[j] = str(rng.choice(["", "nan", "1e999", "-0", "999999999999", "-7", "1/", "//", "1/2/3/4", "0/0/0", "4294967297/1/1", "x", "1e-400"]))
            lines[i] = " ".join(toks)
        if rng.random() < 0.2:
            lines[i] = lines[i][:int(rng.integers(0, len(lines[i]) + 1))]
    return "\n".join(lines)
