"""Writes the stored content fixtures (tests/golden/content/) and their digests (tests/golden/content_fixture_digests.json).

The engine's own content tree does not travel with this repository (only its digests do: content_digests.json), so the loaders are
held to files of our own that carry the same format features as the engine's `Content/Textures/*.png` and `Content/Models/*.obj`:

* PNG, 8 bits per channel: RGB (colour type 2) and RGBA (6); iTXt + pHYs ancillary chunks; one IDAT, two IDATs, and an sRGB image whose
  IDAT stream is cut into many chunks (the engine's cubemaps hold one, two and 97); square and non-square sizes; constant, patterned
  and noisy pixels; every PNG row filter type (None, Sub, Up, Average, Paeth);
* OBJ: CRLF line ends, `#` comments, `g` / `usemtl` lines, `v` / `vt` / `vn` with `f v/vt/vn` triangles; a sphere whose seam shares
  positions between corners of different texture coordinates (fewer `v` than `vt`, deduplication on the whole record); quad faces
  (fanned by the loaders); a face normal index that differs from its position index (the loaders take the normal by POSITION index).

For the engine textures whose digest fixes every pixel (the constant default_* images) it also writes stand-ins under
tests/golden/content/engine/Textures/, so that those are held to the ENGINE'S digests (content_digests.json) everywhere.

The digests come from the readers in make_golden_content.py (PIL; a restatement of LoadMeshAsset), which share no code with the
product.  They cover the DECODED content, so re-running this script with another zlib rewrites the files but not the digests.

    python tests/golden/make_golden_content_fixtures.py
"""
import hashlib
import io
import json
import math
import os
import struct
import sys
import zlib

import numpy as np
from PIL import Image, PngImagePlugin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_content import digest_obj, digest_png  # noqa: E402

OUT = os.path.join(HERE, "content")


def _text_info():
    info = PngImagePlugin.PngInfo()
    info.add_itxt("XML:com.adobe.xmp", "<x:xmpmeta xmlns:x='adobe:ns:meta/'/>")
    return info


def _chunks(data):
    pos, out = 8, []
    while pos < len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        out.append((data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def _filtered_rows(a, filters=(0, 1, 2, 3, 4)):
    """8-bit image rows, row y with filter filters[y % len(filters)] (0..4: None, Sub, Up, Average, Paeth; PNG spec 9.2), zlib-compressed"""
    h, w, bpp = a.shape
    rows = a.reshape(h, w * bpp).astype(np.int32)
    out = bytearray()
    for y in range(h):
        x, up = rows[y], rows[y - 1] if y else np.zeros_like(rows[0])
        left = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]])
        ul = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]])
        f = filters[y % len(filters)]
        if f == 4:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        else:
            pred = (0, left, up, (left + up) // 2)[f]
        out += bytes([f]) + ((x - pred) & 0xFF).astype(np.uint8).tobytes()
    return zlib.compress(bytes(out), 9)


def _png(img, path, info=None, srgb=False, idat_pieces=1, filters=None):
    """PIL's encoder, then (optionally) an sRGB chunk ahead of the image data, the rows re-encoded with the given filter types in turn,
    and the IDAT stream cut into `idat_pieces` chunks"""
    buf = io.BytesIO()
    kw = {"pnginfo": info} if info is not None else {}
    if info is not None:
        kw["dpi"] = (72, 72)                    # pHYs
    img.save(buf, "PNG", **kw)
    ch = _chunks(buf.getvalue())
    idat = _filtered_rows(np.asarray(img), filters) if filters else b"".join(d for t, d in ch if t == b"IDAT")
    step = -(-len(idat) // idat_pieces)
    out = b"\x89PNG\r\n\x1a\n"
    for t, d in ch:
        if t == b"IDAT":
            continue
        if t == b"IEND":
            for k in range(0, len(idat), step):
                out += _chunk(b"IDAT", idat[k:k + step])
        if t == b"IHDR" and srgb:
            out += _chunk(t, d) + _chunk(b"sRGB", b"\x00")
            continue
        out += _chunk(t, d)
    with open(path, "wb") as f:
        f.write(out)


def textures(d):
    rng = np.random.default_rng(20241015)
    os.makedirs(d, exist_ok=True)
    # constant 64 x 64 RGB, one IDAT, iTXt + pHYs (the engine's default_* images)
    _png(Image.new("RGB", (64, 64), (127, 127, 255)), os.path.join(d, "rgb8_flat_text_phys.png"), _text_info())
    # 64 x 64 RGBA grid with an alpha ramp (default_grid*)
    a = np.zeros((64, 64, 4), np.uint8)
    a[..., :3] = 96
    a[::8, :, :3] = 230
    a[:, ::8, :3] = 230
    a[..., 3] = np.arange(64, dtype=np.uint8)[None, :] * 4 + 3
    _png(Image.fromarray(a, "RGBA"), os.path.join(d, "rgba8_grid_text_phys.png"), _text_info())
    # non-square RGB, smooth with noise (background.png's 1080 x 720 at 1 / 8)
    y, x = np.mgrid[0:90, 0:135].astype(np.float64)
    g = np.stack([128 + 100 * np.sin(x / 11.0), 128 + 100 * np.cos(y / 7.0), (x + y) * 255.0 / 224.0], -1)
    g = np.clip(g + rng.integers(-6, 7, size=g.shape), 0, 255).astype(np.uint8)
    _png(Image.fromarray(g, "RGB"), os.path.join(d, "rgb8_nonsquare_text_phys.png"), _text_info())
    # square RGB in two IDAT chunks (cubemap_Z4) and with an sRGB chunk and 97 IDAT chunks (cubemap_Z5)
    y, x = np.mgrid[0:128, 0:128].astype(np.float64)
    r = np.hypot(x - 64, y - 64)
    c = np.stack([127 + 120 * np.cos(r / 5.0), 2 * y - x / 2 + 64, 255 - 2 * x], -1)
    c = np.clip(c + rng.integers(-3, 4, size=c.shape), 0, 255).astype(np.uint8)
    _png(Image.fromarray(c, "RGB"), os.path.join(d, "rgb8_two_idat_text_phys.png"), _text_info(), idat_pieces=2)
    _png(Image.fromarray(np.ascontiguousarray(c[::-1, :, ::-1]), "RGB"), os.path.join(d, "rgb8_srgb_97_idat_all_filters.png"), srgb=True,
         idat_pieces=97, filters=(0, 1, 2, 3, 4))


def engine_stand_ins(d):
    """The engine textures whose pixels their digest fixes (constant images: size + first texel reproduce the sha256), encoded as the
    engine's are (RGB, iTXt + pHYs, filter None): test_content_pins.py holds the loaders to the ENGINE'S digests with these."""
    os.makedirs(d, exist_ok=True)
    for name, t in sorted(json.load(open(os.path.join(HERE, "content_digests.json")))["textures"].items()):
        a = np.empty((t["height"], t["width"], 4), np.uint8)
        a[:] = t["first_texel"]
        if hashlib.sha256(a.tobytes()).hexdigest() != t["rgba8_sha256"] or t["first_texel"][3] != 255:
            continue
        _png(Image.fromarray(np.ascontiguousarray(a[..., :3]), "RGB"), os.path.join(d, name), _text_info(), filters=(0,))


def _fmt(x):
    return "%.6f" % x


def _write_obj(path, lines, crlf):
    with open(path, "wb") as f:
        f.write(("\r\n" if crlf else "\n").join(lines + [""]).encode())


def models(d):
    os.makedirs(d, exist_ok=True)
    # UV sphere: 12 slices x 6 stacks, positions shared across the seam, texture columns not (slices + 1 per ring)
    sl, st = 12, 6
    P, T = [(0.0, 0.0, 0.5)], []
    for i in range(1, st):
        th = math.pi * i / st
        for j in range(sl):
            ph = 2 * math.pi * j / sl
            P.append((0.5 * math.sin(th) * math.cos(ph), 0.5 * math.sin(th) * math.sin(ph), 0.5 * math.cos(th)))
    P.append((0.0, 0.0, -0.5))
    for i in range(st + 1):
        for j in range(sl + 1):
            T.append((j / sl, 1.0 - i / st))

    def pv(i, j):                  # 1-based position index of ring i (0 = north pole, st = south pole), column j
        return 1 if i == 0 else len(P) if i == st else 1 + (i - 1) * sl + j % sl + 1

    def tv(i, j):
        return 1 + i * (sl + 1) + j
    lines = ["# stored fixture: UV sphere, %d slices x %d stacks" % (sl, st), "# positions shared across the texture seam", "",
             "g sphere", "usemtl default"]
    lines += ["v %s %s %s" % tuple(map(_fmt, p)) for p in P]
    lines += ["vn %s %s %s" % tuple(_fmt(c / math.sqrt(sum(q * q for q in p))) for c in p) for p in P]
    lines += ["vt %s %s" % tuple(map(_fmt, t)) for t in T]
    for i in range(st):
        for j in range(sl):
            a, b, c, e = (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
            for tri in ((a, c, b), (b, c, e)):
                if pv(*tri[0]) in (pv(*tri[1]), pv(*tri[2])) or pv(*tri[1]) == pv(*tri[2]):
                    continue                                            # the degenerate half of a pole quad
                lines.append("f " + " ".join("%d/%d/%d" % (pv(*q), tv(*q), pv(*q)) for q in tri))
    _write_obj(os.path.join(d, "sphere_seam_crlf.obj"), lines, crlf=True)

    # 4 x 3 grid of quads + a triangle fan cap, LF line ends; the face normal index runs backwards (the loaders use the position's)
    n_x, n_y = 4, 3
    P = [(x * 0.5 - 1.0, y * 0.5 - 0.75, 0.05 * ((x * 3 + y * 5) % 4)) for y in range(n_y + 1) for x in range(n_x + 1)]
    P.append((0.0, 1.25, 0.3))
    N = [(0.0, 0.0, 1.0) if k % 2 == 0 else (0.0, 0.6, 0.8) for k in range(len(P))]
    T = [(x / n_x, y / n_y) for y in range(n_y + 1) for x in range(n_x + 1)] + [(0.5, 1.25)]
    lines = ["# stored fixture: a grid of quads and a cap of triangles", "g stage", "usemtl default"]
    lines += ["v %s %s %s" % tuple(map(_fmt, p)) for p in P]
    lines += ["vn %s %s %s" % tuple(map(_fmt, q)) for q in N]
    lines += ["vt %s %s" % tuple(map(_fmt, t)) for t in T]
    nv = len(P)

    def k(x, y):
        return y * (n_x + 1) + x + 1
    for y in range(n_y):
        for x in range(n_x):
            lines.append("f " + " ".join("%d/%d/%d" % (q, q, nv + 1 - q) for q in (k(x, y), k(x + 1, y), k(x + 1, y + 1), k(x, y + 1))))
    for x in range(n_x):
        lines.append("f " + " ".join("%d/%d/%d" % (q, q, nv + 1 - q) for q in (k(x, n_y), k(x + 1, n_y), nv)))
    _write_obj(os.path.join(d, "quads_lf.obj"), lines, crlf=False)


def main():
    textures(os.path.join(OUT, "Textures"))
    models(os.path.join(OUT, "Models"))
    engine_stand_ins(os.path.join(OUT, "engine", "Textures"))
    dg = {"source": "tests/golden/content (written by make_golden_content_fixtures.py)", "textures": {}, "models": {}}
    for name in sorted(os.listdir(os.path.join(OUT, "Textures"))):
        dg["textures"][name] = digest_png(os.path.join(OUT, "Textures", name))
    for name in sorted(os.listdir(os.path.join(OUT, "Models"))):
        dg["models"][name] = digest_obj(os.path.join(OUT, "Models", name))
    with open(os.path.join(HERE, "content_fixture_digests.json"), "w") as f:
        json.dump(dg, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d textures, %d models" % (len(dg["textures"]), len(dg["models"])))


if __name__ == "__main__":
    main()
