"""The loaders against the ENGINE'S OWN files (ZeldaEngine.cpp:6882-6948 consume them): Content/Models/*.obj, Content/Textures/*.png.

`tests/golden/content_digests.json` was made from the engine's shipped content by `tests/golden/make_golden_content.py` with readers that
share no code with the product (PIL; a 30-line restatement of LoadMeshAsset): per PNG the size and the sha256 of the RGBA8 bytes, per OBJ
the vertex / index counts and the sha256 of the deduplicated XkVertex and index arrays.  The library's `zr_load_png_rgba8` / `zr_load_obj`
(host code of the C-ABI, no GPU needed) and the Python twins of `zeldaengine_amd.assets` must reproduce every digest.

The content tree itself is not part of this repository.  The known answers that SURVEY App. C derives from two of its files are asserted
from the digests alone.  The files are read from the engine's tree (Engine/ZeldaEngine/Content of its checkout; ZELDA_ENGINE_CONTENT
overrides the location); where that tree is absent, the four constant default_* textures, whose digest fixes every pixel, are read from
their stand-ins under `tests/golden/content/engine/` and the other files skip.  The stored fixtures under `tests/golden/content/`
(`make_golden_content_fixtures.py`, digested by the same readers) carry the engine files' formats and hold the loaders to them everywhere.
"""
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

from zeldaengine_amd import assets, engine

HERE = os.path.dirname(os.path.abspath(__file__))
CONTENT = os.path.join(HERE, "golden", "content")
DIGESTS = json.load(open(os.path.join(HERE, "golden", "content_digests.json")))
FIXTURES = json.load(open(os.path.join(HERE, "golden", "content_fixture_digests.json")))
ENGINE_CONTENT = os.environ.get("ZELDA_ENGINE_CONTENT", "/root/reference/Engine/ZeldaEngine/Content")     # the engine's tree, read-only
STAND_INS = os.path.join(CONTENT, "engine")


def _engine_file(kind, name):
    """the engine's file from its tree, else its stand-in (textures the digest fixes), else skip"""
    for root in (ENGINE_CONTENT, STAND_INS):
        if root and os.path.isfile(os.path.join(root, kind, name)):
            return os.path.join(root, kind, name)
    pytest.skip("%s/%s: the engine's content tree is not on this machine (ZELDA_ENGINE_CONTENT: its Engine/ZeldaEngine/Content)" % (kind, name))


def test_digest_file_covers_the_shipped_content_and_the_known_answers():
    assert len(DIGESTS["textures"]) == 14 and len(DIGESTS["models"]) == 5
    # sphere.obj 960 triangles, cube.obj 48, stage.obj 576 (indices / 3); App. C: default_normal (127,127,255), default_grey 127
    m = DIGESTS["models"]
    assert (m["sphere.obj"]["indices"], m["cube.obj"]["indices"], m["stage.obj"]["indices"]) == (2880, 144, 1728 + 432)
    assert m["sphere.obj"]["vertices"] == 559 and m["cube.obj"]["vertices"] == 48
    t = DIGESTS["textures"]
    assert t["default_normal.png"]["first_texel"][:3] == [127, 127, 255]
    assert t["default_grey.png"]["first_texel"][:3] == [127, 127, 127]
    assert t["default_black.png"]["first_texel"][:3] == [0, 0, 0] and t["default_white.png"]["first_texel"][:3] == [255, 255, 255]
    for k in ("cubemap_X0.png", "cubemap_X1.png", "cubemap_Y2.png", "cubemap_Y3.png", "cubemap_Z4.png", "cubemap_Z5.png"):
        assert (t[k]["width"], t[k]["height"]) == (1024, 1024)      # maxMips = 11 (ZE:4308,6887)


def _png_layout(path):
    """colour type, chunk types in order of first appearance, IDAT count, row filter types"""
    b = open(path, "rb").read()
    pos, types, idat = 8, [], b""
    while pos < len(b):
        n = struct.unpack(">I", b[pos:pos + 4])[0]
        types.append(b[pos + 4:pos + 8].decode())
        if types[-1] == "IDAT":
            idat += b[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, _, ct = struct.unpack(">IIBB", b[16:26])
    stride = w * (4 if ct == 6 else 3) + 1
    raw = zlib.decompress(idat)
    return ct, list(dict.fromkeys(types)), types.count("IDAT"), {raw[y * stride] for y in range(h)}


def test_stored_fixtures_carry_the_engines_file_formats():
    """What the engine's files hold (make_golden_content_fixtures.py lists it) is present in the stored fixtures, so that the loaders'
    tests below reach every path the engine's content would."""
    assert len(FIXTURES["textures"]) >= 5 and len(FIXTURES["models"]) >= 2
    lay = [_png_layout(os.path.join(CONTENT, "Textures", n)) for n in sorted(FIXTURES["textures"])]
    assert {ct for ct, _, _, _ in lay} == {2, 6}                                        # RGB8 and RGBA8
    assert any({"iTXt", "pHYs"} <= set(t) for _, t, _, _ in lay) and any("sRGB" in t for _, t, _, _ in lay)
    assert {1, 2} <= {k for _, _, k, _ in lay} and max(k for _, _, k, _ in lay) >= 97     # one, two and many IDAT chunks
    assert set().union(*(f for _, _, _, f in lay)) == {0, 1, 2, 3, 4}                    # every row filter type
    assert any(t["width"] != t["height"] for t in FIXTURES["textures"].values())
    objs = [open(os.path.join(CONTENT, "Models", n), "rb").read() for n in sorted(FIXTURES["models"])]
    assert any(b"\r\n" in o for o in objs)                                             # CRLF line ends
    assert all(b"\ng " in o and b"\nusemtl " in o and b"\nvn " in o and b"\nvt " in o for o in objs)
    faces = [ln.split()[1:] for o in objs for ln in o.decode().splitlines() if ln.startswith("f ")]
    assert {len(f) for f in faces} == {3, 4}                                             # triangles and quads
    assert any(c.split("/")[0] != c.split("/")[2] for f in faces for c in f)            # normal index != position index


def test_stand_ins_are_the_textures_their_digests_fix():
    """Every engine texture whose digest is a constant image has its stand-in, so those are checked on every machine."""
    want = []
    for name, t in DIGESTS["textures"].items():
        a = np.empty((t["height"], t["width"], 4), np.uint8)
        a[:] = t["first_texel"]
        if hashlib.sha256(a.tobytes()).hexdigest() == t["rgba8_sha256"]:
            want.append(name)
    assert sorted(os.listdir(os.path.join(STAND_INS, "Textures"))) == sorted(want) == ["default_black.png", "default_grey.png",
                                                                                      "default_normal.png", "default_white.png"]


@pytest.mark.parametrize("name", sorted(DIGESTS["textures"]))
def test_png_decoders_reproduce_the_engines_textures(name):
    want = DIGESTS["textures"][name]
    path = _engine_file("Textures", name)
    for who, img in (("zr_load_png_rgba8", engine.load_png_rgba8(path)), ("assets.load_image_rgba8", assets.load_image_rgba8(path))):
        assert img.dtype == np.uint8 and img.shape == (want["height"], want["width"], 4), who
        assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == want["rgba8_sha256"], who
        assert img[0, 0].tolist() == want["first_texel"], who


@pytest.mark.parametrize("name", sorted(DIGESTS["models"]))
def test_obj_loaders_reproduce_the_engines_models(name):
    want = DIGESTS["models"][name]
    path = _engine_file("Models", name)
    for who, (v, idx) in (("zr_load_obj", engine.load_obj(path)), ("assets.load_obj", assets.load_obj(path))):
        assert v.dtype.itemsize == 44 and idx.dtype == np.uint32, who
        assert (len(v), len(idx)) == (want["vertices"], want["indices"]), who
        assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == want["xkvertex_sha256"], who
        assert hashlib.sha256(np.ascontiguousarray(idx).tobytes()).hexdigest() == want["index_sha256"], who


@pytest.mark.parametrize("name", sorted(FIXTURES["textures"]))
def test_png_decoders_reproduce_the_stored_textures(name):
    want = FIXTURES["textures"][name]
    path = os.path.join(CONTENT, "Textures", name)
    for who, img in (("zr_load_png_rgba8", engine.load_png_rgba8(path)), ("assets.load_image_rgba8", assets.load_image_rgba8(path))):
        assert img.dtype == np.uint8 and img.shape == (want["height"], want["width"], 4), who
        assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == want["rgba8_sha256"], who
        assert img[0, 0].tolist() == want["first_texel"], who


@pytest.mark.parametrize("name", sorted(FIXTURES["models"]))
def test_obj_loaders_reproduce_the_stored_models(name):
    want = FIXTURES["models"][name]
    path = os.path.join(CONTENT, "Models", name)
    for who, (v, idx) in (("zr_load_obj", engine.load_obj(path)), ("assets.load_obj", assets.load_obj(path))):
        assert v.dtype.itemsize == 44 and idx.dtype == np.uint32, who
        assert (len(v), len(idx)) == (want["vertices"], want["indices"]), who
        assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == want["xkvertex_sha256"], who
        assert hashlib.sha256(np.ascontiguousarray(idx).tobytes()).hexdigest() == want["index_sha256"], who
