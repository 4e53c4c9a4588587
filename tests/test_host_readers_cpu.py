"""The host's readers of bytes it did not make - the world document (csrc/zr_world_doc.cpp), OBJ and PNG files
(csrc/zr_asset_files.cpp) - as plain C++ in a stand-alone program (tests/host_readers_check.cpp) under the address and
undefined-behaviour sanitizers, over valid, cut and mutated input; and the built library, in process, gives every case the same verdict and
the same content.  No GPU, nothing of the program loaded into Python."""
import copy
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np

import asset_mutations as am
from zeldaengine_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "xkworld_untitled.json")
PLAIN = ("zr_world_doc.cpp", "zr_asset_files.cpp")
N_DOC_MUTATIONS, N_FILES = 2000, 2000
MAX_INSTANCES = 4194304                                    # XK_WORLD_MAX_INSTANCES_PER_OBJECT
LIGHT_LIMITS = {"DirectionalLights": 16, "PointLights": 512, "SpotLights": 16}


def fnv1a(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_the_plain_sources_reach_nothing_of_hip():
    """What the two files include with quotes, followed transitively, holds neither the context nor the device types (and with them
    hip/hip_runtime.h)."""
    reached = {os.path.basename(p) for f in PLAIN for p in build._deps(os.path.join(CSRC, f))}
    assert not reached & {"zr_ctx.h", "zr_types.h"}, sorted(reached)


def test_the_moved_code_lives_in_one_place():
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".h", ".hip"))}
    for needle, home in (("struct JParser", "zr_world_doc.cpp"), ("parse_obj", "zr_asset_files.cpp"), ("unfilter(", "zr_asset_files.cpp"),
                         ("livelink_thread", "zr_livelink.cpp"), ("file names in a world must be relative to the content tree", "zr_assets.cpp")):
        assert [f for f, t in text.items() if needle in t] == [home], needle
    assert text["zr_assets.cpp"].count("file names in a world must be relative to the content tree") == 1


# ---------------------------------------------------------------- the corpus of documents

def _mutated_documents(golden, rng, n):
    """byte, insert and delete mutations of the golden payload, one to three per document; half of the new bytes are JSON's own"""
    own = b'{}[]",:-+.eE0123456789\\utfn '
    out = []
    for _ in range(n):
        d = bytearray(golden)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(d)))
            new = int(own[int(rng.integers(0, len(own)))]) if rng.random() < 0.5 else int(rng.integers(0, 256))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                d[at] = new
            elif kind == 1:
                d.insert(at, new)
            else:
                del d[at]
        out.append(bytes(d))
    return out


RAW = 987654321.5                                          # a number no document holds: its text is replaced by a raw token


def _changed_documents(golden):
    """Documents made by changing values of the golden payload through json.dumps (and raw number tokens through a placeholder)."""
    base = json.loads(golden)
    docs = []

    def emit(d, raw=None, ascii=True, dup=False):
        t = json.dumps(d, ensure_ascii=ascii)
        if raw is not None:
            assert t.count(repr(RAW)) == 1
            t = t.replace(repr(RAW), raw)
        if dup:
            t = t.replace('"__dup__', '"')
        docs.append(t.encode("utf-8", "surrogatepass"))

    def changed(path, value, **kw):
        d = copy.deepcopy(base)
        o = d
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = value
        emit(d, **kw)

    floats = [("MainCamera", "FOV"), ("MainCamera", "Position", 1), ("PointLights", 3, "Intensity"), ("DirectionalLights", 0, "ExtraData", 3), ("Objects", 2, "MinRadius")]
    uints = [("PointLights", 0, "Type"), ("Objects", 1, "RenderFlags"), ("Objects", 4, "InstanceCount")]
    # numbers: negative zero, the ends of the float range and beyond, denormals, integers at and beyond 2^24, 2^32 and 2^53
    for v in (-0.0, 0.0, 1e-50, -1e-45, 5e-324, 1.17549435e-38, 0.1, 1e-7, 123456789.123456789, 3.4028234e38, 3.5e38, 1e39, -1e39, 1e308,
              16777217, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 53 + 1, -2 ** 31, 10 ** 40):
        for path in floats:
            changed(path, v)
    for v in (0, 1, 255, 256, 65535, 65536, MAX_INSTANCES - 1, MAX_INSTANCES, MAX_INSTANCES + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 64, -1, 1.0, 1.5, 1e3):
        for path in uints:
            changed(path, v)
    for tok in ("-0", "-0.0", "1e3", "1E+2", "1e-2", "01", "1.", ".5", "+1", "1e999", "-1e999", "1e-999", "-", "1e", "1e+", "0x10", "NaN", "Infinity", "1" + "0" * 400, "0." + "0" * 400 + "1"):
        changed(floats[0], RAW, raw=tok)
        changed(uints[2], RAW, raw=tok)
    # strings: every escape, control characters, non-ASCII text as \\u escapes and as UTF-8, a lone surrogate, names a loader would refuse
    for v in ("", 'a"b', "back\\slash", "sl/ash", "\b\f\n\r\t", "\x01\x1f\x7f", "Zürich", "東京", "\U0001F3AE", "\ud800", "../x", "/abs", "a\x00b", "x" * 5000):
        for path in (("Skydome", "SkydomeFileName"), ("Skydome", "CubemapFileNames", 2), ("Background", "BackgroundFileName"), ("Objects", 1, "ProfabName")):
            changed(path, v)
            changed(path, v, ascii=False)
    # extra keys (ignored), nesting at and beyond the parser's depth, duplicate keys (the first one counts)
    deep = lambda n: json.loads("[" * n + "]" * n)      # noqa: E731
    for where in ((), ("MainCamera",), ("Skydome",), ("PointLights", 0), ("Objects", 0)):
        for v in (None, {"a": [1, {"b": "c"}]}, deep(60), deep(70)):
            changed(where + ("Extra",), v)
    for path, v in ((("MainCamera", "FOV"), 50.0), (("PointLights", 0, "Type"), 7), (("Objects", 4, "InstanceCount"), 3), (("PointLights",), []), (("Objects", 1, "ProfabName"), "other"),
                    (("MainCamera", "FOV"), "wrong type, but second"), (("Skydome",), None)):
        changed(path[:-1] + ("__dup__" + path[-1],), v, dup=True)
    # a missing key, a value of another type: at every key of the schema
    def keys(o, path=()):
        if isinstance(o, dict):
            for k, v in o.items():
                yield path + (k,)
                yield from keys(v, path + (k,))
        elif isinstance(o, list) and o and isinstance(o[0], dict):
            yield from keys(o[0], path + (0,))
    for path in keys(base):
        d = copy.deepcopy(base)
        o = d
        for k in path[:-1]:
            o = o[k]
        was = o.pop(path[-1])
        emit(d)
        changed(path, "text" if not isinstance(was, str) else 5)
        changed(path, None)
    # lists: lights at 0, 1, their limit and one more; objects 0, 1, many; cube names and vectors too short, too long, of the wrong kind
    for key, limit in LIGHT_LIMITS.items():
        for n in (0, 1, limit, limit + 1):
            changed((key,), [copy.deepcopy(base["PointLights"][i % 16]) for i in range(n)])
    for n in (0, 1, 200):
        changed(("Objects",), [copy.deepcopy(base["Objects"][i % 5]) for i in range(n)])
    for v in ([], ["a"] * 5, ["a"] * 6, ["a"] * 7, ["a", 1, "b", "c", "d", "e"]):
        changed(("Skydome", "CubemapFileNames"), v)
    for v in ([], [1.0, 2.0], [1.0, 2.0, 3.0, 4.0], [1.0, "2", 3.0], [1.0, None, 3.0], [[1.0], 2.0, 3.0]):
        changed(("MainCamera", "Position"), v)
        changed(("PointLights", 5, "ExtraData"), v)
    changed(("PointLights", 2), 5)
    changed(("Objects", 2), [])
    for whole in ([], "text", 5, None, True):
        emit(whole)
    return docs


def _cut_tokens(golden):
    """escapes and numbers cut at the end of the input, a lone surrogate, 100 000 opening brackets, bytes around a whole document"""
    head = golden[:golden.index(b'"FOV": ') + 7]
    cuts = [head + t for t in (b"-", b"1e", b"1e999", b"1.", b"t", b"tru", b"nul", b'"\\', b'"\\u', b'"\\u0', b'"\\u00', b'"\\u004', b'"\\ud800', b'"\\ud800"', b'"\\x"', b'"')]
    return cuts + [b"[" * 100000, b"{" * 100000, b"", b" ", b"\xef\xbb\xbf" + golden, golden + b" \n\t\r", golden + b"x", golden + b"\x00", b" " + golden, golden[:-1] + b",}"]


def _normalize(L, doc):
    """engine.world_json_normalize, the bytes undecoded -> (accepted, the written text or the loader's message)"""
    n = C.c_size_t()
    L.zr_world_json_normalize(doc, len(doc), None, 0, C.byref(n))
    buf = C.create_string_buffer(max(1, n.value))
    rc = L.zr_world_json_normalize(doc, len(doc), buf, n.value, C.byref(n))
    assert rc in (0, -4), rc
    return rc == 0, buf.raw[:n.value]


def _build(tmp_path):
    """as tests/test_frame_delta_codec_cpu.py does: the sanitizers where this machine links them for a stand-alone program"""
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_SANITIZE_VECTOR"]      # (a vector's spare capacity is out of bounds too)
    hello = tmp_path / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp_path / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp_path / "hello")]) == 0):
        sanitize = []
    print("host_readers_check is built %s" % ("with " + " ".join(sanitize) if sanitize else "WITHOUT the sanitizers: this machine does not link them"))
    exe = tmp_path / "host_readers_check"
    sources = [os.path.join(ROOT, "tests", "host_readers_check.cpp")] + [os.path.join(CSRC, f) for f in PLAIN]
    objs = [str(tmp_path / (os.path.basename(src) + ".o")) for src in sources]
    compiles = [subprocess.Popen(["g++"] + flags + sanitize + ["-I", CSRC, "-c", src, "-o", obj]) for src, obj in zip(sources, objs)]      # side by side
    assert [p.wait() for p in compiles] == [0] * len(sources)
    subprocess.check_call(["g++"] + sanitize + objs + ["-lz", "-o", str(exe)])
    return exe


def test_the_host_readers_under_the_sanitizers_and_against_the_library(tmp_path):
    """Documents: the golden payload and every strict prefix of it (5 727; refused, since the payload's last byte is its closing brace),
    2 000 seeded byte / insert / delete mutations, some 500 documents with values changed through json.dumps (numbers up to and beyond
    the ranges of float and uint32, every string escape, non-ASCII text, extra / duplicate / missing keys, wrong types, lists at 0 and at
    their limits, InstanceCount at and above the cap), cut escapes and numbers, 100 000 brackets.  Each is parsed from a heap block of
    exactly its length.  An accepted document whose floats are all finite must be a fixed point of parse -> write -> parse -> write.
    Files: 2 000 damaged PNG and 2 000 damaged OBJ files from tests/asset_mutations.py; an image is w * h * 4 bytes and at most 16 384 on a
    side, an index count a multiple of three with every index below the vertex count.  The library is then given every case in process:
    the same verdict, and for accepted cases the same text, pixels, vertices and indices (64-bit FNV-1a on both sides; a refused
    document: the same message)."""
    exe = _build(tmp_path)
    golden = open(GOLDEN, "rb").read()
    assert golden.endswith(b"}")
    rng = np.random.default_rng(2024)
    prefixes = [golden[:n] for n in range(len(golden))]
    changed = _changed_documents(golden)
    docs = prefixes + [golden] + _mutated_documents(golden, rng, N_DOC_MUTATIONS) + changed + _cut_tokens(golden)
    assert len(changed) >= 300
    with open(tmp_path / "docs.bin", "wb") as f:
        f.write(struct.pack("<I", len(docs)) + b"".join(struct.pack("<I", len(d)) + d for d in docs))
    os.makedirs(tmp_path / "png"); os.makedirs(tmp_path / "obj")
    seeds = am.png_seeds(tmp_path, rng)
    for k in range(N_FILES):
        open(tmp_path / "png" / ("%d.png" % k), "wb").write(am.mutated_png(rng, seeds, k))
    for k in range(N_FILES):
        open(tmp_path / "obj" / ("%d.obj" % k), "w").write(am.mutated_obj(rng, am.OBJ * 3))

    run = subprocess.run([str(exe), str(tmp_path), str(N_FILES), str(N_FILES)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = run.stdout.splitlines()
    print("\n".join(lines[-3:]))
    assert run.returncode == 0, "\n".join(lines[-3:]) + run.stderr[-4000:]
    rows = {"doc": [], "png": [], "obj": []}
    for line in lines[:-3]:
        w = line.split()
        assert int(w[1]) == len(rows[w[0]])
        rows[w[0]].append(dict(x.split("=") for x in w[2:]))
    assert [len(rows[k]) for k in ("doc", "png", "obj")] == [len(docs), N_FILES, N_FILES]
    tally = [dict(zip(t[2::2], map(int, t[3::2]))) for t in (line.split() for line in lines[-3:])]
    assert all(t["broken"] == 0 for t in tally)

    doc = rows["doc"]
    assert all(r["ok"] == "0" for r in doc[:len(prefixes)]) and doc[len(prefixes)]["ok"] == "1"
    accepted = [r for r in doc if r["ok"] == "1"]
    assert len(accepted) >= 200 and len(doc) - len(accepted) >= 200
    assert all(r["fixed"] == "1" for r in accepted if r["finite"] == "1")
    assert tally[0]["nonfinite"] == sum(r["finite"] == "0" for r in accepted) > 0      # (1e39 and its like: DESIGN.md, "Where the host code lives")

    L = engine.lib()
    for k, (d, r) in enumerate(zip(docs, doc)):
        ok, text = _normalize(L, d)
        assert (ok, fnv1a(text)) == (r["ok"] == "1", r["hash"]), (k, d[:80], text[:200])
    for k, r in enumerate(rows["png"]):
        try:
            img = engine.load_png_rgba8(str(tmp_path / "png" / ("%d.png" % k)))
            assert r["ok"] == "1" and (int(r["h"]), int(r["w"]), 4) == img.shape and fnv1a(img.tobytes()) == r["hash"], k
        except engine.ZeldaRenderError:
            assert r["ok"] == "0", k
    for k, r in enumerate(rows["obj"]):
        try:
            v, idx = engine.load_obj(str(tmp_path / "obj" / ("%d.obj" % k)))
            assert r["ok"] == "1" and (int(r["nv"]), int(r["ni"])) == (len(v), len(idx)) and fnv1a(v.tobytes() + idx.tobytes()) == r["hash"], k
        except engine.ZeldaRenderError:
            assert r["ok"] == "0", k
    # both verdicts are met: of the damaged images more than a quarter are refused (the proportion tests/test_assets.py asks of its 150)
    assert tally[1]["refused"] > N_FILES // 4 and tally[1]["accepted"] > 0 and tally[2]["refused"] > 0 and tally[2]["accepted"] > 0
