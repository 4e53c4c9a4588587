"""Highlighting a selection without a GPU: the blend of csrc/zr_highlight.h is the nearest integer and its shift form the division; the
library's host statement of the rule (zr_frame_highlight, context-free host code) equals the numpy statement
(tests/highlight_reference.py) byte for byte over the edge shapes, every radius, four styles and the masks that sit on tile and word
borders; the identities; a stand-alone program runs the shared header - the rule and the kernels' windows - under the sanitizers from
and into exactly-sized heap buffers; the C-ABI carries the entry points in the public header, the ctypes binding and the built library
alike; and the frames the GPU test renders (tests/highlight_cases.py), rendered here on the CPU oracle, put selected and outline pixels
where the kernels can go wrong."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import highlight_cases as hc
import highlight_reference as hr
import ids_reference as idr
from zeldaengine_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
ENTRY_POINTS = ("zr_highlight_set", "zr_highlight_clear", "zr_highlight_get", "zr_set_highlight_style", "zr_get_highlight_style",
                "zr_read_color_highlighted", "zr_copy_frame_highlighted_async", "zr_set_frame_delta_highlight", "zr_frame_highlight")


def _random(W, H, seed=0):
    return np.random.default_rng(1000 * W + H + seed).integers(0, 256, size=(H, W, 4), dtype=np.uint8)


def _masks(W, H):
    """name -> (H, W) uint8"""
    rng = np.random.default_rng(7 * W + H)
    out = {}
    for pct in (1, 50, 99):
        out["random%d" % pct] = (rng.random((H, W)) < pct / 100.0).astype(np.uint8)
    out["empty"] = np.zeros((H, W), np.uint8)
    out["full"] = np.ones((H, W), np.uint8)
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (31, 31), (32, 32), (63, 0), (64, 0)):
        if x < W and y < H:
            m = np.zeros((H, W), np.uint8)
            m[y, x] = 200                                # (any non-zero byte is "highlighted")
            out["pixel_%d_%d" % (x, y)] = m
    yy, xx = np.mgrid[0:H, 0:W]
    out["checker"] = ((xx + yy) & 1).astype(np.uint8)
    out["row"] = np.zeros((H, W), np.uint8); out["row"][H // 2, :] = 1
    out["column"] = np.zeros((H, W), np.uint8); out["column"][:, W // 2] = 1
    return out


def _abi_style(st):
    return abi.make_highlight_style(st["outline"], st["fill"], st["radius"])


# ---- the blend

def test_the_blend_is_the_nearest_integer_and_the_shift_form_is_the_division():
    x = np.arange(0, 65026, dtype=np.int64)
    rule = (x + 127) // 255
    assert np.array_equal(rule, np.rint(x / 255.0).astype(np.int64))
    assert float(np.abs(x / 255.0 - np.floor(x / 255.0) - 0.5).min()) > 1e-3        # 255 is odd: no tie
    t = x + 128
    assert np.array_equal((t + (t >> 8)) >> 8, rule)
    assert int((255 * 255 + 127)) == 65152                                         # the largest intermediate of the rule
    p, q = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal(hr.blend(p, q, 0), p) and np.array_equal(hr.blend(p, q, 255), q)
    text = open(os.path.join(CSRC, "zr_highlight.h")).read()
    assert "const uint32_t t = x + 128u; return (t + (t >> 8)) >> 8;" in text      # the form the header divides by


# ---- zr_frame_highlight against the reference

@pytest.mark.parametrize("W,H", hc.SHAPES, ids=hc.SHAPE_IDS)
def test_host_statement_equals_the_reference(W, H):
    img = _random(W, H)
    masks = _masks(W, H)
    n = 0
    for name, m in masks.items():
        for r in hr.RADII:
            for sname in hr.STYLES:
                st = hr.style(sname, r)
                got = engine.frame_highlight(img, m, _abi_style(st))
                want = hr.highlight(img, m, st)
                assert np.array_equal(got, want), "%s r=%d %s: first difference at %s" % (name, r, sname, np.argwhere(got != want)[0].tolist())
                assert np.array_equal(got[..., 3], img[..., 3])
                n += 1
    assert n == len(masks) * 9 * 4 and len(masks) >= 10


def test_identities():
    img = _random(66, 34, seed=3)
    full = np.ones((34, 66), np.uint8)
    for r in hr.RADII:
        for sname in hr.STYLES:
            st = _abi_style(hr.style(sname, r))
            assert np.array_equal(engine.frame_highlight(img, np.zeros((34, 66), np.uint8), st), img)      # an empty set
    for m in _masks(66, 34).values():
        st = abi.make_highlight_style((1, 2, 3, 255), (4, 5, 6, 0), 0)                                      # radius 0, no fill
        assert np.array_equal(engine.frame_highlight(img, m, st), img)
        assert np.array_equal(engine.frame_highlight(img, m, _abi_style(hr.style("clear", 8))), img)        # everything transparent
    out = engine.frame_highlight(img, full, abi.make_highlight_style((0, 0, 0, 255), (9, 8, 7, 255), 8))
    assert (out[..., :3] == (9, 8, 7)).all() and np.array_equal(out[..., 3], img[..., 3])                   # A is never touched
    assert np.array_equal(engine.frame_highlight(img, full, None), img)                                     # the default fills nothing
    d = abi.make_highlight_style()
    assert (list(d.outline), list(d.fill), d.radius, d.reserved) == ([255, 160, 0, 255], [255, 160, 0, 0], 2, 0)
    assert hr.DEFAULT == {"outline": tuple(d.outline), "fill": tuple(d.fill), "radius": d.radius}


def test_refusals_of_the_context_free_function():
    L = engine.lib()
    img, m = _random(33, 17), np.ones((17, 33), np.uint8)
    out = np.full((17, 33, 4), 0xA5, dtype=np.uint8)
    src, msk, dst = (a.ctypes.data_as(C.c_void_p) for a in (img, m, out))
    st = abi.make_highlight_style()
    ok = (src, msk, 33, 17, C.byref(st), 16, dst, out.nbytes)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.zr_frame_highlight(*a)
    assert call(a0=None) == call(a1=None) == call(a4=None) == call(a6=None) == abi.ERR_ARG
    assert call(a2=0) == call(a3=0) == abi.ERR_ARG
    assert call(a5=12) == call(a5=20) == abi.ERR_ARG
    assert call(a7=out.nbytes - 4) == call(a7=out.nbytes + 4) == abi.ERR_ARG
    for bad in (abi.HighlightStyle((C.c_uint8 * 4)(), (C.c_uint8 * 4)(), 9, 0), abi.HighlightStyle((C.c_uint8 * 4)(), (C.c_uint8 * 4)(), 2, 1)):
        assert call(a4=C.byref(bad)) == abi.ERR_ARG
    assert (out == 0xA5).all(), "a refused call wrote into the destination"
    assert call() == 0 and np.array_equal(out, hr.highlight(img, m, hr.DEFAULT))
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.frame_highlight(img, m, abi.HighlightStyle((C.c_uint8 * 4)(), (C.c_uint8 * 4)(), 9, 0))
    assert e.value.code == abi.ERR_ARG


# ---- the shared header as a stand-alone program under the sanitizers

def _fnv(a):
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_shared_header_under_the_sanitizers(tmp_path):
    """tests/highlight_check.cpp includes csrc/zr_highlight.h alone and is compiled with g++ under the address and undefined-behaviour
    sanitizers where this machine links them for a stand-alone program (as tests/test_frame_scale_cpu.py does), and run on the CPU:
    the rule from and into exactly-sized heap buffers, and the kernels' windows - one or two words per row, every x0, every radius -
    against it; its digests are the reference's."""
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hello = tmp_path / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp_path / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp_path / "hello")]) == 0):
        sanitize = []
    exe = tmp_path / "highlight_check"
    subprocess.check_call(["g++"] + flags + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "highlight_check.cpp"), "-o", str(exe)])
    cases = []
    for W, H in [(7, 5), (33, 17), (66, 34), (130, 40), (257, 131)]:
        img, masks = _random(W, H, seed=2), _masks(W, H)
        for i, (name, m) in enumerate(masks.items()):
            for r in (hr.RADII if name in ("random1", "random50", "checker") or name.startswith("pixel") else (0, 3, 8)):
                cases.append((img, m, hr.style(list(hr.STYLES)[(i + r) % 4], r)))
    blob = [np.array([len(cases)], dtype="<u4").tobytes()]
    for img, m, st in cases:
        blob += [np.array([img.shape[1], img.shape[0], st["radius"]], dtype="<u4").tobytes(), bytes(st["outline"]), bytes(st["fill"]), img.tobytes(), m.tobytes()]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    run = subprocess.run([str(exe), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "cases %d failed 0" % len(cases) and len(lines) == len(cases) + 1
    want = {}
    for line, (img, m, st) in zip(lines, cases):
        key = (img.shape, m.tobytes(), repr(st))
        if key not in want:
            want[key] = _fnv(hr.highlight(img, m, st))
        assert int(line.split("fnv=")[1], 16) == want[key], line


# ---- the C-ABI

def test_the_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert hasattr(L, name), name
        assert name in abi.HIGHLIGHT_SIGNATURES and getattr(L, name).argtypes == abi.HIGHLIGHT_SIGNATURES[name]
    assert set(ENTRY_POINTS) == set(abi.HIGHLIGHT_SIGNATURES)
    for m in ("highlight_set", "highlight_clear", "highlight_get", "set_highlight_style", "highlight_style", "color_highlighted",
              "copy_frame_highlighted_async", "set_frame_delta_highlight"):
        assert callable(getattr(engine.Renderer, m))
    assert callable(engine.frame_highlight)


def test_header_binding_and_library_agree_on_version_7_and_the_style_is_16_bytes(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == abi.ABI_VERSION == engine.lib().zr_abi_version() == 7
    src = tmp_path / "style.c"
    src.write_text('#include "zelda_render.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu %zu %zu", sizeof(zr_highlight_style), '
                   'offsetof(zr_highlight_style, outline), offsetof(zr_highlight_style, fill), offsetof(zr_highlight_style, radius), '
                   'offsetof(zr_highlight_style, reserved));return 0;}\n')
    exe = tmp_path / "style"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = abi.HighlightStyle
    assert got == [16, 0, 4, 8, 12] == [C.sizeof(S), S.outline.offset, S.fill.offset, S.radius.offset, S.reserved.offset]


def test_the_kernel_file_shares_the_census_steps():
    """find_draw, the wave's one-search shortcut and primitive -> instance live once, in the header both kernel files include"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("zr_ids.hip", "zr_highlight.hip", "zr_ids_dev.h")}
    for f in ("zr_ids.hip", "zr_highlight.hip"):
        assert '#include "zr_ids_dev.h"' in text[f] and "uint32_t find_draw(" not in text[f] and "/ D.n_tris" not in text[f]
    assert text["zr_ids_dev.h"].count("uint32_t find_draw(") == 1 and text["zr_ids_dev.h"].count("local / D.n_tris") == 1
    shared = open(os.path.join(CSRC, "zr_highlight.h")).read()
    assert "#include <hip" not in shared and "__global__" not in shared and "zr_dev.h" not in shared      # plain C++: nothing of HIP in it


# ---- the GPU test's inputs are not vacuous

def _conditions(mask, empty, r):
    """what one case (a mask, the empty pixels, a radius) shows, as a dict of booleans"""
    H, W = mask.shape
    near = hr.dilate(mask, r)
    ring = near & ~mask
    c = {"corner_%d" % i: bool(mask[y, x]) for i, (x, y) in enumerate(((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)))}
    c.update(row0=bool(mask[0].any()), row_last=bool(mask[-1].any()), col0=bool(mask[:, 0].any()), col_last=bool(mask[:, -1].any()))
    c["across_x"] = W > 32 and bool((mask[:, 31] != mask[:, 32]).any())
    c["across_y"] = H > 32 and bool((mask[31] != mask[32]).any())
    c["isolated"] = bool(_isolated(mask).any())
    other, bare = False, False
    for y0 in range(0, H, 32):
        for x0 in range(0, W, 32):
            t = np.zeros_like(mask)
            t[y0:y0 + 32, x0:x0 + 32] = mask[y0:y0 + 32, x0:x0 + 32]
            local = hr.dilate(t, r)[y0:y0 + 32, x0:x0 + 32]
            tring = ring[y0:y0 + 32, x0:x0 + 32]
            other |= bool((tring & ~local).any())                  # an outline pixel whose every selected neighbour lies in another tile
            bare |= bool(tring.any()) and not t.any()              # a tile with no selected pixel but with outline pixels
    c["outline_from_other_tile"], c["bare_tile_with_outline"] = other, bare
    c["outline_on_empty"] = bool((ring & empty).any())
    return c


def _isolated(mask):
    """selected pixels with no selected 8-neighbour"""
    H, W = mask.shape
    pad = np.zeros((H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1] = mask
    nb = np.zeros((H, W), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                nb |= pad[dy:dy + H, dx:dx + W]
    return mask & ~nb


@pytest.fixture(scope="module")
def oracle_planes(oracle_lib):
    """(W, H, camera) -> (slot plane, -1 = no winner), rendered once on the CPU oracle"""
    s = hc.scene()
    items = idr.items_of_scene(s)
    out = {}
    for W, H in hc.SHAPES:
        for cam in hc.CAMERAS:
            o = oracle_lib.Oracle(W, H, 128)
            try:
                s.load(o)
                hc.uniforms(o, cam)
                o.render()
                out[(W, H, cam)] = hr.slots_of(idr.object_plane(o.visibility().copy(), items), hc.SLOT_BASE)
            finally:
                o.close()
    return out


@pytest.mark.parametrize("W,H", hc.SHAPES[1:], ids=hc.SHAPE_IDS[1:])
def test_the_gpu_tests_frames_are_not_vacuous(oracle_planes, W, H):
    """over the union of the cases the GPU test runs at this shape (two cameras, the sets, radius 1 and 8): selected pixels in every
    corner and on every border, mask transitions across the first tile border both ways, an isolated selected pixel, outline pixels
    that only another tile's pixels cause, a tile that holds outline pixels alone, and an outline over an empty pixel"""
    union = {}
    for cam in hc.CAMERAS:
        slots = oracle_planes[(W, H, cam)]
        for name, flags in hc.SETS.items():
            mask = hr.mask_of(np.stack([np.where(slots < 0, 0xFFFFFFFF, 0), np.where(slots < 0, 0xFFFFFFFF, np.maximum(slots, 0))], axis=-1).astype(np.uint32),
                              flags, [0])                          # (slots as one object's instances: mask_of's own path)
            assert np.array_equal(mask, (slots >= 0) & (flags[np.maximum(slots, 0)] != 0))
            assert mask.any(), "%s / %s selects nothing at %dx%d" % (cam, name, W, H)
            for r in (1, 8):
                for k, v in _conditions(mask, slots < 0, r).items():
                    union[k] = union.get(k, False) or v
    if H <= 32:
        union.pop("across_y")
    missing = sorted(k for k, v in union.items() if not v)
    assert not missing, missing
