"""Overlaying lines without a GPU: the library's host statement of the rule (zr_frame_overlay, context-free host code over
csrc/zr_overlay.h) equals the independent statement (tests/overlay_reference.py: numpy float32, Python integers) byte for byte on every
list of tests/overlay_cases.py, on the CPU oracle's frames of both cameras at both shapes and under both styles; the header's transform
and projection are the oracle's, word for word, over the tables of tests/device_function_cases.py; the walk is the exact rational
line's, rounded to 1/256 pixel with halves upward, half-open along the major axis; a stand-alone program runs the shared header - the
walk with and without its division, the bound at the largest extents - under the sanitizers; the C-ABI carries the entry points in the
public header, the ctypes binding and the built library alike; and the lists put visible, hidden and cleared-depth pixels into the
frames the GPU test renders."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import device_function_cases as T
import highlight_cases as hc
import overlay_cases as oc
import overlay_reference as ovr
from zeldaengine_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
ENTRY_POINTS = ("zr_overlay_set", "zr_overlay_get", "zr_set_overlay_style", "zr_get_overlay_style", "zr_read_color_overlaid",
                "zr_copy_frame_overlaid_async", "zr_set_frame_delta_overlay", "zr_frame_overlay")


def _abi_style(st):
    return abi.make_overlay_style(st["depth_bias"], st["hidden_opacity"])


def _first(a, b):
    return "first difference at %s" % (np.argwhere(a != b)[:1].tolist(),)


@pytest.fixture(scope="module")
def frames(oracle_lib):
    """(W, H, camera) -> (colour (H, W, 4) uint8, depth (H, W) float32, PVM (16,) float32, the lists), rendered once on the CPU oracle"""
    s = hc.scene()
    out = {}
    for W, H in oc.SHAPES:
        for cam in oc.CAMERAS:
            o = oracle_lib.Oracle(W, H, 128)
            try:
                s.load(o)
                hc.uniforms(o, cam)
                o.render()
                mvp = o.get_frame()[0]
                pvm = ovr.pvm_of(mvp["Proj"], mvp["View"], mvp["Model"])
                out[(W, H, cam)] = (o.color().copy(), o.gbuffer(0).copy().astype(np.float32), pvm, oc.lists(pvm, W, H))
            finally:
                o.close()
    return out


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/overlay_check.cpp, which includes csrc/zr_overlay.h alone, under the address and undefined-behaviour sanitizers where this
    machine links them for a stand-alone program (as tests/test_highlight_cpu.py does with its own)"""
    tmp = tmp_path_factory.mktemp("overlay_check")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hello = tmp / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp / "hello")]) == 0):
        sanitize = []
    exe = tmp / "overlay_check"
    subprocess.check_call(["g++"] + flags + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "overlay_check.cpp"), "-o", str(exe)])
    return str(exe), tmp


# ---- the transform and the projection against the oracle's

def test_transform_and_projection_are_the_oracles_word_for_word(oracle_lib, check_exe):
    """zr_ov_point and zr_ov_project of the header (through the stand-alone program) and the reference's own equal zo_mat4_point and
    zo_project bit for bit over the tables of tests/device_function_cases.py, unchanged"""
    exe, tmp = check_exe
    L = oracle_lib.lib()
    for name, mode, table, words in (("mat4_point", "point", T.vectors19(), 4), ("project", "project", T.project(), 3)):
        want = T.oracle_batch(L, name, table)[:, :words]
        src, dst = tmp / (mode + ".in"), tmp / (mode + ".out")
        src.write_bytes(np.ascontiguousarray(table, dtype=np.uint32).tobytes())
        subprocess.check_call([exe, mode, str(src), str(dst)])
        got = np.frombuffer(dst.read_bytes(), dtype=np.uint32).reshape(-1, words)
        nan = np.zeros(want.shape, dtype=bool)
        if mode == "point":
            nan = np.isnan(want.view(np.float32)) & np.isnan(got.view(np.float32))      # (a NaN's payload is not part of the statement)
        assert got.shape == want.shape and (nan | (got == want)).all(), "%s: %s" % (name, _first(np.where(nan, 0, got), np.where(nan, 0, want)))
        f = table.view(np.float32)
        if mode == "point":
            mine = np.stack([ovr.mat4_point(f[i, :16], f[i:i + 1, 16:19])[0] for i in range(len(f))]).view(np.uint32)
            assert (nan | (mine == want)).all(), "the reference's mat4_point: %s" % _first(np.where(nan, 0, mine), np.where(nan, 0, want))
        else:
            for hw, hh in T.PROJECT_TARGETS:
                rows = (f[:, 4] == np.float32(hw)) & (f[:, 5] == np.float32(hh))
                X, Y, z = ovr.project(f[rows, :4], hw, hh)
                mine = np.stack([X.astype(np.int32).view(np.uint32), Y.astype(np.int32).view(np.uint32), z.view(np.uint32)], axis=1)
                zn = np.isnan(z)[:, None] & (np.arange(3) == 2)
                assert (zn | (mine == want[rows])).all(), "the reference's project at (%s, %s)" % (hw, hh)


# ---- zr_frame_overlay against the reference

@pytest.mark.parametrize("W,H", oc.SHAPES, ids=oc.SHAPE_IDS)
def test_host_statement_equals_the_reference(frames, W, H):
    n = 0
    for cam in oc.CAMERAS:
        frame, depth, pvm, lists = frames[(W, H, cam)]
        assert set(lists) == set(oc.LIST_NAMES)
        for name, seg in lists.items():
            for sname, st in oc.STYLES.items():
                got = engine.frame_overlay(frame, depth, pvm, seg, _abi_style(st))
                want = ovr.overlay(frame, depth, pvm, seg, st)
                assert np.array_equal(got, want), "%s/%s/%s: %s" % (cam, name, sname, _first(got, want))
                assert np.array_equal(got[..., 3], frame[..., 3])                                   # A is never changed
                if name == "empty":
                    assert np.array_equal(got, frame)
                else:
                    assert not np.array_equal(got, frame), "%s/%s/%s draws nothing" % (cam, name, sname)
                n += 1
    assert n == 2 * len(oc.LIST_NAMES) * 2


def test_the_order_of_the_list_decides(frames):
    """[red, blue] and [blue, red], half-transparent, over one pixel: different bytes"""
    for key, (frame, depth, pvm, lists) in frames.items():
        rb, br = (engine.frame_overlay(frame, depth, pvm, lists[k]) for k in ("order_rb", "order_br"))
        diff = np.argwhere((rb != br).any(axis=2))
        assert len(diff) == 1, (key, diff.tolist())
        y, x = diff[0]
        assert rb[y, x, 2] > rb[y, x, 0] and br[y, x, 0] > br[y, x, 2]                              # the later colour weighs more


def test_identities_and_the_style(frames):
    frame, depth, pvm, lists = frames[(66, 34, "side")]
    assert np.array_equal(engine.frame_overlay(frame, depth, pvm, ovr.segments([])), frame)           # an empty list
    clear = lists["slopes"].copy()
    clear["rgba"][:, 3] = 0
    assert np.array_equal(engine.frame_overlay(frame, depth, pvm, clear, abi.make_overlay_style(0.0, 255)), frame)      # opacity 0
    # hidden_opacity 255 draws a depth-tested list as its XRAY twin does; XRAY ignores the style
    seg = lists["seams"]
    xr = seg.copy()
    xr["flags"] |= ovr.XRAY
    a = engine.frame_overlay(frame, depth, pvm, seg, abi.make_overlay_style(0.0, 255))
    b = engine.frame_overlay(frame, depth, pvm, xr)
    assert np.array_equal(a, b) and np.array_equal(b, engine.frame_overlay(frame, depth, pvm, xr, abi.make_overlay_style(0.5, 7)))
    # a NaN in the depth plane hides; a bias only ever shows more
    nan_depth = np.full_like(depth, np.nan)
    only_xray = seg[(seg["flags"] & ovr.XRAY) != 0]
    assert len(only_xray) and np.array_equal(engine.frame_overlay(frame, nan_depth, pvm, seg), engine.frame_overlay(frame, depth, pvm, only_xray))
    c0, c1 = {}, {}
    ovr.overlay(frame, depth, pvm, seg, oc.STYLES["default"], c0)
    ovr.overlay(frame, depth, pvm, seg, {"depth_bias": 1e-4, "hidden_opacity": 0}, c1)
    assert not (c0["visible"] & ~c1["visible"]).any() and c0["hidden"].any()
    d = abi.make_overlay_style()
    assert (d.depth_bias, d.hidden_opacity, list(d.reserved)) == (0.0, 0, [0, 0])


# ---- the walk against exact rationals

IDENT = np.eye(4, dtype=np.float32).reshape(16)
WW, WH = 64, 32                    # hw = 32, hh = 16: with PVM = 1 a snapped end (X, Y) is the point ((X / 256 - 32) / 32, (Y / 256 - 16) / 16) exactly


def _seg(Xa, Ya, Xb, Yb, rgba=(255, 255, 255, 255), flags=ovr.XRAY):
    return (Fraction(Xa, 256 * 32) - 1, Fraction(Ya, 256 * 16) - 1, 0.5, Fraction(Xb, 256 * 32) - 1, Fraction(Yb, 256 * 16) - 1, 0.5) + tuple(rgba) + (flags,)


def _covered(rows):
    """the pixels the library's host statement draws for segments given by their snapped ends -> a set of (x, y)"""
    seg = ovr.segments([tuple(float(v) for v in r[:6]) + r[6:] for r in rows])
    black = np.zeros((WH, WW, 4), dtype=np.uint8)
    out = engine.frame_overlay(black, np.ones((WH, WW), dtype=np.float32), IDENT, seg)
    assert np.array_equal(out, ovr.overlay(black, np.ones((WH, WW), dtype=np.float32), IDENT, seg))
    return {(int(x), int(y)) for y, x in np.argwhere(out[..., :3].any(axis=2))}, out


def _exact(Xa, Ya, Xb, Yb):
    """the rule in exact rationals: along the major axis every pixel whose centre lies in [first end, second end); across it the pixel
    that holds the line's crossing of that centre line, rounded to the nearest 1/256 pixel, exact halves to the larger value"""
    dX, dY = Xb - Xa, Yb - Ya
    if dX == 0 and dY == 0:
        return set()
    ymajor = not abs(dX) >= abs(dY)
    a, b = ((Ya, Xa), (Yb, Xb)) if ymajor else ((Xa, Ya), (Xb, Yb))
    if b[0] < a[0]:
        a, b = b, a
    out = set()
    for m in range(WH if ymajor else WW):
        c = 256 * m + 128
        if not a[0] <= c < b[0]:
            continue
        cross = a[1] + Fraction((c - a[0]) * (b[1] - a[1]), b[0] - a[0])
        snapped = (cross + Fraction(1, 2)).__floor__()                 # nearest integer, halves upward
        n = snapped // 256
        if 0 <= n < (WW if ymajor else WH):
            out.add((n, m) if ymajor else (m, n))
    return out


WALKS = [(300, 1000, 9000, 1000), (9000, 1000, 300, 1000),                        # slope 0, both directions
         (1000, 300, 1000, 7000), (1000, 7000, 1000, 300),
         (512, 512, 5632, 5632), (5632, 5632, 512, 512), (512, 5632, 5632, 512), (5632, 512, 512, 5632),      # slope +-1: the tie is X-major
         (640, 640, 5760, 5760), (640, 5760, 5760, 640),                              # ... through pixel centres (128 mod 256)
         (700, 300, 2100, 7900), (2100, 7900, 700, 300), (2100, 300, 700, 7900),      # steeper than 1
         (100, 3000, 16000, 4111), (16000, 3000, 100, 4111), (100, 4111, 16000, 3000),
         (1152, 2000, 3200, 2777), (3200, 2777, 1152, 2000),                          # an end exactly on a pixel centre: the half-open rule
         (1000, 1152, 1777, 3200), (1000, 2000, 3200 + 128, 2100), (1153, 2000, 1407, 2001),      # ... and a segment that holds no centre
         (128, 640, 128 + 512, 641), (128, 640, 128 + 512, 639), (128, 641, 128 + 512, 640),      # exact halves, either sign of dY
         (-3000, -2000, 20000, 9000), (20000, 9000, -3000, -2000), (15000, -500, 15500, 9000)]    # crossing the frame's edges


def test_the_walk_is_the_exact_line_rounded_to_a_256th_halves_upward():
    for w in WALKS:
        got, _ = _covered([_seg(*w)])
        assert got == _exact(*w), (w, sorted(got ^ _exact(*w)))
        rev, _ = _covered([_seg(w[2], w[3], w[0], w[1])])
        assert rev == got, "a segment and its reverse cover different pixels: %s" % (w,)
    assert _covered([_seg(1153, 2000, 1407, 2001)])[0] == set()
    # the tie |dX| = |dY| is X-major: one pixel per column, and the last column is the one whose centre lies ahead of the second end
    got, _ = _covered([_seg(512, 512, 5632, 5632)])
    assert sorted(x for x, _ in got) == list(range(2, 22))
    # exact halves go to the larger value for either sign of dY: (2 k dY + dX) / (2 dX) with dX = 512, k = 256, dY = +-1
    assert _exact(128, 640, 640, 641) == _covered([_seg(128, 640, 640, 641)])[0]
    for dy, want in ((1, 641), (-1, 640)):
        k, dX = 256, 512
        assert 640 + (2 * k * dy + dX) // (2 * dX) == want == (Fraction(640) + Fraction(k * dy, dX) + Fraction(1, 2)).__floor__()


def test_a_chain_covers_its_joint_once():
    half = (255, 255, 255, 128)
    chains = [((300, 1000), (3200, 2900), (6000, 1200)), ((300, 1000), (1152 + 1024, 2944), (7000, 3100)), ((900, 200), (1500, 4224), (2000, 8000)),
              ((300, 300), (4224, 4224), (300, 8000))]
    for a, b, c in chains:
        one, img1 = _covered([_seg(*a, *b, rgba=half)])
        two, img2 = _covered([_seg(*b, *c, rgba=half)])
        both, img = _covered([_seg(*a, *b, rgba=half), _seg(*b, *c, rgba=half)])
        ymaj = [not abs(q[0] - p[0]) >= abs(q[1] - p[1]) for p, q in ((a, b), (b, c))]
        if ymaj[0] == ymaj[1] and ((b[ymaj[0]] - a[ymaj[0]] > 0) == (c[ymaj[0]] - b[ymaj[0]] > 0)):
            assert not one & two, "the joint of %s is covered twice" % ((a, b, c),)                  # same axis, same direction: half-open ends meet
        assert both == one | two
        once = img[..., 0] == 128
        assert once.sum() == len(one ^ two) and (img[..., 0] == 192).sum() == len(one & two)          # a pixel blended twice shows it


# ---- the shared header as a stand-alone program under the sanitizers

def _fnv(a):
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_shared_header_under_the_sanitizers(frames, check_exe):
    """every list of tests/overlay_cases.py, at both shapes, both cameras, alternating styles: the walk with its division from and into
    exactly-sized heap buffers, the kernels' form without one against it tile by tile, the bound's assertions at 8 160 and 16 320 pixels
    a side, the shift counts; its digests are the reference's"""
    exe, tmp = check_exe
    cases = []
    for (W, H, cam), (frame, depth, pvm, lists) in frames.items():
        for i, name in enumerate(oc.LIST_NAMES):
            cases.append((frame, depth, pvm, lists[name], list(oc.STYLES.values())[(i + (cam == "top")) % 2]))
    blob = [np.array([len(cases)], dtype="<u4").tobytes()]
    for frame, depth, pvm, seg, st in cases:
        blob += [np.array([frame.shape[1], frame.shape[0], len(seg)], dtype="<u4").tobytes(), np.array([st["depth_bias"]], dtype="<f4").tobytes(),
                 np.array([st["hidden_opacity"]], dtype="<u4").tobytes(), pvm.astype("<f4").tobytes(), frame.tobytes(), depth.astype("<f4").tobytes(), seg.tobytes()]
    path = tmp / "cases.bin"
    path.write_bytes(b"".join(blob))
    run = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "cases %d failed 0" % len(cases) and len(lines) == len(cases) + 1
    for line, (frame, depth, pvm, seg, st) in zip(lines, cases):
        assert int(line.split("fnv=")[1], 16) == _fnv(ovr.overlay(frame, depth, pvm, seg, st)), line


# ---- the C-ABI

def test_the_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert hasattr(L, name), name
        assert name in abi.OVERLAY_SIGNATURES and getattr(L, name).argtypes == abi.OVERLAY_SIGNATURES[name]
    assert set(ENTRY_POINTS) == set(abi.OVERLAY_SIGNATURES)
    for m in ("overlay_set", "overlay_get", "overlay_style", "read_color_overlaid", "copy_frame_overlaid_async", "set_frame_delta_overlay"):
        assert callable(getattr(engine.Renderer, m))
    assert callable(engine.frame_overlay)
    assert "#define ZR_OVERLAY_XRAY 1u" in hdr and "#define ZR_OVERLAY_MAX_SEGMENTS 16384u" in hdr
    assert (abi.OVERLAY_XRAY, abi.OVERLAY_MAX_SEGMENTS) == (ovr.XRAY, ovr.MAX_SEGMENTS) == (1, 16384)


def test_the_abi_stays_at_version_7_and_the_structs_are_32_and_16_bytes(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == abi.ABI_VERSION == engine.lib().zr_abi_version() == 7
    src = tmp_path / "sizes.c"
    src.write_text('#include "zelda_render.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu", '
                   'sizeof(zr_overlay_segment), offsetof(zr_overlay_segment, b), offsetof(zr_overlay_segment, rgba), offsetof(zr_overlay_segment, flags), '
                   'sizeof(zr_overlay_style), offsetof(zr_overlay_style, depth_bias), offsetof(zr_overlay_style, hidden_opacity), '
                   'offsetof(zr_overlay_style, reserved));return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S, Y = abi.OverlaySegment, abi.OverlayStyle
    assert got == [32, 12, 24, 28, 16, 0, 4, 8] == [C.sizeof(S), S.b.offset, S.rgba.offset, S.flags.offset, C.sizeof(Y), Y.depth_bias.offset, Y.hidden_opacity.offset,
                                                    Y.reserved.offset]
    D = abi.OVERLAY_SEGMENT
    assert (D.itemsize, D.fields["b"][1], D.fields["rgba"][1], D.fields["flags"][1]) == (32, 12, 24, 28) and ovr.SEGMENT == D


def test_the_header_is_plain_cpp_and_shares_the_blend():
    shared = open(os.path.join(CSRC, "zr_overlay.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", shared, re.M)
    assert sorted(includes) == ['"../../include/zelda_render.h"', '"zr_highlight.h"', "<cstddef>", "<cstdint>"] and "__global__" not in shared      # nothing of HIP in it
    assert '#include "zr_highlight.h"' in shared and "zr_hl_blend_px(" in shared and "/ 255" not in shared      # the blend is not restated
    kern = open(os.path.join(CSRC, "zr_overlay.hip")).read()
    assert '#include "zr_overlay.h"' in kern and "atomic" not in kern.replace("No atomics", "")
    for step in ("zr_ov_setup(", "zr_ov_covers(", "zr_ov_depth(", "zr_ov_shade(", "rect_of_pixels(", "rect_has(", "ld_global(", "__ballot(", "__syncthreads_or("):
        assert step in kern, step


def test_refusals_of_the_context_free_function(frames):
    L = engine.lib()
    frame, depth, pvm, lists = frames[(66, 34, "side")]
    seg = lists["slopes"]
    out = np.full_like(frame, 0xA5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    st = abi.make_overlay_style()
    ok = [p(frame), p(depth), 66, 34, p(pvm), p(seg), len(seg), C.byref(st), 16, p(out), out.nbytes]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.zr_frame_overlay(*a)
    assert call(a0=None) == call(a1=None) == call(a4=None) == call(a5=None) == call(a7=None) == call(a9=None) == abi.ERR_ARG
    assert call(a2=0) == call(a3=0) == call(a8=12) == call(a8=20) == call(a10=out.nbytes - 4) == call(a10=out.nbytes + 4) == abi.ERR_ARG
    assert call(a6=abi.OVERLAY_MAX_SEGMENTS + 1) == abi.ERR_ARG
    for bad in (abi.make_overlay_style(-1e-6), abi.make_overlay_style(float("nan")), abi.make_overlay_style(float("inf")), abi.make_overlay_style(0.0, 256),
                abi.OverlayStyle(0.0, 0, (C.c_uint32 * 2)(0, 1))):
        assert call(a7=C.byref(bad)) == abi.ERR_ARG
    flagged = seg.copy()
    flagged["flags"][-1] = 2
    assert call(a5=p(flagged)) == abi.ERR_ARG
    assert (out == 0xA5).all(), "a refused call wrote into the destination"
    assert call() == 0 and np.array_equal(out, ovr.overlay(frame, depth, pvm, seg))
    assert call(a5=None, a6=0) == 0 and np.array_equal(out, frame)


# ---- the GPU test's inputs are not vacuous

@pytest.mark.parametrize("W,H", oc.SHAPES, ids=oc.SHAPE_IDS)
def test_the_gpu_tests_lists_are_not_vacuous(frames, W, H):
    """on the oracle's frames of the two cameras, every list (but the empty one, which is a case because it draws nothing) passes the
    depth test at some pixel, fails it behind geometry at some pixel and is drawn over some pixel of cleared depth; over the lists,
    pixels are drawn in every corner region, on both sides of the first tile seams, and - where there is one - in the partial last tile"""
    drawn = np.zeros((H, W), dtype=bool)
    for name in oc.LIST_NAMES:
        if name == "empty":
            continue
        seen = {"visible": False, "hidden": False, "cleared": False}
        for cam in oc.CAMERAS:
            frame, depth, pvm, lists = frames[(W, H, cam)]
            c = {}
            out = ovr.overlay(frame, depth, pvm, lists[name], oc.STYLES["biased"], c)
            seen["visible"] |= bool(c["visible"].any())
            seen["hidden"] |= bool((c["hidden"] & (depth < 1.0)).any())
            seen["cleared"] |= bool((c["drawn"] & (depth == 1.0)).any())
            drawn |= c["drawn"]
            assert (out != frame).any()
        assert all(seen.values()), (name, seen)
    assert drawn[:4, :4].any() and drawn[:4, -4:].any() and drawn[-4:, :4].any() and drawn[-4:, -4:].any()
    assert drawn[:, 31].any() and drawn[:, 32].any() and drawn[31].any() and drawn[32].any()
    assert drawn[:, W - W % 32:].any() and drawn[H - H % 32:].any()                                   # the partial last tile, both ways
