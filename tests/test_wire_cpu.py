"""The wireframe without a GPU: the host statement (zr_frame_wire, csrc/zr_wire.h) held to the exact-rational statement of
tests/wire_reference.py on the table of tests/wire_cases.py; the stand-alone program tests/wire_check.cpp under the sanitizers; the
style's layout, its numpy and ctypes mirrors, the constants, and every refusal of the context-free call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import wire_cases
import wire_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
UNDECIDED_CAP = 1.0 / 10000.0         # of the pixel-edge pairs, on the reference's side alone


@pytest.fixture(scope="module")
def table():
    """every case with the reference's answer, computed once"""
    out = []
    for c in wire_cases.cases():
        want, verdict, stats = R.frame(c["img"], c["prim"], c["corners"], c["style"], c["selected"])
        out.append((c, want, verdict, stats))
    return out


def test_the_table_covers_what_it_claims(table):
    """Each class is present; every width occurs with both verdicts; exact ties occur where the table places them (and the <= turns
    them on); the undecided pairs stay within the cap on the reference's side alone."""
    from zeldaengine_amd import abi
    classes = {c["cls"] for c, _, _, _ in table}
    assert classes == set(wire_cases.CLASSES)
    assert min(wire_cases.WIDTHS) == 1 and max(wire_cases.WIDTHS) == abi.WIRE_WIDTH_MAX      # the style's whole range of widths
    assert all(c["style"]["flags"] in (0, abi.WIRE_SELECTED) for c, _, _, _ in table)
    for width in wire_cases.WIDTHS:
        seen = set()
        for c, _, verdict, _ in table:
            if c["style"]["width_256"] == width:
                seen |= set(np.unique(verdict[c["prim"] < len(c["corners"])]).tolist())
        assert {R.ON, R.OFF} <= seen, (width, seen)
    for cls in ("tie_axis", "tie_345"):
        for width in wire_cases.WIDTHS:
            ties = sum(s["ties"] for c, _, _, s in table if c["cls"] == cls and c["style"]["width_256"] == width)
            assert ties > 0, (cls, width)
    assert any(c["selected"] is None for c, _, _, _ in table if c["cls"] == "selected")
    assert any(c["selected"] is not None and c["style"]["flags"] for c, _, _, _ in table)
    assert any((c["prim"] >= len(c["corners"])).any() and (c["prim"] < len(c["corners"])).any() for c, _, _, _ in table)
    assert any(not np.isfinite(c["corners"]).all() for c, _, _, _ in table)
    assert any((c["corners"][..., 2] < 0).any() for c, _, _, _ in table if c["cls"] == "wneg")
    pairs = sum(s["pairs"] for _, _, _, s in table)
    undecided = sum(s["undecided_pairs"] for _, _, _, s in table)
    print("pairs %d, undecided %d, ties %d" % (pairs, undecided, sum(s["ties"] for _, _, _, s in table)))
    assert pairs > 10000 and undecided <= UNDECIDED_CAP * pairs


def test_frame_wire_equals_the_exact_statement(table):
    """Every pixel that the reference decides is equal in every byte: blended where it is on the wire, untouched elsewhere."""
    from zeldaengine_amd import abi, engine
    for c, want, verdict, _ in table:
        st = abi.make_wire_style(**c["style"])
        got = engine.frame_wire(c["img"], c["prim"], c["corners"], st, c["selected"])
        decided = verdict != R.UNDECIDED
        bad = np.argwhere((got != want).any(axis=2) & decided)
        assert len(bad) == 0, (c["name"], bad[:5].tolist())
        und = ~decided
        if und.any():      # an undecided pixel is still one of the two
            for y, x in np.argwhere(und):
                assert got[y, x].tolist() in (c["img"][y, x].tolist(), R.blend_pixel(c["img"][y, x], c["style"]["rgba"])), (c["name"], int(x), int(y))
        assert np.array_equal(got[..., 3], c["img"][..., 3]), c["name"]


def test_blend_is_the_highlights(table):
    """A pixel on the wire is engine.frame_highlight's fill of the same colour: one blend, not a second one."""
    from zeldaengine_amd import abi, engine
    c, want, verdict, _ = next(t for t in table if t[0]["name"] == "random_w1024_0")
    rgba = c["style"]["rgba"]
    got = engine.frame_wire(c["img"], c["prim"], c["corners"], abi.make_wire_style(**c["style"]), c["selected"])
    on = (verdict == R.ON) | ((verdict == R.UNDECIDED) & (got != c["img"]).any(axis=2))
    hl = engine.frame_highlight(c["img"], on, abi.make_highlight_style(outline=(0, 0, 0, 0), fill=rgba, radius=0))
    assert (verdict == R.ON).any() and np.array_equal(hl, got) and np.array_equal(hl[verdict != R.UNDECIDED], want[verdict != R.UNDECIDED])


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/wire_check.cpp, which includes csrc/zr_wire.h alone, under the address and undefined-behaviour sanitizers where this
    machine links them for a stand-alone program (as tests/test_overlay_cpu.py does with its own)"""
    tmp = tmp_path_factory.mktemp("wire_check")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hello = tmp / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp / "hello")]) == 0):
        sanitize = []
    exe = tmp / "wire_check"
    subprocess.check_call(["g++"] + flags + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "wire_check.cpp"), "-o", str(exe)])
    return str(exe)


def test_stand_alone_program_under_the_sanitizers(check_exe):
    """The style check, zr_wire_frame's bounds on 1 x 1, 1 x N and N x 1 frames (exactly-sized heap arrays), the edge order, and
    dst == blend only where the rule says so."""
    run = subprocess.run([check_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "wire_check failed 0"


def test_style_layout_mirrors_and_constants(tmp_path):
    from zeldaengine_amd import abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zelda_render.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u %u %u %u %u\\n", '
                   'sizeof(zr_wire_style), offsetof(zr_wire_style, rgba), offsetof(zr_wire_style, width_256), offsetof(zr_wire_style, flags), '
                   'offsetof(zr_wire_style, reserved), ZR_WIRE_SELECTED, ZR_WIRE_WIDTH_MAX, ZR_STAGE_WIRE, ZR_STAGE_HIGHLIGHT, ZR_STAGE_OVERLAY);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S, N = abi.WireStyle, abi.WIRE_STYLE
    assert got[:5] == [16, 0, 4, 8, 12] == [C.sizeof(S), S.rgba.offset, S.width_256.offset, S.flags.offset, S.reserved.offset]
    assert [N.itemsize] + [N.fields[k][1] for k in ("rgba", "width_256", "flags", "reserved")] == got[:5]
    assert got[5:] == [abi.WIRE_SELECTED, abi.WIRE_WIDTH_MAX, abi.STAGE_WIRE, abi.STAGE_HIGHLIGHT, abi.STAGE_OVERLAY] == [1, 4096, 1, 2, 4]
    d = abi.make_wire_style()
    assert (list(d.rgba), d.width_256, d.flags, d.reserved) == ([0, 0, 0, 255], 256, 0, 0)
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    assert int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1)) == 7      # additive: the version stays


def test_every_refusal_of_the_context_free_call():
    from zeldaengine_amd import abi, engine
    L = engine.lib()
    W, H = 4, 3
    img = np.zeros((H, W, 4), dtype=np.uint8); prim = np.zeros((H, W), dtype=np.uint32); out = np.zeros_like(img)
    cor = np.zeros((2, 9), dtype=np.float32); sel = np.zeros(2, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(img_=img, prim_=prim, w=W, h=H, cor_=cor, n=2, sel_=sel, st=None, st_bytes=16, out_=out, nbytes=None):
        st = st or abi.make_wire_style()
        return L.zr_frame_wire(p(img_) if img_ is not None else None, p(prim_) if prim_ is not None else None, w, h, p(cor_) if cor_ is not None else None, n,
                               p(sel_) if sel_ is not None else None, C.byref(st), st_bytes, p(out_) if out_ is not None else None,
                               out.nbytes if nbytes is None else nbytes)
    assert call() == 0 and call(sel_=None) == 0 and call(cor_=None, n=0) == 0
    ARG = -1
    assert engine.ZeldaRenderError(ARG, "").code == ARG
    for kw in (dict(img_=None), dict(prim_=None), dict(out_=None), dict(w=0), dict(h=0), dict(cor_=None), dict(st_bytes=12), dict(st_bytes=20),
               dict(nbytes=out.nbytes - 4), dict(nbytes=out.nbytes + 4)):
        assert call(**kw) == ARG, kw
    for bad in (dict(width_256=0), dict(width_256=4097), dict(flags=2), dict(flags=0x80000001)):
        assert call(st=abi.make_wire_style(**bad)) == ARG, bad
    st = abi.make_wire_style(); st.reserved = 1
    assert call(st=st) == ARG
    for ok in (dict(width_256=1), dict(width_256=4096), dict(flags=1)):
        assert call(st=abi.make_wire_style(**ok)) == 0, ok
    assert L.zr_frame_wire(p(img), p(prim), W, H, p(cor), 2, None, None, 16, p(out), out.nbytes) == ARG
