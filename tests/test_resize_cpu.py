"""zr_resize / zr_get_extent at the C-ABI boundary, without a GPU: declared, exported, bound, guarded - and refused without a context.
(What the call does is held to a new context's frames on the GPU: tests/test_gpu_resize.py.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("zr_resize", "zr_get_extent")


def _header():
    return open(os.path.join(ROOT, "include", "zelda_render.h")).read()


def test_header_declares_both_calls_in_the_lifetime_block_and_the_abi_stays():
    hdr = _header()
    life = hdr[hdr.index("/* --- lifetime"):hdr.index("/* --- scene submission")]
    assert re.search(r"^int\s+zr_resize\(zr_ctx\* ctx, uint32_t width, uint32_t height\);", life, re.M)
    assert re.search(r"^int\s+zr_get_extent\(zr_ctx\* ctx, uint32_t\* width, uint32_t\* height\);", life, re.M)
    assert "RecreateSwapChain" in life
    assert "#define ZR_ABI_VERSION 7u" in hdr                      # additive: no bump
    for name in ("zr_color_device_ptr", "zr_tiles_device_buffer"):   # documented as stable until zr_destroy OR a resize
        at = hdr.index("int  %s(" % name)
        assert "zr_resize" in hdr[hdr.rfind("\n", 0, hdr.rfind("\n", 0, at)):hdr.index("\n", at)], name


def test_binding_knows_both_calls_and_the_library_exports_them():
    from zeldaengine_amd import abi, engine
    assert set(abi.EXTENT_SIGNATURES) == set(CALLS)
    L = engine.lib()
    for name in CALLS:
        f = getattr(L, name)
        assert f.argtypes == abi.EXTENT_SIGNATURES[name] and f.restype == C.c_int
    assert callable(engine.Renderer.resize) and callable(engine.Renderer.extent)


def test_both_calls_are_defined_once_behind_the_guard_in_a_file_of_their_own():
    csrc = os.path.join(ROOT, "zeldaengine_amd", "csrc")
    text = open(os.path.join(csrc, "zr_resize.cpp")).read()
    assert text.count("\n") <= 752
    for name in CALLS:
        defs = re.findall(r'extern "C" int %s\(([^{;]*)\)\s*\{\s*if \(!c\) return ZR_ERR_ARG;\s*return zr_guard\(' % name, text)
        assert len(defs) == 1, name
    others = "\n".join(open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith(".cpp") and f != "zr_resize.cpp")
    assert not re.search(r'extern "C" int zr_(resize|get_extent)\(', others)
    # the extent's set is made by ONE function, for zr_create and zr_resize alike
    assert "zr_extent_create(c)" in open(os.path.join(csrc, "zr_context.cpp")).read()


def test_no_context_is_an_argument_error():
    from zeldaengine_amd import abi, engine
    L = engine.lib()
    w, h = C.c_uint32(7), C.c_uint32(9)
    assert L.zr_resize(None, 64, 64) == abi.ERR_ARG
    assert L.zr_resize(None, 0, 0) == abi.ERR_ARG
    assert L.zr_get_extent(None, C.byref(w), C.byref(h)) == abi.ERR_ARG and (w.value, h.value) == (7, 9)
