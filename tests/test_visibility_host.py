"""Hiding and showing (zr_object_set_visible, zr_object_set_instance_visibility, zr_object_update_instance_visibility_async,
zr_object_get_visibility) at the C-ABI boundary, without a GPU: exported, declared with argument types, and loud on a null context."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zr_object_set_visible", "zr_object_set_instance_visibility", "zr_object_update_instance_visibility_async",
         "zr_object_get_visibility")


def test_the_four_entry_points_are_exported_and_declared():
    from zeldaengine_amd import abi, engine
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert name in abi.VISIBILITY_SIGNATURES
        f = getattr(L, name)                                        # (AttributeError: not exported)
        assert f.argtypes == abi.VISIBILITY_SIGNATURES[name] and f.restype is C.c_int
    nargs = {n: len(a) for n, a in abi.VISIBILITY_SIGNATURES.items()}
    assert nargs == dict(zip(NAMES, (3, 5, 7, 5)))
    for method in ("object_set_visible", "object_set_instance_visibility", "object_update_instance_visibility_async",
                   "object_get_visibility"):
        assert callable(getattr(engine.Renderer, method))


def test_a_null_context_is_an_argument_error():
    """ZR_ERR_ARG (-1) before anything touches a device."""
    from zeldaengine_amd import engine
    L = engine.lib()
    one = (C.c_uint8 * 4)(1, 0, 1, 0)
    n, ov = C.c_uint32(7), C.c_int(7)
    assert L.zr_object_set_visible(None, 0, 0) == -1
    assert L.zr_object_set_instance_visibility(None, 0, 0, C.cast(one, C.c_void_p), 4) == -1
    assert L.zr_object_update_instance_visibility_async(None, 0, 0, None, C.cast(one, C.c_void_p), 4, None) == -1
    assert L.zr_object_get_visibility(None, 0, C.byref(ov), None, C.byref(n)) == -1
    assert (n.value, ov.value) == (7, 7)


def test_the_abi_version_did_not_move():
    """The exports are additive: ZR_ABI_VERSION stays 7 and zr_stats 96 bytes."""
    from zeldaengine_amd import abi, engine
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == 7 == abi.ABI_VERSION == engine.lib().zr_abi_version()
    assert C.sizeof(abi.Stats) == 96
