"""Renderer.update_uniforms' pointer arguments (zeldaengine_amd/engine.py: uniform_arguments) without a GPU.

The arguments are plain integers read from the objects at every call - no pointer object, no cast, no kept address - so each of these
must reach the library as a.ctypes.data (ctypes.addressof for the camera) gives it at the moment of the call: another array, the same
array after reallocation, another camera object, an empty array or None (a null pointer and a count of 0).  The last case sends them
through a C function of zr_update_uniforms' signature (libc's snprintf stands in: it is given the addresses as numbers to print).
"""
import ctypes as C

import numpy as np

from zeldaengine_amd import abi
from zeldaengine_amd.engine import uniform_arguments


def _lights(n):
    return np.zeros(n, dtype=abi.XkLight)


def _want(cam, *arrays):
    out = [C.addressof(cam)]
    for a in arrays:
        out += [a.ctypes.data if a is not None and a.size else None, 0 if a is None else len(a)]
    return tuple(out)


def test_each_argument_is_the_objects_address_now():
    cam = abi.make_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0))
    d, p, s = _lights(1), _lights(16), _lights(2)
    assert uniform_arguments(cam, d, p, s) == _want(cam, d, p, s)
    assert all(isinstance(v, int) for v in uniform_arguments(cam, d, p, s))


def test_another_array_and_another_camera():
    cam, cam2 = abi.make_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0)), abi.make_camera((4.0, 5.0, 6.0), (0.0, 0.0, 1.0))
    d, p, s = _lights(1), _lights(16), _lights(2)
    first = uniform_arguments(cam, d, p, s)
    p2 = p.copy()
    second = uniform_arguments(cam2, d, p2, s)
    assert second == _want(cam2, d, p2, s) and second[0] != first[0] and second[3] != first[3] and second[1] == first[1]
    # a slice and a view with an offset: the address is the view's, the count its length
    v = p[3:9]
    assert uniform_arguments(cam, d, v, s)[3:5] == (p.ctypes.data + 3 * p.itemsize, 6)


def test_the_same_array_after_reallocation():
    cam = abi.make_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0))
    d, s = _lights(1), _lights(2)
    p = _lights(4)
    seen = set()
    for n in (4096, 16, 1 << 16, 3):      # resize in place: the object stays, its buffer moves
        before = uniform_arguments(cam, d, p, s)
        assert before == _want(cam, d, p, s)
        p.resize(n, refcheck=False)
        after = uniform_arguments(cam, d, p, s)
        assert after == _want(cam, d, p, s) and after[4] == n
        seen.add(after[3])
    assert len(seen) > 1, "the buffer never moved: the case shows nothing"


def test_empty_and_none_are_a_null_pointer_and_a_count_of_zero():
    cam = abi.make_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0))
    d = _lights(1)
    for nothing in (None, _lights(0), _lights(4)[:0]):
        a = uniform_arguments(cam, d, nothing, nothing)
        assert a[3:] == (None, 0, None, 0) and a[:3] == (C.addressof(cam), d.ctypes.data, 1)


def test_through_a_c_call_of_the_same_argument_types():
    vp, u32 = C.c_void_p, C.c_uint32
    libc = C.CDLL(None)
    f = libc.snprintf
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, vp, vp, u32, vp, u32, vp, u32]
    cam = abi.make_camera((1.0, 2.0, 3.0), (0.0, 0.0, 0.0))
    d, p = _lights(1), _lights(16)
    buf = C.create_string_buffer(256)
    f(buf, 256, b"%p %p %u %p %u %p %u", *uniform_arguments(cam, d, p, None))
    got = buf.value.decode().split()
    num = lambda t: 0 if t in ("(nil)", "0x0", "0") else int(t, 16)
    assert [num(got[0]), num(got[1]), int(got[2]), num(got[3]), int(got[4]), num(got[5]), int(got[6])] == \
           [C.addressof(cam), d.ctypes.data, 1, p.ctypes.data, 16, 0, 0], got
