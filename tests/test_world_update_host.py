"""A world applied as a difference (zr_world_update_json, zr_world_update_file, zr_world_json_diff, zr_livelink_set_incremental) at the
C-ABI boundary, without a GPU: the context-free payload diff, the exports, the layout of zr_world_delta, and the loud failure when no
device is usable."""
import copy
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from zeldaengine_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zr_world_update_json", "zr_world_update_file", "zr_world_json_diff", "zr_livelink_set_incremental")
CAMERA, LIGHTS, SKY, BACKGROUND, OBJECTS = (abi.WORLD_DIFF_CAMERA, abi.WORLD_DIFF_LIGHTS, abi.WORLD_DIFF_SKY, abi.WORLD_DIFF_BACKGROUND,
                                            abi.WORLD_DIFF_OBJECTS)


def _edit(fn):
    w = copy.deepcopy(scenes.sample_world())
    fn(w)
    return json.dumps(w)


def _camera(w):
    w["MainCamera"]["Position"] = [6.0, 4.0, 5.0]


def _light(w):
    w["PointLights"][3]["Color"] = [0.25, 0.5, 0.75]


def _sky(w):
    w["Skydome"]["CubemapFileNames"][4] = "another_Z4.png"


def _background(w):
    w["Background"]["EnableBackground"] = not w["Background"]["EnableBackground"]


def _object_field(w):
    w["Objects"][2]["MaxRadius"] = w["Objects"][2]["MaxRadius"] + 1.0


def _object_order(w):
    w["Objects"].reverse()


def _both(w):
    _camera(w)
    _object_field(w)


CASES = [("camera", _camera, CAMERA), ("light", _light, LIGHTS), ("sky names", _sky, SKY), ("background flag", _background, BACKGROUND),
         ("object field", _object_field, OBJECTS), ("object order", _object_order, OBJECTS), ("camera + object", _both, CAMERA | OBJECTS)]


def test_identical_payloads_do_not_differ():
    from zeldaengine_amd import engine
    a = json.dumps(scenes.sample_world())
    assert engine.world_json_diff(a, a) == 0
    assert engine.world_json_diff(a, json.dumps(scenes.sample_world(), indent=3)) == 0      # (the values, not the text)


@pytest.mark.parametrize("name,fn,bits", CASES, ids=[c[0] for c in CASES])
def test_each_difference_sets_exactly_its_bit(name, fn, bits):
    from zeldaengine_amd import engine
    a = json.dumps(scenes.sample_world())
    assert engine.world_json_diff(a, _edit(fn)) == bits
    assert engine.world_json_diff(_edit(fn), a) == bits
    assert engine.world_json_diff(_edit(fn), _edit(fn)) == 0


def test_the_bits_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    for name, bit in (("CAMERA", CAMERA), ("LIGHTS", LIGHTS), ("SKY", SKY), ("BACKGROUND", BACKGROUND), ("OBJECTS", OBJECTS)):
        assert re.search(r"#define ZR_WORLD_DIFF_%s %du\b" % (name, bit), hdr), name


@pytest.mark.parametrize("side", [0, 1])
def test_a_malformed_side_is_a_parse_error(side):
    from zeldaengine_amd import engine
    good = json.dumps(scenes.sample_world())
    pair = [good, good]
    pair[side] = "{not json"
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.world_json_diff(*pair)
    assert e.value.code == abi.ERR_PARSE
    pair[side] = _edit(lambda w: w.pop("Objects"))                  # well-formed JSON, not a world
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.world_json_diff(*pair)
    assert e.value.code == abi.ERR_PARSE
    d = C.c_uint32(99)
    assert engine.lib().zr_world_json_diff(None, 0, good.encode(), len(good), C.byref(d)) == abi.ERR_ARG and d.value == 99


def test_the_entry_points_are_exported_and_declared():
    from zeldaengine_amd import engine
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        f = getattr(L, name)                                        # (AttributeError: not exported)
        assert f.argtypes is not None and f.restype is C.c_int
    for method in ("world_update_json", "world_update_file", "livelink_set_incremental"):
        assert callable(getattr(engine.Renderer, method))
    assert callable(engine.world_json_diff)
    # a null context is an argument error before anything touches a device
    d = abi.WorldDelta()
    assert L.zr_world_update_json(None, b"{}", 2, C.byref(d), C.sizeof(d)) == abi.ERR_ARG
    assert L.zr_world_update_file(None, None, C.byref(d), C.sizeof(d)) == abi.ERR_ARG
    assert L.zr_livelink_set_incremental(None, 1) == abi.ERR_ARG
    assert d.struct_bytes == 0


def test_the_delta_mirror_has_the_headers_size(tmp_path):
    src = tmp_path / "delta_size.c"
    src.write_text('#include "zelda_render.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu", sizeof(zr_world_delta), offsetof(zr_world_delta, history_items), '
                   'offsetof(zr_world_delta, reserved));return 0;}\n')
    exe = tmp_path / "delta_size"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, hist, res = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    assert size == C.sizeof(abi.WorldDelta) == 48
    assert hist == abi.WorldDelta.history_items.offset and res == abi.WorldDelta.reserved.offset


def test_the_abi_version_and_zr_stats_did_not_move():
    from zeldaengine_amd import engine
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == 7 == abi.ABI_VERSION == engine.lib().zr_abi_version()
    assert C.sizeof(abi.Stats) == 96


def test_no_gpu_means_the_update_fails_loudly():
    """Without a HIP device there is no context to update: the way to zr_world_update_json ends at ZR_ERR_DEVICE, not at a CPU path."""
    import torch
    from zeldaengine_amd import engine
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised here")
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.Renderer(64, 64).world_update_json(json.dumps(scenes.sample_world()))
    assert e.value.code == abi.ERR_DEVICE
