"""The C-ABI boundary without a GPU: layouts, exported symbols, loud failure when no device is usable."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_compile_as_c_and_cpp(tmp_path):
    """include/zelda_abi.h carries the static asserts of SURVEY App. B; it must compile as C11 and C++17."""
    src = tmp_path / "t.c"
    src.write_text('#include "zelda_render.h"\nint main(void){return (int)sizeof(XkView) != 35068;}\n')
    for cc, std in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        exe = tmp_path / ("t_" + cc)
        subprocess.check_call([cc, std, "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        assert subprocess.call([str(exe)]) == 0


def test_numpy_mirrors_match_abi():
    from zeldaengine_amd import abi
    assert abi.XkVertex.itemsize == 44 and abi.XkVertex.fields["TexCoord"][1] == 36
    assert abi.XkInstanceData.itemsize == 32 and abi.XkInstanceData.fields["InstanceTexIndex"][1] == 28
    assert abi.XkMeshlet.itemsize == 64 and abi.XkMeshlet.fields["ConeCutoff"][1] == 56
    assert abi.XkView.itemsize == 35068 and abi.XkView.fields["PointLights"][1] == 1248
    assert abi.XkView.fields["LightsCount"][1] == 35040 and abi.XkView.fields["zFar"][1] == 35064
    assert C.sizeof(abi.Config) == 32 and C.sizeof(abi.Camera) == 40 and C.sizeof(abi.Material) == 7 * 16


def test_library_exports_every_declared_symbol():
    """Every zr_* function declared in include/zelda_render.h must be exported by the in-tree .so."""
    from zeldaengine_amd import engine
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    declared = sorted(set(re.findall(r"\b(zr_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 35
    L = engine.lib()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing
    assert os.path.dirname(engine.LIB_PATH).endswith("zeldaengine_amd")       # in-tree, not site-packages


def test_every_status_entry_point_is_defined_once_behind_the_guard():
    """No exception crosses the C-ABI (csrc/zr_ctx.h): every `int zr_*` of include/zelda_render.h has exactly one `extern "C" int`
    definition in csrc/*.cpp, and behind its bare `return ZR_ERR_ARG` argument checks the body is `return zr_guard(...)`.  zr_tile_size is
    the one `int` export that is no status: it returns a constant and cannot throw.  No `_impl` twin is left, and HIPCHK is defined once."""
    csrc = os.path.join(ROOT, "zeldaengine_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".h", ".hip"))}
    cpp = "\n".join(t for f, t in text.items() if f.endswith(".cpp"))
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(zr_[a-z0-9_]+)\s*\(", hdr, re.M)) - {"zr_tile_size"})
    assert len(declared) >= 80
    early = re.compile(r"\s*if \([^;{}]*\) return ZR_ERR_ARG;")
    bad = []
    for name in declared:
        defs = list(re.finditer(r'extern "C" int %s\(([^{;]*)\)\s*\{' % name, cpp))
        if len(defs) != 1:
            bad.append((name, "%d definitions" % len(defs)))
            continue
        body = cpp[defs[0].end():]
        while early.match(body):
            body = body[early.match(body).end():]
        if not body.lstrip().startswith("return zr_guard("):
            bad.append((name, body.lstrip()[:60]))
    assert not bad, bad
    assert not re.findall(r"\b\w+_impl\b", "\n".join(text.values()))
    assert sum(t.count("#define HIPCHK") for t in text.values()) == 1


def test_host_sources_are_split_by_concern_and_share_their_idioms():
    """The host is one translation unit per concern, none longer than 752 lines (zr_host.cpp is gone), and the idioms every update path
    used to spell out exist once: the refusal between the stages of a frame (zr_stage_idle) and the host forms' lane (zr_update_lane);
    so do the steps of delivering a frame."""
    csrc = os.path.join(ROOT, "zeldaengine_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".h"))}
    assert sum(t.count("between the stages of a frame (finish it") for t in text.values()) == 1
    assert sum(t.count("cam_s ? c->cam_s : c->stream") for t in text.values()) == 1
    assert not os.path.exists(os.path.join(csrc, "zr_host.cpp"))
    long = {f: t.count("\n") for f, t in text.items() if f.endswith(".cpp") and t.count("\n") > 752}
    assert not long, long
    # delivering a frame is one path (zr_deliver_host.cpp): one readiness check, one source stage that alone launches the highlight and
    # the filter, one note of a winner-plane reader, one scale_ok - in no more lines than the three files it came from had (246 + 91 + 205)
    cpp = {f: t for f, t in text.items() if f.endswith(".cpp")}
    assert sum(t.count("writes packed tiles, not the frame") for t in text.values()) == 1
    assert sum(t.count("ids_wait = true") for t in text.values()) == 1
    for launcher in ("zr_launch_frame_scale(", "zr_launch_highlight_mask(", "zr_launch_highlight_apply("):
        assert sum(t.count(launcher) for t in cpp.values()) == 1, launcher
    assert sum(t.count("scale_ok(uint32_t") for t in text.values()) == 1
    assert not {"zr_delta_host.cpp", "zr_scale_host.cpp"} & set(text)
    assert text["zr_deliver_host.cpp"].count("\n") + text["zr_highlight_host.cpp"].count("\n") <= 542


def test_kernel_files_share_their_steps():
    """The steps the kernels that draw geometry share exist once (zr_dev.h, zr_raster.h): a work item's record (bin_entry), the empty
    key, a tile's context in tile-relative coordinates; the arms nothing instantiated are gone; the two pass files did not grow."""
    csrc = os.path.join(ROOT, "zeldaengine_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}

    def count(s):
        return sum(t.count(s) for t in text.values())
    assert count("be.counts =") == 1
    assert count("<< 32 | ZR_EMPTY_PRIM") == 1
    assert count("T.px0 = 0") == 1
    assert count("find_object_work(objs, (int)P.n_objects") <= 2
    assert count("k_tile_slow") == 0 and count("vis_clear") == 0
    assert text["zr_shadow.hip"].count("\n") <= 517 and text["zr_camera.hip"].count("\n") <= 842


def test_no_gpu_means_loud_failure_not_fallback():
    """Without a HIP device zr_create fails with ZR_ERR_DEVICE and Renderer raises: there is no CPU path in the product."""
    import torch
    from zeldaengine_amd import engine
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path cannot be exercised here")
    with pytest.raises(engine.ZeldaRenderError) as e:
        engine.Renderer(64, 64)
    assert e.value.code == -2


def test_product_never_imports_the_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkg = os.path.join(ROOT, "zeldaengine_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in text.replace("CPU oracle", "").replace("the oracle", "") or f == "build.py", (dirpath, f)


def test_abi_version_is_one_number_everywhere():
    """include/zelda_render.h, the ctypes binding and the built library must name the same ZR_ABI_VERSION (no GPU needed); zr_stats
    is passed with the caller's size, so its ctypes mirror must be the header's struct."""
    from zeldaengine_amd import abi, engine
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    ver = int(re.search(r"#define ZR_ABI_VERSION (\d+)u", hdr).group(1))
    assert ver == abi.ABI_VERSION
    L = engine.lib()
    assert L.zr_abi_version() == ver
    assert C.sizeof(abi.Stats) == 96                          # ABI version 5 (zr_stats::struct_bytes)
    src = os.path.join(ROOT, "tests", "_stats_size.c")
    try:
        open(src, "w").write('#include "zelda_render.h"\n#include <stdio.h>\nint main(void){printf("%zu", sizeof(zr_stats));return 0;}\n')
        exe = src[:-2]
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        assert int(subprocess.check_output([exe]).decode()) == C.sizeof(abi.Stats)
    finally:
        for f in (src, src[:-2]):
            if os.path.exists(f):
                os.remove(f)


def test_shadow_mode_names_map_to_the_dist_flags():
    from zeldaengine_amd import abi
    assert [abi.dist_flags(abi.shadow_mode(m)) for m in (False, True, "replicated", "split", "tiles")] == [0, 1, 0, 1, 2]
    assert abi.shadow_mode(False, "tiles") == "tiles"
    with pytest.raises(ValueError):
        abi.shadow_mode("bands")
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    assert "#define ZR_DIST_SPLIT_SHADOW 1u" in hdr and "#define ZR_DIST_SHADOW_TILES 2u" in hdr
