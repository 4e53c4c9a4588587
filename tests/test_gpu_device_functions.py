"""Each device function of csrc/zr_math.h, the vertex stage of zr_dev.h and the BxDF terms / shadow tap of zr_shade.h, one call per case on the
GPU (tests/device_probe/), against the CPU oracle's copy over the tables of tests/device_function_cases.py.

The rule is a condition, not a tolerance: every case is compared and the result words must be equal - the sign of zero, infinities and
denormals included; a NaN matches a NaN of any payload or sign.  A frame is bit-identical to the oracle only because each of these calls
is; whole-frame tests reach them only at the operands their scenes happen to produce.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import device_function_cases as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _probe_build_module():
    spec = importlib.util.spec_from_file_location("device_probe_build", os.path.join(HERE, "device_probe", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class ZpScene(C.Structure):
    _fields_ = [("map", C.c_void_p), ("map_dim", C.c_int32), ("cube", C.c_void_p), ("cube_dim", C.c_uint32), ("lut", C.c_void_p),
                ("view", C.c_void_p), ("SB", C.c_float * 16)]


class Probe:
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.zp_run_scene.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        assert self.L.zp_count() == len(T.PROBE_FUNCTIONS)

    def run(self, name, table, shadow_map=None, scene=None):
        """scene: a device_function_cases.Scene whose oracle() has been called (it holds the oracle's mip chain and decode table)"""
        fn = T.PROBE_FUNCTIONS.index(name)
        table = np.ascontiguousarray(table, dtype=np.uint32)
        assert table.ndim == 2 and table.shape[1] == self.L.zp_words_in(fn), (name, table.shape)
        out = np.zeros((len(table), self.L.zp_words_out(fn)), dtype=np.uint32)
        err = C.c_int(0)
        sc, keep = ZpScene(), []
        if shadow_map is not None:
            keep.append(np.ascontiguousarray(shadow_map, dtype=np.float32))
            sc.map, sc.map_dim = keep[-1].ctypes.data, keep[-1].shape[0]
            sc.SB[:] = list(T.IDENTITY)
        if scene is not None:
            keep += [scene.map, np.concatenate([m.ravel() for m in scene.mips]), scene.lut, np.ascontiguousarray(scene.view), scene.SB]
            sc.map, sc.map_dim = scene.map.ctypes.data, scene.map_dim
            sc.cube, sc.cube_dim, sc.lut = keep[-4].ctypes.data, scene.cube_dim, scene.lut.ctypes.data
            sc.view = keep[-2].ctypes.data
            sc.SB[:] = list(scene.SB)
        rc = self.L.zp_run_scene(fn, table.ctypes.data, out.ctypes.data, len(table), C.byref(sc), C.byref(err))
        assert rc == 0, "probe %s: status %d, HIP error %d" % (name, rc, err.value)
        return out


@pytest.fixture(scope="module")
def probe(gpu_engine):
    """The probe library: rebuilt when stale; a missing library FAILS (gpu_engine's policy).  gpu_engine has loaded torch's HIP runtime by now,
    which the probe binds to by SONAME."""
    b = _probe_build_module()
    lib = b.build()
    assert os.path.exists(lib), "tests/device_probe/_build/libzr_probe.so is missing and did not build"
    return Probe(lib)


def mismatches(name, table, dev, ora, label=None):
    """failure text for function `name`, or None: words equal, or both NaN where the word is a float"""
    fl = np.array(T.FLOAT_WORDS[name], dtype=bool)
    label = label or "zr " + name
    both_nan = np.isnan(dev.view(np.float32)) & np.isnan(ora.view(np.float32)) & fl[None, :]
    bad = np.flatnonzero(((dev != ora) & ~both_nan).any(axis=1))
    if not len(bad):
        return None
    lines = ["%s: %d of %d cases differ" % (label, len(bad), len(table))]
    for i in bad[:6]:
        lines.append("  in %s  device %s  oracle %s" % (" ".join("%08x" % w for w in table[i]), " ".join("%08x" % w for w in dev[i]),
                                                       " ".join("%08x" % w for w in ora[i])))
    return "\n".join(lines)


def check(probe, oracle_lib, names, tables=None):
    fails = []
    for name in names:
        table = getattr(T, T.TABLE_OF.get(name, name))() if tables is None else tables[name]
        assert len(table) <= 250000, name
        m = mismatches(name, table, probe.run(name, table), T.oracle_batch(oracle_lib.lib(), name, table))
        if m:
            print(m)
            fails.append(m)
    assert not fails, "\n".join(fails)


def test_transcendentals(probe, oracle_lib):
    """zr_rsqrt, zr_sincos (its table crosses |k| = 2^31, where a cast of k to int parts ways between x86 and gfx950), zr_exp2 (denormal
    results compared), zr_log2, zr_pow at its call sites' operands, zr_pow5"""
    check(probe, oracle_lib, ["rsqrt", "sincos", "exp2", "log2", "pow", "pow5"])


def test_clamps_and_format_conversions(probe, oracle_lib):
    """zr_saturate / zr_clamp with NaN in each position, zr_unorm at every rounding threshold, all 65 536 half codes, every rounding tie of
    zr_f32_to_f16, the ZR_UNORM8 quotient for all 256 inputs"""
    check(probe, oracle_lib, ["saturate", "clamp", "unorm", "f16_to_f32", "f32_to_f16", "unorm8"])


def test_f32_to_f16_is_numpy_float16(probe):
    t = T.f32_to_f16()
    got = probe.run("f32_to_f16", t)[:, 0]
    x = T.u2f(t[:, 0])
    with np.errstate(all="ignore"):
        want = x.astype(np.float16).view(np.uint16).astype(np.uint32)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.array_equal(got[nan] & 0x7FFF, np.full(int(nan.sum()), 0x7E00, dtype=np.uint32))       # NaN -> the quiet NaN, sign kept


def test_ieee_division_and_sqrt(probe, oracle_lib):
    """'/' and sqrtf as the device compiler expands them under the product's flags: correctly rounded, denormals kept"""
    check(probe, oracle_lib, ["div", "sqrt"])


def test_vector_helpers_fix_one_fma_order(probe, oracle_lib):
    check(probe, oracle_lib, ["dot", "cross", "normalize", "tangent_normal", "mat4_point"])


def test_vertex_stage(probe, oracle_lib):
    """instance_record (k_instance_prep / k_instance_apply), vs_position, vs_normal, vertex_flags + classify, project on what classify lets through"""
    check(probe, oracle_lib, ["instance_record", "vs_position", "vs_normal", "classify", "project"])


def test_bxdf_terms(probe, oracle_lib):
    check(probe, oracle_lib, ["F_Schlick", "Fr_DisneyDiffuse", "V_SmithGGXCorrelated", "D_GGX"])


@pytest.mark.parametrize("dim", [8, 64, 100])
def test_shadow_tap(probe, oracle_lib, dim):
    fails = []
    table = T.shadow_tap(dim)
    for kind, mp in T.shadow_maps(dim).items():
        m = mismatches("shadow_tap", table, probe.run("shadow_tap", table, mp), T.oracle_batch(oracle_lib.lib(), "shadow_tap", table, mp),
                       "shadow_tap[%d, %s]" % (dim, kind))
        if m:
            print(m)
            fails.append(m)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dim", [1, 2, 16])
def test_cube_sample(probe, oracle_lib, dim):
    """textureLod of the reflection cubemap: face ties, the zero vector, NaN, every lod edge, chains of 1, 2 and 5 levels"""
    sc = T.Scene(cube_dim=dim)
    o = sc.oracle(oracle_lib)
    table = T.cube_sample(dim)
    m = mismatches("cube_sample", table, probe.run("cube_sample", table, scene=sc), sc.oracle_batch(o, "cube_sample", table), "cube_sample[%d]" % dim)
    assert not m, m


@pytest.mark.parametrize("dim", [8, 64, 100])
def test_pcf_block(probe, oracle_lib, dim):
    """The PCF block of shade_surface (its ShadowFactor, in a frame without lights) against zo_pcf, over P projected to the interior (both
    column patterns), every edge and corner (the per-texel path), sz at +-1 +- ulp and on the `dist < sz` tie, w zero / negative / denormal,
    on a random map, the cleared map and the all-ties map.  Needing no oracle: wherever the 16-byte pattern path applies it gives the sum
    of the 25 single taps (pcf_taps: shadow_tap called 25 times in the shader's order)."""
    fails = []
    points = T.pcf_points(dim)
    surf = np.zeros((len(points), 23), dtype=np.uint32)
    surf[:, 12:15] = points                                  # P; N, cam and the material are zero: only ShadowFactor is read
    _, _, pattern, _, _ = T.pcf_columns(T.u2f(points)[:, 0], dim)
    for kind, mp in T.shadow_maps(dim).items():
        for wname, w in T.PCF_W.items():
            sc = T.Scene(map_dim=dim, shadow_map=mp, SB=T.pcf_SB(w))
            o = sc.oracle(oracle_lib)
            want = sc.oracle_batch(o, "pcf_taps", points)
            block = probe.run("shade", surf, scene=sc)[:, 9:10]
            taps = probe.run("pcf_taps", points, scene=sc)
            label = "[%d, %s map, w %s]" % (dim, kind, wname)
            for got, what in ((block, "PCF block of shade_surface"), (taps, "25 x shadow_tap")):
                m = mismatches("pcf_taps", points, got, want, what + label)
                if m:
                    print(m)
                    fails.append(m)
            if w == 1.0:
                assert pattern.sum() > 1000 and np.array_equal(block[pattern], taps[pattern]), "pattern path != per-texel path " + label
    assert not fails, "\n".join(fails)


def test_shade_surface(probe, oracle_lib):
    """shade_surface<false> and <true> against zo_shade over surfaces x geometry x masks, for every pair of light counts.  The unmasked
    form equals the oracle; the masked form equals the oracle run with exactly the masked lights, in order; an all-ones mask equals the
    unmasked form bit for bit."""
    fails = []
    shadow = T.shadow_maps(64)["random"]
    for i, (nd, npt, poison) in enumerate(T.SHADE_VIEWS):
        sc = T.Scene(map_dim=64, shadow_map=shadow, cube_dim=16, SB=T.SHADE_SB, view=T.shade_view(nd, npt, roll=i, poison=poison))
        o = sc.oracle(oracle_lib)
        table = T.shade_cases(npt, i)
        ones = T.shade_all_ones(table)
        label = "[nDir %d, nPoint %d%s]" % (nd, npt, ", NaN lights" if poison else "")
        plain = probe.run("shade", table, scene=sc)
        for name, tab, got in (("shade", table, plain), ("shade_masked", table, probe.run("shade_masked", table, scene=sc)),
                               ("shade_masked", ones, probe.run("shade_masked", ones, scene=sc))):
            m = mismatches(name, tab, got, sc.oracle_batch(o, name, tab), "shade_surface<%s>%s" % ("true" if name == "shade_masked" else "false", label))
            if m:
                print(m)
                fails.append(m)
            if tab is ones:
                m = mismatches("shade", tab, got, plain, "all-ones mask vs unmasked " + label)
                if m:
                    fails.append(m)
    assert not fails, "\n".join(fails[:6])
