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


class ZpSlot(C.Structure):
    _fields_ = [("chain", C.c_void_p), ("bytes", C.c_uint64), ("w", C.c_uint32), ("h", C.c_uint32), ("levels", C.c_uint32), ("texel", C.c_uint32),
                ("constant", C.c_float * 4)]


class ZpTextures(C.Structure):
    _fields_ = [("slot", ZpSlot * 7), ("lut", C.c_void_p), ("image_slot", C.c_int32), ("srgb", C.c_int32)]


class Probe:
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.zp_run_scene.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self.L.zp_run_textures.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
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


    def textures(self, tex, slot=0, srgb=True):
        """the zp_textures of a device_function_cases.Textures whose oracle() has been called: its chains are the oracle's"""
        tx = ZpTextures()
        tx.lut, tx.image_slot, tx.srgb = tex.lut.ctypes.data, slot, int(srgb)
        for s in range(7):
            sl = tx.slot[s]
            sl.constant[:] = [float(v) for v in tex.constants[s]]
            if tex.is_image(s):
                h, w = tex.slots[s].shape[:2]
                sl.chain, sl.bytes, sl.w, sl.h, sl.levels = tex.chains[s].ctypes.data, tex.chains[s].nbytes, w, h, T.levels_of(w, h)
            else:
                sl.texel = int(np.ascontiguousarray(tex.slots[s]).view(np.uint32)[0])
        return tx

    def run_textures(self, name, table, tex, slot=0, srgb=True, expect=0):
        fn = T.PROBE_FUNCTIONS.index(name)
        table = np.ascontiguousarray(table, dtype=np.uint32)
        assert table.ndim == 2 and table.shape[1] == self.L.zp_words_in(fn) and len(table) <= 250000, (name, table.shape)
        out = np.zeros((len(table), self.L.zp_words_out(fn)), dtype=np.uint32)
        err = C.c_int(0)
        tx = tex if isinstance(tex, ZpTextures) else self.textures(tex, slot, srgb)
        rc = self.L.zp_run_textures(fn, table.ctypes.data, out.ctypes.data, len(table), C.byref(tx), C.byref(err))
        assert rc == expect, "probe %s: status %d, HIP error %d" % (name, rc, err.value)
        return out

    def packed_channels(self, slot):
        """the result words of tex_packed that hold slot `slot`, by the product's kSlotPack"""
        first, count = C.c_uint32(0), C.c_uint32(0)
        assert self.L.zp_slot_pack(slot, C.byref(first), C.byref(count)) == 0
        return first.value, count.value


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


# ------------------------------------------------------------------------------------------------ the sampler and the surface stage

def _collect(fails, m):
    if m:
        print(m)
        fails.append(m)


@pytest.mark.parametrize("w,h", T.IMAGE_SETS, ids=["%dx%d" % s for s in T.IMAGE_SETS])
def test_tex_footprint(probe, oracle_lib, w, h):
    """N, lambda and the major axis' derivative: on and 1, 2 ulp around every N^2 breakpoint, the tie (to x), a zero minor axis, lambda on
    every level of the chain, denormal and overflowing products, non-finite derivatives"""
    t = T.tex_footprint(w, h)
    m = mismatches("tex_footprint", t, probe.run("tex_footprint", t), T.oracle_batch(oracle_lib.lib(), "tex_footprint", t), "tex_footprint[%d x %d]" % (w, h))
    assert not m, m


@pytest.mark.parametrize("w,h", T.IMAGE_SETS, ids=["%dx%d" % s for s in T.IMAGE_SETS])
def test_tex_sample_image(probe, oracle_lib, w, h):
    """tex_sample<1> / tex_sample_image on one slot, as sRGB and as UNORM, over the image set's coordinates and footprints; a slot that
    holds no image takes the constant arm"""
    fails = []
    t = T.tex_cases(w, h)
    for srgb in (True, False):
        tex, slot = T.single_image(w, h, srgb)
        o = tex.oracle(oracle_lib)
        _collect(fails, mismatches("tex_image", t, probe.run_textures("tex_image", t, tex, slot, srgb), tex.oracle_image(o, slot, t, srgb),
                                   "tex_sample_image[%d x %d, %s]" % (w, h, "sRGB" if srgb else "UNORM")))
        if (w, h) == (2, 2):
            c = t[:64]
            _collect(fails, mismatches("tex_image", c, probe.run_textures("tex_image", c, tex, 5, False), tex.oracle_image(o, 5, c, False), "constant arm"))
        o.close()
    assert not fails, "\n".join(fails)


MATERIALS = {"one_size_128x4": lambda: T.material_one_size(128, 4), "one_size_33x7": lambda: T.material_one_size(33, 7),
             "one_size_16384x1": lambda: T.material_one_size(16384, 1), "three_sizes": T.material_three_sizes, "lead_not_zero": T.material_lead_not_zero}


@pytest.mark.parametrize("which", list(MATERIALS))
def test_tex_sample_material(probe, oracle_lib, which):
    """tex_sample_material's grouping by image size: one turn, two (led by slot 1, slot 0 constant) and three, constant slots between"""
    tex = MATERIALS[which]()
    o = tex.oracle(oracle_lib)
    t = T.material_cases(tex)
    m = mismatches("tex_material", t, probe.run_textures("tex_material", t, tex), tex.oracle_material(o, t), "tex_sample_material[%s]" % which)
    o.close()
    assert not m, m


def _packed_from_material(probe, mat):
    """the 13 channels tex_packed gives, picked from the seven slots' samples by the product's table"""
    out = np.zeros((len(mat), 13), dtype=np.uint32)
    for s in range(7):
        first, count = probe.packed_channels(s)
        out[:, first:first + count] = mat[:, 4 * s:4 * s + count]
    return out


@pytest.mark.parametrize("which", ["one_size_128x4", "one_size_33x7", "one_size_16384x1"])
def test_tex_sample_packed(probe, oracle_lib, which):
    """tex_sample_packed (16-byte texels laid out by kSlotPack) against the oracle's per-slot samples, channel by channel; a packed form
    over images of two sizes is refused, as the product's host never builds one"""
    tex = MATERIALS[which]()
    o = tex.oracle(oracle_lib)
    t = T.material_cases(tex)
    m = mismatches("tex_packed", t, probe.run_textures("tex_packed", t, tex), _packed_from_material(probe, tex.oracle_material(o, t)), "tex_sample_packed[%s]" % which)
    o.close()
    assert not m, m
    if which == "one_size_33x7":
        mixed = T.material_three_sizes()
        mixed.oracle(oracle_lib).close()
        probe.run_textures("tex_packed", t[:8], mixed, expect=-1)


@pytest.mark.parametrize("which", ["one_size_128x4", "one_size_33x7"])
def test_three_sampler_forms_agree(probe, oracle_lib, which):
    """tex_sample_image slot by slot, tex_sample_material and tex_sample_packed on the one-size material: device against device, word for
    word (and each against the oracle in the tests above, so a disagreement says which side moved)"""
    fails = []
    tex = MATERIALS[which]()
    tex.oracle(oracle_lib).close()
    t = T.material_cases(tex)
    mat = probe.run_textures("tex_material", t, tex)
    pk = probe.run_textures("tex_packed", t, tex)
    for s in range(7):
        img = probe.run_textures("tex_image", t, tex, s, s == 0)
        _collect(fails, mismatches("tex_image", t, mat[:, 4 * s:4 * s + 4], img, "tex_sample_material vs tex_sample_image, slot %d" % s))
    _collect(fails, mismatches("tex_packed", t, pk, _packed_from_material(probe, mat), "tex_sample_packed vs tex_sample_material"))
    assert not fails, "\n".join(fails)


def test_sampler_refuses_what_the_host_refuses(probe, oracle_lib):
    tex, slot = T.single_image(2, 2, True)
    tex.oracle(oracle_lib).close()
    t = T.tex_cases(2, 2)[:8]
    for field, value in (("w", 0), ("h", 16385), ("levels", 17), ("levels", 1), ("bytes", 16)):
        tx = probe.textures(tex, slot, True)
        setattr(tx.slot[slot], field, value)
        probe.run_textures("tex_image", t, tx, expect=-1)


def test_barycentrics_and_interpolation(probe, oracle_lib):
    """bary_screen over set-ups made of project()'s results (quad partners included; rw sums 0, denormal, huge), bary_homog over
    clip_vertices() (w <= 0 corners, a zero denominator), interp1 / interp3, model_point with and without the identity short cut"""
    L = oracle_lib.lib()
    check(probe, oracle_lib, ["bary_screen", "bary_homog", "interp", "model_point"],
          {"bary_screen": T.bary_screen(L), "bary_homog": T.bary_homog(), "interp": T.vectors12(), "model_point": T.model_point()})


def test_compute_normal(probe, oracle_lib):
    """ComputeNormal with the determinant of the UV derivatives 0 (constant and collinear UVs), denormal, of either sign; T parallel to N;
    fragN zero, denormal, non-finite; the default normal map"""
    check(probe, oracle_lib, ["compute_normal"])


def test_half_conversions_by_the_conversion_unit(probe, oracle_lib):
    """f32_to_f16_hw / f16_to_f32_hw (the hardware conversions resolve_pixel and the lighting pass use) against the integer spelling"""
    check(probe, oracle_lib, ["f32_to_f16_hw", "f16_to_f32_hw"])


def test_a_constant_image_is_filtered_not_collapsed(probe, oracle_lib):
    """A slot that holds an image whose texels are all equal (a texture update may leave one) is filtered by the kernels like any image:
    equal bits with the oracle run with as_image (the N-tap average of N equal texels, NaN for a NaN coordinate), over every N - and
    not, on the cases the oracle itself shows to differ, the collapsed texel (oracle/CONTRACT.md, "a constant image")."""
    fails, moved = [], 0
    t = T.constant_image_cases()
    for code in T.CONSTANT_CODES:
        tex, filtered, collapsed = T.constant_image(code, oracle_lib, t)
        dev = probe.run_textures("tex_image", t, tex, 0, True)
        _collect(fails, mismatches("tex_image", t, dev, filtered, "constant image of code %d, filtered" % code))
        both_nan = np.isnan(dev.view(np.float32)) & np.isnan(collapsed.view(np.float32))
        moved += int(((dev != collapsed) & ~both_nan).any(axis=1).sum())
    assert not fails, "\n".join(fails)
    assert moved > 0, "the device gave the collapsed texel everywhere: the tables no longer tell the two rules apart"
