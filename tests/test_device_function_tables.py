"""CPU side of the per-call device-function tests (tests/test_gpu_device_functions.py compares the GPU with the oracle over the same tables):

(a) the tables' own coverage claims, so that a table which silently loses an edge fails here;
(b) the oracle's batch exports against its scalar ones;
(c) the oracle against float64 (numpy) on the same tables, with the bounds csrc/zr_math.h and tests/test_oracle_kat.py state inside each
    function's documented domain, and the measured figures of DESIGN.md section 4 where a table goes beyond it;
(d) the shape of the probe's sources: it defines no zr_* function of its own and is compiled with the product's flags.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import device_function_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered in cast")       # signalling NaNs widened to float64 on purpose


@pytest.fixture(scope="module")
def L(oracle_lib):
    return oracle_lib.lib()


def _f(L, name, table):
    return T.u2f(T.oracle_batch(L, name, table))


# ------------------------------------------------------------------------------------------------------------------ (a) coverage

def test_generic_table_holds_every_kind_of_float():
    g = T.generic()
    assert len(g) == 2 * 256 * 72 and len(np.unique(g >> 23)) == 512          # both signs x every exponent
    x = T.u2f(g)
    assert np.isnan(x).any() and np.isinf(x).any() and (g == 0).any() and (g == 0x80000000).any()
    assert ((g & 0x7F800000 == 0) & (g & 0x7FFFFF != 0)).sum() >= 2 * 70       # denormals
    assert ((g & 0x7FC00000) == 0x7F800000).sum() > 2 and T.NAN_S in T.SPECIALS  # signalling NaNs


def test_sincos_table_crosses_the_casts_range_on_both_signs():
    x = T.sincos()[:, 0]
    k = T.sincos_k(x).astype(np.float64)
    fin = np.isfinite(k)
    for sgn in (1.0, -1.0):
        kk = np.unique(sgn * k[fin])
        assert (kk == 2.0 ** 31).any() and (kk == 2.0 ** 31 - 128).any(), "k = 2^31 and its float predecessor"
        assert ((kk > 2.0 ** 31) & (kk < 2.0 ** 32)).any() and (kk >= 2.0 ** 33).any()
        assert all((kk == q).any() for q in range(65)) and (kk == 2.0 ** 24).any()
    assert set(np.unique(k[fin & (np.abs(k) < 2.0 ** 24)] % 4)) == {0.0, 1.0, 2.0, 3.0}


def test_exp2_log2_pow_tables_hold_their_breakpoints():
    e = T.u2f(T.exp2()[:, 0])
    assert all((e == v).any() for v in np.arange(-127.0, 128.5, 0.5)) and (e == np.nextafter(np.float32(-126), np.float32(-200))).any()
    lg = T.log2()[:, 0]
    s = int(T.f2u(np.float32(1.41421356237))[0])
    assert all((lg == s + d).any() for d in (-1, 0, 1)) and (lg == 1).any() and (lg == 0x00800000).any() and (lg == 0x007FFFFF).any()
    p = T.u2f(T.pow_())
    assert ((p[:, 0] == 0) & (p[:, 1] == 0)).any(), "pow(0, 0)"
    assert len(np.unique(p[:, 1])) == 257 and (np.isnan(p[:, 0]) | np.isinf(p[:, 0]) | (p[:, 0] < 0)).any()


def test_clip_tables_reach_both_sides_of_every_plane(L):
    tri = T.classify()
    r = T.oracle_batch(L, "classify", tri)[:, 0]
    assert set(np.unique(r)) == {0, 1, 2}
    v = T.u2f(T.clip_vertices())
    w1 = v[v[:, 3] == 1.0]
    for col in (0, 1):
        for edge in (1.0, -1.0, 4.0, -4.0):
            e = np.float32(edge)
            assert all((w1[:, col] == t).any() for t in (np.nextafter(e, np.float32(9)), e, np.nextafter(e, np.float32(-9))))
    assert (v[:, 3] == 0).any() and (T.clip_vertices()[:, 3] == 0x80000000).any() and (T.clip_vertices()[:, 3] == 1).any() and (v[:, 3] < 0).any()
    # project()'s table: exactly the vertices a fast-path triangle may hold - with two inside corners the oracle classifies each as 1 -
    # and the edge of that set (on the guard band, z = 0) is among them
    p = T.project()
    inside = np.tile(np.array([0, 0, 0x3F000000, 0x3F800000], dtype=np.uint32), (len(p), 1))
    assert (T.oracle_batch(L, "classify", np.concatenate([p[:, :4], inside, inside], axis=1))[:, 0] == 1).all()
    pv = T.u2f(p[:, :4])
    assert ((np.abs(pv[:, 0]) == np.float32(4) * pv[:, 3]).any() and (p[:, 2] == 0).any() and (p[:, 2] == 0x80000000).any())
    assert not T.projectable(T.clip_vertices()).all()


def test_shadow_tap_tables_reach_edges_ties_and_both_outcomes(L):
    for dim in (8, 64, 100):
        t = T.shadow_tap(dim)
        x = T.u2f(t)
        u = x[:, 0].astype(np.float64) * dim - 0.5
        assert (u < 0).any() and (u > dim - 1).any() and ((u > 1) & (u < dim - 2)).any()         # clamped on both sides, and interior
        for v in (1.0, -1.0):
            assert all((x[:, 2] == np.nextafter(np.float32(v), np.float32(s))).any() for s in (-9, 9)) and (x[:, 2] == v).any()
        assert (x[:, 2] == T.SHADOW_TIE).any() and (x[:, 3] == 0).any() and (x[:, 3] < 0).any() and (t[:, 3] == 1).any()
        maps = T.shadow_maps(dim)
        assert (maps["tie"] == T.SHADOW_TIE).all() and (maps["cleared"] == 1).all()
        r = T.u2f(T.oracle_batch(L, "shadow_tap", t, maps["random"]))[:, 0]
        assert set(np.unique(r)) == {np.float32(0.1), np.float32(1.0)}


# ------------------------------------------------------------------------------------------------------------------ (b) batch = scalar

def test_batch_exports_are_the_scalar_ones(L):
    rng = np.random.default_rng(5)

    def sample(t, n=1500):
        return t[np.sort(rng.choice(len(t), min(n, len(t)), replace=False))]

    def same(a, b):
        a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
        return np.array_equal(a.view(np.uint32)[~(np.isnan(a) & np.isnan(b))], b.view(np.uint32)[~(np.isnan(a) & np.isnan(b))])

    for name, scalar in (("rsqrt", L.zo_kat_rsqrt), ("exp2", L.zo_kat_exp2), ("log2", L.zo_kat_log2), ("pow", L.zo_kat_pow), ("D_GGX", L.zo_kat_D_GGX),
                         ("V_SmithGGXCorrelated", L.zo_kat_V_SmithGGXCorrelated), ("F_Schlick", L.zo_kat_F_Schlick),
                         ("Fr_DisneyDiffuse", L.zo_kat_Fr_DisneyDiffuse)):
        t = sample(getattr(T, T.TABLE_OF.get(name, name))())
        t = t[~np.isnan(T.u2f(t)).any(axis=1)]             # a float argument passed by value may not keep a signalling NaN's bits
        assert same(_f(L, name, t)[:, 0], [scalar(*[float(v) for v in row]) for row in T.u2f(t)]), name
    t = sample(T.sincos())
    out = (C.c_float * 2)()
    want = []
    for x in T.u2f(t)[:, 0]:
        L.zo_kat_sincos(float(x), out)
        want.append((out[0], out[1]))
    assert same(_f(L, "sincos", t), want)
    t = sample(T.f32_to_f16())
    t = t[~np.isnan(T.u2f(t))[:, 0]]
    assert np.array_equal(T.oracle_batch(L, "f32_to_f16", t)[:, 0], [L.zo_kat_f32_to_f16(float(x)) for x in T.u2f(t)[:, 0]])
    t = sample(T.instance_record(), 500)
    rec = T.oracle_batch(L, "instance_record", t)
    r9 = np.zeros(9, dtype=np.float32)
    for row, got in zip(t, rec):
        e = np.ascontiguousarray(T.u2f(row[3:6]))
        L.zo_kat_rotmat(e.ctypes.data_as(C.c_void_p), r9.ctypes.data_as(C.c_void_p))
        assert same(T.u2f(got[:9]), r9) and np.array_equal(got[9:12], row[0:3]) and got[12] == row[6] and not got[13:].any()


# ------------------------------------------------------------------------------------------------------------------ (c) oracle vs float64

def _finite_rows(t):
    return t[np.isfinite(T.u2f(t)).all(axis=1)]


def test_rsqrt_against_float64(L):
    t = T.rsqrt()
    x = T.u2f(t)[:, 0]
    ok = np.isfinite(x) & (x >= np.float32(1.17549435e-38))
    got = _f(L, "rsqrt", t)[:, 0]
    ref = 1.0 / np.sqrt(x[ok].astype(np.float64))
    ulp = 2.0 ** (np.frexp(ref)[1] - 24)
    assert (np.abs(got[ok] - ref) / ulp).max() < 1.2
    rest = got[~ok & ~np.isnan(x)]
    assert np.isnan(got[np.isnan(x)]).all() and ((rest == np.inf) | ((rest == 0) & (x[~ok & ~np.isnan(x)] == np.inf))).all()


def sincos_worst(L, lo, hi):
    x = T.u2f(T.sincos())[:, 0]
    m = np.isfinite(x) & (np.abs(x) >= lo) & (np.abs(x) < hi)
    got = _f(L, "sincos", T.sincos()[m])
    x64 = x[m].astype(np.float64)
    return len(x64), max(np.abs(got[:, 0] - np.sin(x64)).max(), np.abs(got[:, 1] - np.cos(x64)).max())


# |x| range -> the absolute error bound asserted there.  3e-7 is the documented bound (csrc/zr_math.h, test_oracle_kat.py: to 700); the
# measured worst over this table is below 1e-7 in every row, so the documented figure is asserted to the end of the
# domain and a decade past it.  Beyond, the only statement is the GPU test's: device and oracle give the same bits.
SINCOS_BOUNDS = [(0.0, 700.0, 3e-7), (700.0, 1e4, 3e-7), (1e4, 1.1e5, 3e-7)]


@pytest.mark.parametrize("lo,hi,bound", SINCOS_BOUNDS)
def test_sincos_against_float64(L, lo, hi, bound):
    n, worst = sincos_worst(L, lo, hi)
    print("sincos |x| in [%g, %g): %d cases, worst %.3g" % (lo, hi, n, worst))
    assert n >= 100 and worst < bound


def test_exp2_log2_pow_against_float64(L):
    x = T.u2f(T.exp2())[:, 0]
    got = _f(L, "exp2", T.exp2())[:, 0].astype(np.float64)
    m = np.isfinite(x) & (x >= -126) & (x < 128)
    assert (np.abs(got[m] / np.exp2(x[m].astype(np.float64)) - 1.0)).max() < 4e-7           # normal results: the documented bound
    assert (got[np.isfinite(x) & (x < -126)] == 0).all() and (got[x >= 128] == np.inf).all() and np.isnan(got[np.isnan(x)]).all()
    x = T.u2f(T.log2())[:, 0]
    got = _f(L, "log2", T.log2())[:, 0].astype(np.float64)
    m = np.isfinite(x) & (x > 0)                                                            # denormals included
    ref = np.log2(x[m].astype(np.float64))
    assert (np.abs(got[m] - ref) / np.maximum(1.0, np.abs(ref))).max() < 4e-7
    assert (got[x == 0] == -np.inf).all() and np.isnan(got[x < 0]).all() and (got[x == np.inf] == np.inf).all()
    p = T.u2f(T.pow_())
    got = _f(L, "pow", T.pow_())[:, 0].astype(np.float64)
    b, e = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        ref = b ** e
    m = np.isfinite(b) & (b > 0) & (ref >= 2.0 ** -126) & (ref < 2.0 ** 127)
    # 3e-6 is the documented bound (test_oracle_kat.py: exponent 0.4545 on [0, 12]).  It holds wherever |y log2 x| <= 16, which covers both
    # call sites' ordinary operands.  The gamma table runs over every positive float, |y log2 x| up to 58; there the rounding of the
    # product y * log2 x (half an ulp of a number up to 64) adds up to 1.3e-6: measured worst 3.1e-6, DESIGN.md section 4 states 4e-6.
    t_abs = np.abs(e * np.log2(np.where(m, b, 1.0)))
    for lo, hi, bound in ((0.0, 16.0, 3e-6), (16.0, 64.0, 4e-6)):
        sel = m & (t_abs >= lo) & (t_abs < hi)
        worst = (np.abs(got[sel] / ref[sel] - 1.0)).max()
        print("pow |y log2 x| in [%g, %g): %d cases, worst %.3g" % (lo, hi, sel.sum(), worst))
        assert sel.sum() > 1000 and worst < bound
    z = (b == 0) & (e > 0)
    assert (got[z] == 0).all() and np.isnan(got[(b < 0)]).all()


def test_f16_conversions_are_exact(L):
    codes = T.f16_codes()
    got = _f(L, "f16_to_f32", codes)[:, 0]
    want = codes[:, 0].astype(np.uint16).view(np.float16).astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)) and np.isnan(got[nan]).all()
    t = T.f32_to_f16()
    x = T.u2f(t)[:, 0]
    with np.errstate(all="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = T.oracle_batch(L, "f32_to_f16", t)[:, 0]
    assert np.array_equal(got[~np.isnan(x)], want[~np.isnan(x)])
    q = _f(L, "unorm8", T.unorm8())[:, 0]
    assert np.array_equal(q, T.unorm8_quotients())


def test_division_sqrt_and_unorm_are_the_ieee_results(L):
    t = T.div()
    a, b = T.u2f(t)[:, 0].astype(np.float64), T.u2f(t)[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        want = (a / b).astype(np.float32)         # float64 quotient of two floats rounds to the correctly rounded float (no double rounding: 53 >= 2 * 24 + 2)
    got = _f(L, "div", t)[:, 0]
    nan = np.isnan(want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)) and np.isnan(got[nan]).all()
    t = T.sqrt()
    with np.errstate(all="ignore"):
        want = np.sqrt(T.u2f(t)[:, 0].astype(np.float64)).astype(np.float32)
    got = _f(L, "sqrt", t)[:, 0]
    nan = np.isnan(want)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)) and np.isnan(got[nan]).all()
    t = T.unorm()
    c, mx = T.u2f(t)[:, 0].astype(np.float64), T.u2f(t)[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        cc = np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 1.0))
        want = np.floor((cc * mx + 0.5).astype(np.float32))        # one rounding of the fma: c * max + 0.5 is exact in float64
    assert np.array_equal(T.oracle_batch(L, "unorm", t)[:, 0], want.astype(np.uint32))


def test_sincos_quadrant_in_float_moved_no_bit_where_the_cast_was_defined(L):
    """zo_sincosf takes k mod 4 as k - 4 floor(k / 4); before, it was ((int)k) & 3.  Over the whole table, wherever |k| < 2^31 (the cast's
    range) the two give the same bits; beyond, the new form gives quadrant 0, which is what the x86 build of the cast happened to give."""
    t = T.sincos()
    new = T.oracle_batch(L, "sincos", t)
    out = (C.c_float * 2)()
    L.zo_kat_sincos_intcast.argtypes = [C.c_float, C.c_void_p]
    n_in = n_out = 0
    for bits, x, got in zip(t[:, 0], T.u2f(t)[:, 0], new):
        if np.isnan(x):
            continue
        if L.zo_kat_sincos_intcast(float(x), out):
            n_in += 1
            assert np.array_equal(np.array([out[0], out[1]], dtype=np.float32).view(np.uint32), got) or np.isnan(T.u2f(got)).all(), hex(bits)
        else:
            n_out += 1
            assert abs(float(T.sincos_k(np.array([bits], dtype=np.uint32))[0])) >= 2.0 ** 31 or np.isinf(x)
    assert n_in > 30000 and n_out > 10000


# ------------------------------------------------------------------------------------------------------------------ (d) source shape

def test_probe_defines_no_arithmetic_of_its_own_and_uses_the_products_flags():
    src = open(os.path.join(ROOT, "tests", "device_probe", "probe.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.findall(r"\bzr_[a-z0-9_]+\s*\([^;{]*\)\s*\{", code), "probe.hip defines a zr_* function"
    assert '#include "../../zeldaengine_amd/csrc/zr_shade.h"' in src and "__builtin_amdgcn" not in src and "atomic" not in src.lower()
    # the sampler and surface entries call the product's functions (zr_texture.h, zr_surface.h) and define none of them; the packed texel
    # is laid out by the product's kSlotPack
    assert '#include "../../zeldaengine_amd/csrc/zr_surface.h"' in src and '#include "../../zeldaengine_amd/csrc/zr_ctx.h"' in src
    called = ["tex_footprint", "tex_sample<1>", "tex_sample_material", "tex_sample_packed", "bary_screen", "bary_homog", "interp1", "interp3",
              "compute_normal", "model_point", "f32_to_f16_hw", "f16_to_f32_hw"]
    assert all(f + "(" in code for f in called)
    assert not re.findall(r"\b(?:tex_|pk_|bary_|interp|compute_normal|model_point|f32_to_f16|f16_to_f32)[a-z0-9_]*\s*\([^;{]*\)\s*\{", code), "probe.hip defines a product function"
    assert "kSlotPack[" in code and not re.search(r"ZR_PK_(?!CHANNELS)", code)
    enum = re.search(r"enum \{(.*?)ZP_COUNT", src, re.S).group(1)
    ids = [s.strip().split("=")[0].strip() for s in enum.replace("\n", " ").split(",") if s.strip()]
    assert len(ids) == len(T.PROBE_FUNCTIONS)
    b = open(os.path.join(ROOT, "tests", "device_probe", "build.py")).read()
    assert "zbuild.FLAGS" in b and "-ffp-contract" not in b.split('"""')[2] and "-l:libamdhip64.so" in b
    from zeldaengine_amd import build as zbuild
    assert "-ffp-contract=off" in zbuild.FLAGS and "-fno-fast-math" in zbuild.FLAGS
    pkg = os.path.join(ROOT, "zeldaengine_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                assert "device_probe" not in open(os.path.join(dirpath, f), errors="replace").read(), f


# ------------------------------------------------------------------------------------------------------------------ the tables that read a scene

def test_pcf_table_takes_both_column_patterns_and_the_per_texel_path():
    for dim in (8, 64, 100):
        p = T.pcf_points(dim)
        x = T.u2f(p)
        _, _, pattern, p1, p3 = T.pcf_columns(x[:, 0], dim)
        assert (pattern & p1).sum() > 100 and (pattern & ~p1).sum() > 100, "both values of p1"
        assert (pattern & p3).sum() > 100 and (pattern & ~p3).sum() > 100, "both values of p3"
        assert (~pattern).sum() > 1000, "map edges: the per-texel path"
        u = x[:, 0].astype(np.float64) * dim
        assert (u < 1).any() and (u > dim - 1).any() and np.isnan(u).any()
        for v in (1.0, -1.0):
            assert all((x[:, 2] == np.nextafter(np.float32(v), np.float32(s))).any() for s in (-9, 9)) and (x[:, 2] == v).any()
        assert (x[:, 2] == T.SHADOW_TIE).any()
    w = np.array(list(T.PCF_W.values()), dtype=np.float32)
    assert (w == 0).any() and (w < 0).any() and ((w > 0) & (w < np.float32(1.17549435e-38))).any()


def test_pcf_batch_is_25_shadow_taps(L, oracle_lib):
    """zo_pcf over a caller-supplied map = the sum, in the shader's order, of zo_shadow_tap's batch export, / 25 as a multiplication"""
    dim = 64
    mp = T.shadow_maps(dim)["random"]
    sc = T.Scene(map_dim=dim, shadow_map=mp)
    o = sc.oracle(oracle_lib)
    pts = T.pcf_points(dim)[::7]
    got = T.u2f(sc.oracle_batch(o, "pcf_taps", pts))[:, 0]
    P = T.u2f(pts)
    total = np.zeros(len(pts), dtype=np.float32)
    one = np.ones(len(pts), dtype=np.float32)
    for x in range(-2, 3):
        for y in range(-2, 3):
            taps = np.column_stack([P[:, 0], P[:, 1], P[:, 2], one, np.full(len(pts), sc.dxy * np.float32(x)), np.full(len(pts), sc.dxy * np.float32(y))])
            total = (total + T.u2f(T.oracle_batch(L, "shadow_tap", T.f2u(taps).reshape(-1, 6), mp))[:, 0]).astype(np.float32)
    assert np.array_equal(got, (total * np.float32(0.04)).astype(np.float32))


def test_shade_tables_straddle_the_falloff_early_out_and_hold_every_mask_kind():
    both = set()
    for i, (nd, npt, poison) in enumerate(T.SHADE_VIEWS):
        v = T.shade_view(nd, npt, roll=i, poison=poison)
        assert tuple(v["LightsCount"][:2]) == (nd, npt)
        lp = v["PointLights"]["Position"][:npt, :3].astype(np.float32)
        fo = v["PointLights"]["Direction"][:npt, 3].astype(np.float32)
        d2 = (lp[:, 2] * lp[:, 2] + (lp[:, 1] * lp[:, 1] + lp[:, 0] * lp[:, 0])).astype(np.float32)       # from P = origin: zr_dot's order, exact products here
        with np.errstate(all="ignore"):
            lim = ((fo * fo).astype(np.float32) * np.float32(1.000001)).astype(np.float32)
            near = np.isfinite(fo) & (fo > 0) & (np.abs(np.sqrt(d2.astype(np.float64)) / fo - 1.0) < 2e-5)
        both |= {("skip", bool(s)) for s in (d2 > lim)[near]}
        both |= {("exact", True) for a, b in zip(lp[near], fo[near]) if a[0] == b and a[1] == 0 and a[2] == 0}
        if npt >= 31 and not poison:
            assert (d2 == 0).any() and (fo < 0).any() and np.isinf(fo).any()
        if poison and npt >= 33:
            col = v["PointLights"]["Color"][:npt]
            assert np.isnan(col).any() and np.isinf(col).any() and (fo == 0).any() and np.isnan(fo).any()
        t = T.shade_cases(npt, i)
        m = t[:, 15:]
        assert (m == 0xFFFFFFFF).all(axis=1).any() and (m == 0).all(axis=1).any()
        if npt:
            last = np.zeros(8, dtype=np.uint32)
            last[(npt - 1) >> 5] = np.uint32(1) << np.uint32((npt - 1) & 31)
            assert (m == last).all(axis=1).any(), "only the last valid bit"
        if npt < 256:
            valid = np.zeros(8, dtype=np.uint32)
            for b in range(npt):
                valid[b >> 5] |= np.uint32(1) << np.uint32(b & 31)
            assert (((m & valid) == 0).all(axis=1) & (m != 0).any(axis=1)).any(), "only bits beyond nPoint"
        s = T.u2f(t[:, :15])
        assert (s[:, 7] == T.ROUGHNESS_SWITCH).any() and (s[:, 7] == 0).any() and (s[:, 7] == T.unorm8_quotients()[1]).any()
        assert (np.abs(np.einsum("ij,ij->i", s[:, 8:11], s[:, 0:3] - s[:, 12:15])) == 0).any(), "N perpendicular to V"
        assert (s[:, 0:3] == s[:, 12:15]).all(axis=1).any(), "cam == P"
    assert both == {("skip", True), ("skip", False), ("exact", True)}, both
    assert {n for _, n, _ in T.SHADE_VIEWS} == {0, 1, 31, 32, 33, 64, 256} and {n for n, _, _ in T.SHADE_VIEWS} == {0, 1, 2}


def test_cube_batch_is_the_scalar_export_and_reaches_every_face_and_level(oracle_lib):
    for dim in (1, 2, 16):
        sc = T.Scene(cube_dim=dim)
        o = sc.oracle(oracle_lib)
        t = T.cube_sample(dim)
        got = T.u2f(sc.oracle_batch(o, "cube_sample", t))
        x = T.u2f(t)
        for i in range(0, len(t), 37):
            if not np.isnan(x[i]).any():
                assert np.array_equal(o.cube_sample(x[i, :3], x[i, 3]).view(np.uint32), got[i].view(np.uint32))
        ax = np.abs(x[:, :3])
        assert ((ax[:, 0] == ax[:, 1]) & (ax[:, 1] == ax[:, 2]) & (ax[:, 0] > 0)).any() and (ax == 0).all(axis=1).any() and np.isnan(x[:, :3]).any()
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert ((ax[:, a] == ax[:, b]) & (ax[:, a] > ax[:, 3 - a - b])).any(), "a two-way tie for the major axis"
        lod = x[:, 3]
        assert (lod < 0).any() and (lod > sc.levels).any() and np.isnan(lod).any() and all((lod == l).any() for l in range(sc.levels))


# ------------------------------------------------------------------------------------------------------------------ the sampler and the surface stage
# (a) coverage

IMAGE_IDS = ["%dx%d" % s for s in T.IMAGE_SETS]


def _frac(x):
    from fractions import Fraction
    return Fraction(float(np.float32(x)))


def _is_f32(q):
    """the rational q is a float32 (a normal one: at most 24 significant bits, exponent in range)"""
    f = np.float32(float(q))
    return np.isfinite(f) and _frac(f) == q


@pytest.mark.parametrize("w,h", T.IMAGE_SETS, ids=IMAGE_IDS)
def test_footprint_table_sits_on_every_breakpoint(L, w, h):
    """every N in 1..16 and both major axes occur; on the exact breakpoints the products are exact and N is what rational arithmetic on the
    float32 operands gives (not excused by any margin); 1 and 2 ulp either side are present; lambda lands on every level of the chain, below
    0 and above the last level; a zero minor axis gives 16; denormal, overflowing and non-finite operands are present"""
    from fractions import Fraction
    t = T.tex_footprint(w, h)
    assert len(t) <= 250000
    r = T.oracle_batch(L, "tex_footprint", t)
    N, lam = r[:, 0].astype(np.int64), T.u2f(r[:, 1])
    d = T.u2f(t[:, 3:])
    assert set(np.unique(N)) == set(range(1, 17))
    x_major = (r[:, 2] == t[:, 3]) & (r[:, 3] == t[:, 4]) & ((t[:, 3] != t[:, 5]) | (t[:, 4] != t[:, 6]))
    y_major = (r[:, 2] == t[:, 5]) & (r[:, 3] == t[:, 6]) & ((t[:, 3] != t[:, 5]) | (t[:, 4] != t[:, 6]))
    for n in range(2, 17):
        assert (x_major & (N == n)).any() and (y_major & (N == n)).any(), n
    bp = T.footprint_breakpoints(w, h)
    assert np.array_equal(T.f2u(bp[:, :4].astype(np.float32)).reshape(-1, 4), t[:len(bp), 3:])
    W, H = Fraction(w), Fraction(h)
    seen = set()
    for row, got, out in zip(bp, N[:len(bp)], r[:len(bp)]):
        dudx, dvdx, dudy, dvdy = (_frac(v) for v in row[:4])
        n, major, ulps = int(row[4]), int(row[5]), int(row[6])
        seen.add((n, major, ulps))
        if ulps:
            continue
        rx2, ry2 = (dudx * W) ** 2 + (dvdx * H) ** 2, (dudy * W) ** 2 + (dvdy * H) ** 2
        rmax2, rmin2 = max(rx2, ry2), min(rx2, ry2)
        assert all(_is_f32(q) for q in (dudx * W, dvdx * H, dudy * W, dvdy * H, rx2, ry2)) and all(_is_f32(k * k * rmin2) for k in range(1, 17)), row
        assert rmax2 == n * n * rmin2, "the quotient is exactly N^2"
        assert got == min(k for k in range(1, 17) if k * k * rmin2 >= rmax2) == n, row
        if n == 1:                                           # the tie goes to x
            assert rx2 == ry2 and (out[2], out[3]) == tuple(T.f2u(np.float32(row[:2]))), row
    assert seen == {(n, m, u) for n in range(1, 17) for m in (0, 1) for u in range(-2, 3)}
    # N on either side of a breakpoint: one more tap as soon as the ratio exceeds N^2
    for k, row in enumerate(bp):
        if row[4] < 16 and row[6] > 0:
            assert N[k] == row[4] + 1, row
        if row[6] < 0 and row[4] > 1:
            assert N[k] == row[4], row
    levels = T.levels_of(w, h)
    fin = np.isfinite(lam)
    assert fin.all() and lam.min() == 0 and lam.max() == levels - 1
    assert all((lam == l).any() for l in range(levels))
    with np.errstate(all="ignore"):
        ax2 = (d[:, 0].astype(np.float64) * w) ** 2 + (d[:, 1].astype(np.float64) * h) ** 2
        by2 = (d[:, 2].astype(np.float64) * w) ** 2 + (d[:, 3].astype(np.float64) * h) ** 2
    # lambda against float64 where the clamp does not act: zr_log2's bound 4e-7 max(1, |log2 x|) on log2(Pmax^2) halved (6.4e-6 while
    # |log2 Pmax^2| <= 32) and on log2 N (1.6e-6), the float32 roundings of the products and of Pmax^2 (3 eps / ln 2 / 2 = 1.3e-7) and of
    # the subtraction (eps * 32 = 1.9e-6): 1e-5 absolute
    with np.errstate(all="ignore"):
        ref = 0.5 * np.log2(np.maximum(ax2, by2)) - np.where(N > 1, np.log2(N.astype(np.float64)), 0.0)
        inside = np.isfinite(ref) & (ref > 1e-4) & (ref < levels - 1 - 1e-4) & (np.abs(np.log2(np.maximum(ax2, by2))) <= 32)
    if levels > 1:
        worst = np.abs(lam[inside] - ref[inside]).max()
        print("tex_footprint %d x %d: lambda against float64 on %d cases, worst %.3g" % (w, h, inside.sum(), worst))
        assert inside.sum() > 50 and worst < 1e-5
    tiny = np.float64(np.float32(1.17549435e-38))
    assert ((ax2 > 0) & (ax2 < tiny)).any() and (ax2 > 3.5e38).any() and ((np.minimum(ax2, by2) == 0) & (np.maximum(ax2, by2) > 0) & (N == 16)).any()
    assert ((ax2 == 0) & (by2 == 0) & (N == 1)).any()
    for k in range(4):
        assert np.isnan(d[:, k]).any() and (d[:, k] == np.inf).any() and (d[:, k] == -np.inf).any()
    assert (t[:, 3:] == 0x80000000).any()


@pytest.mark.parametrize("w,h", T.IMAGE_SETS, ids=IMAGE_IDS)
def test_sampler_table_reaches_every_level_pair_and_every_wrap(L, w, h):
    t = T.tex_cases(w, h)
    assert len(t) <= 250000
    levels = T.levels_of(w, h)
    head = np.tile(np.array([w, h, levels], dtype=np.uint32), (len(t), 1))
    r = T.oracle_batch(L, "tex_footprint", np.concatenate([head, t[:, 2:]], axis=1))
    N, lam = r[:, 0], T.u2f(r[:, 1])
    assert set(np.unique(N)) == set(range(1, 17))
    one = N == 1
    l0, l1, fx, fy, wl, hl = T.tap_addresses(w, h, t[one], lam[one])
    pairs = set(zip(l0.tolist(), l1.tolist()))
    assert pairs == {(l, min(l + 1, levels - 1)) for l in range(levels)}, pairs           # the last level with l1 == l0 included
    for l in range(levels):
        at = l0 == l
        assert (at & (fx == -1)).any() and (at & (fx == wl - 1)).any(), "x wraps on level %d" % l     # x0 = w - 1 with x1 = 0, from either side
        assert (at & (fy == -1)).any() and (at & (fy == hl - 1)).any(), "y wraps on level %d" % l
    # the coordinates: every texel centre and edge (+- 1 ulp) of levels 0 and 1, and the special values
    u, v = t[:, 0], t[:, 1]
    for col, n in ((u, w), (v, h)):
        have = set(col.tolist())
        for m in (n, max(1, n >> 1)):
            k = np.arange(m + 1, dtype=np.float64)
            assert set(T.f2u(((k[:-1] + 0.5) / m).astype(np.float32)).tolist()) <= have and set(T.around((k / m).astype(np.float32), 1).tolist()) <= have
        x = T.u2f(col)
        assert {0, 0x80000000, 0x3F800000, 0x80000001, T.INF, 0xFF800000} <= have and np.isnan(x).any()
        assert (x == np.float32(2.0 ** 23 + 0.5)).any() and (x == np.float32(1e30)).any() and (x == np.float32(3e38)).any()
        assert ((x > -3) & (x < 0)).sum() > 100 and ((x > 1) & (x < 4)).sum() > 100
    tiny = T.u2f(np.array([0x80000001], dtype=np.uint32))
    assert (tiny - np.floor(tiny)).astype(np.float32)[0] == 1.0        # u - floor(u) rounds to exactly 1


def test_material_sets_take_one_two_and_three_grouping_turns():
    def sizes(tex):
        return [tex.slots[s].shape[1::-1] if tex.is_image(s) else None for s in range(7)]
    one = sizes(T.material_one_size(128, 4))
    assert len(set(one)) == 1 and None not in one
    three = sizes(T.material_three_sizes())
    assert len({s for s in three if s}) == 3 and three[0] is not None and None in three[1:6]
    lead = sizes(T.material_lead_not_zero())
    assert lead[0] is None and len({s for s in lead if s}) == 2
    # the level count is a function of the size: two slots equal in w and h cannot differ in levels
    assert all(T.levels_of(w, h) == int(np.floor(np.log2(max(w, h)))) + 1 for w, h in T.IMAGE_SETS)
    for tex in (T.material_three_sizes(), T.material_lead_not_zero(), T.material_one_size(16384, 1)):
        assert 1000 < len(T.material_cases(tex)) <= 250000


def test_surface_tables_hold_their_edges(L):
    t = T.compute_normal()
    x = T.u2f(t).astype(np.float64)
    s1, t1, s2, t2 = x[:, 6], x[:, 7], x[:, 8], x[:, 9]
    with np.errstate(all="ignore"):
        det = s1 * t2 - s2 * t1                              # exact in float64 for the hand-made rows (products of floats with few bits)
    hand = np.arange(len(t)) < len(t) - len(T.vectors(16)) - 2000
    const = hand & (s1 == 0) & (t1 == 0) & (s2 == 0) & (t2 == 0)
    collinear = hand & (det == 0) & (s1 != 0) & (t1 != 0)
    assert const.any() and collinear.any() and (hand & (det > 0)).any() and (hand & (det < 0)).any()
    assert (hand & (det != 0) & (np.abs(det) < 1.17549435e-38)).any(), "a denormal determinant"
    assert (hand & (det != 0) & (x[:, 0:6] == 0).all(axis=1)).any(), "a zero position derivative"
    n = x[:, 10:13]
    assert (hand & (n == 0).all(axis=1)).any() and (hand & np.isnan(n).any(axis=1)).any() and (hand & np.isinf(n).any(axis=1)).any()
    assert (hand & (n[:, 0] == np.float64(np.float32(1e-40)))).any() and (hand & (x[:, 13:16] == (0, 0, 1)).all(axis=1)).any()
    assert (hand & (t1 == 0) & (n == x[:, 0:3]).all(axis=1) & (x[:, 0] != 0)).any(), "T parallel to N"
    # bary_screen: the subtraction px * 256 + 128 - X0 stays inside int, pixels reach 16383, each pixel's quad partners are cases too
    b = T.bary_screen(L)
    X0, Y0 = b[:, 0].view(np.int32).astype(np.int64), b[:, 1].view(np.int32).astype(np.int64)
    px, py = b[:, 9].astype(np.int64), b[:, 10].astype(np.int64)
    assert np.abs(px * 256 + 128 - X0).max() < 2 ** 31 and np.abs(py * 256 + 128 - Y0).max() < 2 ** 31
    assert px.min() == 0 and px.max() == T.MAX_PIXEL and py.max() == T.MAX_PIXEL
    blocks = np.concatenate([np.arange(k * 4500, k * 4500 + 1500) for k in range(4)])
    assert len(b) == 18000 and np.array_equal(b[blocks + 1500, 9], b[blocks, 9] ^ 1) and np.array_equal(b[blocks + 3000, 10], b[blocks, 10] ^ 1)
    rw = T.u2f(b[:, 6:9]).astype(np.float64)
    s = rw.sum(axis=1)
    assert (s == 0).any() and ((s > 0) & (s < 1.17549435e-38)).any() and (s > 3.4e38).any()
    # project()'s table feeds the set-ups: every X0, Y0 is one of its results
    sv = T.oracle_batch(L, "project", T.project())
    assert set(b[:, 0].tolist()) <= set(sv[:, 0].tolist()) and set(b[:, 1].tolist()) <= set(sv[:, 1].tolist())
    sat = (np.abs(sv[:, 0].view(np.int32).astype(np.int64)) >= T.PROJECT_SATURATED) | (np.abs(sv[:, 1].view(np.int32).astype(np.int64)) >= T.PROJECT_SATURATED)
    assert sat.sum() == 320 and (T.project()[sat, 3] == 1).all(), "the corners left out are exactly those with w = 2^-149"
    h = T.bary_homog()
    wv = T.u2f(h[:, [3, 7, 11]])
    nonpos = (wv <= 0).sum(axis=1)
    assert (nonpos == 1).any() and (nonpos == 2).any()
    assert ((h[:, 0:4] == h[:, 4:8]).all(axis=1) & (h[:, 0:4] == h[:, 8:12]).all(axis=1)).any(), "a zero denominator"
    assert set(T.clip_vertices()[:, 0].tolist()) >= set(h[:, 0].tolist())
    m = T.model_point()
    flag = m[:, 19]
    ident = (m[:, :16] == T.f2u(T.IDENTITY)).all(axis=1)
    p = T.u2f(m[:, 16:19])
    p1 = p[flag == 1]
    assert (ident | (flag == 0)).all() and (np.isfinite(p1).all(axis=1) | np.isnan(p1).all(axis=1)).all() and np.isnan(p1).any() and np.isinf(p[flag == 0]).any()
    assert (np.isnan(p[flag == 0]).any(axis=1) & np.isfinite(p[flag == 0]).any(axis=1)).any()
    assert ((m[:, 12:15] == 0x80000000).all(axis=1) & (flag == 0)).any() and (m[:, :16] == T.f2u(T.stage_roll())).all(axis=1).any()
    assert (m[flag == 1, 16:19] == 0x80000000).any(), "-0 through the short cut"
    assert set(T.f32_to_f16()[:, 0].tolist()) >= set(T.generic().tolist()) and len(T.f16_codes()) == 65536


# (b) batch = scalar

def test_sampler_batch_exports_are_the_scalar_ones(L, oracle_lib):
    rng = np.random.default_rng(6)
    out3 = np.zeros(3, dtype=np.float32)
    for w, h in ((33, 7), (128, 4), (2, 2)):
        t = T.tex_footprint(w, h)
        t = t[np.sort(rng.choice(len(t), 600, replace=False))]
        t = t[~np.isnan(T.u2f(t[:, 3:])).any(axis=1)]
        got = T.oracle_batch(L, "tex_footprint", t)
        for row, g in zip(t, got):
            d = T.u2f(row[3:])
            with np.errstate(all="ignore"):
                a = [float(np.float32(d[0] * np.float32(w))), float(np.float32(d[1] * np.float32(h))), float(np.float32(d[2] * np.float32(w))), float(np.float32(d[3] * np.float32(h)))]
            L.zo_kat_aniso(*a, int(row[2]), out3.ctypes.data)
            assert int(out3[0]) == g[0] and out3[1:2].view(np.uint32)[0] == g[1], row
            assert (g[2], g[3]) == ((row[3], row[4]) if out3[2] else (row[5], row[6]))
        for srgb in (True, False):
            tex, slot = T.single_image(w, h, srgb)
            o = tex.oracle(oracle_lib)
            c = T.tex_cases(w, h)
            c = c[np.sort(rng.choice(len(c), 400, replace=False))]
            c = c[~np.isnan(T.u2f(c)).any(axis=1)]
            got = T.u2f(tex.oracle_image(o, slot, c, srgb))
            x = T.u2f(c)
            for row, g in zip(x, got):
                want = o.tex_sample(tex.slots[slot], srgb, row[:2], row[2:])
                assert np.array_equal(want.view(np.uint32)[~np.isnan(want)], g.view(np.uint32)[~np.isnan(want)]) and np.isnan(g[np.isnan(want)]).all(), row
            o.close()
    tex = T.material_three_sizes()
    o = tex.oracle(oracle_lib)
    c = T.material_cases(tex)[::97]
    mat = tex.oracle_material(o, c)
    for s in range(7):
        assert np.array_equal(mat[:, 4 * s:4 * s + 4], tex.oracle_image(o, s, c, s == 0)), s
    o.close()


# (c) float64

def sampler_random_cases(w, h, n, seed):
    """finite, in-domain samples: coordinates in [-2, 3], footprints from an eighth of a texel to half the image at ratios none of which
    is an integer (a rotated footprint of ratio 1 has Pmax / Pmin = 1 +- 1e-16 in the reference, which its margin rule would excuse, so the
    single-tap case is drawn as an exactly isotropic footprint instead, every tenth sample): the reference alone keeps the share"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-2.0, 3.0, (n, 2))
    scale = 2.0 ** rng.uniform(-3.0, np.log2(max(w, h)) - 1.0, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    ratio = rng.choice([1.37, 2.4, 3.3, 5.5, 8.6, 11.3, 15.6, 40.0], n)
    major = np.stack([np.cos(ang) / w, np.sin(ang) / h], axis=1) * scale[:, None]
    minor = np.stack([-np.sin(ang) / w, np.cos(ang) / h], axis=1) * (scale / ratio)[:, None]
    swap = (np.arange(n) % 2 == 0)[:, None]
    duv = np.concatenate([np.where(swap, minor, major), np.where(swap, major, minor)], axis=1)
    iso = np.arange(n) % 10 == 0
    t = 2.0 ** (rng.integers(-3, 6, n) - np.ceil(np.log2(w * h)))       # (h t) w == (w t) h exactly: w h t texels either way, 1/8 .. 32 of them
    duv[iso] = np.stack([h * t, np.zeros(n), np.zeros(n), w * t], axis=1)[iso]
    return T.f2u(np.concatenate([uv, duv], axis=1).astype(np.float32)).reshape(-1, 6)


@pytest.mark.parametrize("w,h", [(33, 7), (64, 64), (128, 4)], ids=["33x7", "64x64", "128x4"])
@pytest.mark.parametrize("srgb", [True, False], ids=["sRGB", "UNORM"])
def test_sampler_batch_against_float64(oracle_lib, w, h, srgb):
    """the rule of test_material_sampler_against_float64: atol 3e-5, a sample excused where the reference's margin to an integer
    Pmax / Pmin is below 1e-3, and at least 550 of 600 kept"""
    import independent_sampler as isamp
    tex, slot = T.single_image(w, h, srgb)
    o = tex.oracle(oracle_lib)
    c = sampler_random_cases(w, h, 600, 20280 + w + srgb)
    got = T.u2f(tex.oracle_image(o, slot, c, srgb))
    chain = o.tex_mips(tex.slots[slot], srgb)
    x = T.u2f(c).astype(np.float64)
    kept, worst = 0, 0.0
    for row, g in zip(x, got):
        want, n, lam, margin = isamp.sample_2d(chain, srgb, row[:2], row[2:])
        if margin < 1e-3:
            continue
        kept += 1
        worst = max(worst, float(np.abs(g - want).max()))
        assert np.allclose(g, want, atol=3e-5, rtol=0), (row, n, lam, g, want)
    print("sampler %d x %d %s: kept %d of 600, worst %.3g" % (w, h, "sRGB" if srgb else "UNORM", kept, worst))
    assert kept >= 550
    o.close()


EPS = 2.0 ** -24          # half an ulp of float32, relative


def _well(x, lo=2.0 ** -20, hi=2.0 ** 20):
    a = np.abs(x)
    return np.isfinite(x).all(axis=1) & ((a == 0) | ((a > lo) & (a < hi))).all(axis=1)


def test_surface_batches_against_float64(L):
    """interp, both barycentric forms and ComputeNormal against float64 on the finite, well-conditioned part of their tables.  Each bound
    is a count of roundings (eps = 2^-24 each, relative to the magnitudes that enter) with a factor 2 of slack; the measured worst case is
    printed and recorded in DESIGN.md section 4."""
    # interp: b0 a0 + b1 a1 + b2 a2 with one rounded product and two fmas: 3 roundings, each at most eps * sum |b_k a_k|
    t = T.vectors12()
    x = T.u2f(t).astype(np.float64)
    ok = _well(x, 2.0 ** -60, 2.0 ** 60)                     # no product overflows, none is denormal
    got = T.u2f(T.oracle_batch(L, "interp", t)).astype(np.float64)[ok]
    x = x[ok]
    b, A = x[:, 0:3], x[:, 3:12].reshape(-1, 3, 3)
    ref3 = np.einsum("nk,nkc->nc", b, A)
    mag3 = np.einsum("nk,nkc->nc", np.abs(b), np.abs(A))
    ref1 = b[:, 0] * A[:, 0, 0] + b[:, 1] * A[:, 1, 1] + b[:, 2] * A[:, 2, 2]
    mag1 = np.abs(b[:, 0] * A[:, 0, 0]) + np.abs(b[:, 1] * A[:, 1, 1]) + np.abs(b[:, 2] * A[:, 2, 2])
    tiny = 2.0 ** -126
    e = max((np.abs(got[:, :3] - ref3) / (mag3 * EPS + tiny)).max(), (np.abs(got[:, 3] - ref1) / (mag1 * EPS + tiny)).max())
    print("interp: %d cases, worst %.3g eps of sum |b a| (bound 3)" % (ok.sum(), e))
    assert ok.sum() > 300 and e <= 3.0

    # bary_screen on proper set-ups (finite, positive rw): fx, fy are exact.  With m = 1 + |a1 fx| + |b1 fy| + |a2 fx| + |b2 fy|, which bounds
    # every |l_k|: l1 and l2 carry 2 roundings of terms below m (2 eps m each), l0 those 4 and 2 of its own (6 eps m); q_k = l_k rw_k one more
    # (7 eps m |rw_k|); the sum of three adds 2 (in all 9 eps m sum |rw|); the reciprocal and the last product 2.  So
    # |b_k - ref| <= (7 eps m max |rw| + |b_k| 9 eps m sum |rw|) / |sum q| + 2 eps |b_k| <= 18 eps D, D = m sum |rw| / |sum q| * max(1, max |b_k|),
    # doubled for the second-order terms: 36 eps D, asserted where D < 2^10.
    s = T.bary_screen(L)
    f = T.u2f(s[:, 2:9]).astype(np.float64)
    X0, Y0 = s[:, 0].view(np.int32).astype(np.float64), s[:, 1].view(np.int32).astype(np.float64)
    fx, fy = s[:, 9].astype(np.float64) * 256 + 128 - X0, s[:, 10].astype(np.float64) * 256 + 128 - Y0
    with np.errstate(all="ignore"):
        l1, l2 = f[:, 1] * fy + f[:, 0] * fx, f[:, 3] * fy + f[:, 2] * fx
        l0 = 1.0 - l1 - l2
        q = np.stack([l0, l1, l2], axis=1) * f[:, 4:7]
        ref = q / q.sum(axis=1, keepdims=True)
        m = 1.0 + np.abs(f[:, 1] * fy) + np.abs(f[:, 0] * fx) + np.abs(f[:, 3] * fy) + np.abs(f[:, 2] * fx)
        D = m * np.abs(f[:, 4:7]).sum(axis=1) / np.abs(q.sum(axis=1)) * np.maximum(1.0, np.abs(ref).max(axis=1))
        ok = np.isfinite(f).all(axis=1) & (f[:, 4:7] > 2.0 ** -20).all(axis=1) & (f[:, 4:7] < 2.0 ** 20).all(axis=1) & np.isfinite(D) & (D < 2.0 ** 10)
    got = T.u2f(T.oracle_batch(L, "bary_screen", s)).astype(np.float64)
    e = (np.abs(got[ok] - ref[ok]).max(axis=1) / (D[ok] * EPS)).max()
    print("bary_screen: %d cases, worst %.3g eps * D (bound 36)" % (ok.sum(), e))
    assert ok.sum() > 1000 and e <= 36.0

    # bary_homog: each k is a 3-term fma chain of 2 x 2 determinants (each: one rounded product, one fma): relative to
    # K = sum over terms of the magnitudes, 2 + 3 roundings; the sum two more, the reciprocal and the product two: 9, doubled: 18 eps * K / |sum k|.
    hcase = T.bary_homog()
    c = T.u2f(hcase[:, :12]).astype(np.float64).reshape(-1, 3, 4)
    hw, hh = T.u2f(hcase[:, 12]).astype(np.float64), T.u2f(hcase[:, 13]).astype(np.float64)
    with np.errstate(all="ignore"):
        u, v = (hcase[:, 14].astype(np.float64) + 0.5 - hw) / hw, (hcase[:, 15].astype(np.float64) + 0.5 - hh) / hh
        k, K = [], []
        for i in range(3):
            p, q_ = c[:, (i + 1) % 3], c[:, (i + 2) % 3]
            kx, ky, kz = p[:, 1] * q_[:, 3] - q_[:, 1] * p[:, 3], q_[:, 0] * p[:, 3] - p[:, 0] * q_[:, 3], p[:, 0] * q_[:, 1] - q_[:, 0] * p[:, 1]
            k.append(kx * u + ky * v + kz)
            K.append((np.abs(p[:, 1] * q_[:, 3]) + np.abs(q_[:, 1] * p[:, 3])) * np.abs(u) + (np.abs(q_[:, 0] * p[:, 3]) + np.abs(p[:, 0] * q_[:, 3])) * np.abs(v) +
                     np.abs(p[:, 0] * q_[:, 1]) + np.abs(q_[:, 0] * p[:, 1]))
        k, K = np.stack(k, axis=1), np.stack(K, axis=1).sum(axis=1)
        den = k.sum(axis=1)
        ref = k / den[:, None]
        scale = K / np.abs(den) * np.maximum(1.0, np.abs(ref).max(axis=1))
        ok = _well(T.u2f(hcase[:, :12]).astype(np.float64)) & np.isfinite(ref).all(axis=1) & (scale < 2.0 ** 12) & (np.abs(u) < 8) & (np.abs(v) < 8)
    got = T.u2f(T.oracle_batch(L, "bary_homog", hcase)).astype(np.float64)
    e = (np.abs(got[ok] - ref[ok]).max(axis=1) / (scale[ok] * EPS)).max()
    print("bary_homog: %d cases, worst %.3g eps * K / |sum k| (bound 18)" % (ok.sum(), e))
    assert ok.sum() > 1000 and e <= 18.0

    # ComputeNormal on well-conditioned cases: a unit result; the chain is det (2 roundings), T (3 x 2, times 1 / det: 2), three normalisations
    # (dot: 3, rsqrt 1.2 ulp ~ 2.4 eps, product 1: ~7 each), the projection N (N . T) (3 + 1 + 1), the cross product (2), the final
    # combination (3): about 45 roundings, amplified by 1 / sin(angle(T, N)) where T is projected off N and by |det|'s cancellation.  Asserted
    # on cases with sin > 1/4 and |s1 t2| + |s2 t1| < 4 |det|: bound 45 * 4 * 4 eps = 720 eps = 4.3e-5 absolute on a unit vector.
    t = T.compute_normal()
    x = T.u2f(t).astype(np.float64)
    with np.errstate(all="ignore"):
        pdx, pdy, s1, t1, s2, t2, fN, ts = x[:, 0:3], x[:, 3:6], x[:, 6], x[:, 7], x[:, 8], x[:, 9], x[:, 10:13], x[:, 13:16]
        det = s1 * t2 - s2 * t1
        Tn = (t2[:, None] * pdx - t1[:, None] * pdy) / det[:, None]
        N = fN / np.linalg.norm(fN, axis=1, keepdims=True)
        Tp = Tn - N * (N * Tn).sum(axis=1, keepdims=True)
        sin = np.linalg.norm(Tp, axis=1) / np.linalg.norm(Tn, axis=1)
        Tu = Tp / np.linalg.norm(Tp, axis=1, keepdims=True)
        B = np.cross(N, Tu)
        B = B / np.linalg.norm(B, axis=1, keepdims=True)
        wv = Tu * ts[:, 0:1] + B * ts[:, 1:2] + N * ts[:, 2:3]
        ref = wv / np.linalg.norm(wv, axis=1, keepdims=True)
        cancel_t = (np.abs(t2[:, None] * pdx) + np.abs(t1[:, None] * pdy)).max(axis=1) / np.abs(t2[:, None] * pdx - t1[:, None] * pdy).max(axis=1)
        ok = (_well(x, 2.0 ** -12, 2.0 ** 12) & np.isfinite(ref).all(axis=1) & (sin > 0.25) & (np.abs(s1 * t2) + np.abs(s2 * t1) < 4 * np.abs(det)) & (cancel_t < 4) &
              (np.linalg.norm(wv, axis=1) > 0.25 * np.linalg.norm(ts, axis=1)) & (np.linalg.norm(ts, axis=1) > 0.01))
    got = T.u2f(T.oracle_batch(L, "compute_normal", t)).astype(np.float64)
    e = np.abs(got[ok] - ref[ok]).max()
    print("compute_normal: %d cases, worst %.3g absolute (bound 720 eps = %.3g)" % (ok.sum(), e, 720 * EPS))
    assert ok.sum() > 200 and e <= 720 * EPS


def test_model_point_short_cut_is_the_matrix_product(L):
    """on the flag-1 rows (M the identity, p all finite or all NaN) M * vec4(p, 1) has the bits of p + 0.0f - the claim model_point's short cut rests on"""
    m = T.model_point()
    one = m[m[:, 19] == 1]
    got = T.oracle_batch(L, "model_point", one)
    with np.errstate(all="ignore"):
        want = T.f2u(T.u2f(one[:, 16:19]) + np.float32(0.0)).reshape(-1, 3)
    nan = np.isnan(T.u2f(want))
    assert np.array_equal(got[~nan], want[~nan]) and np.isnan(T.u2f(got)[nan]).all()


# the stand-alone sanitized run

def _sanitized_oracle_check(tmp_path):
    import subprocess
    flags = ["-std=c11", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-function",
             "-Wno-misleading-indentation", "-Wno-stringop-overread"]
    sanitize = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
    hello = tmp_path / "hello.c"
    hello.write_text("int main(void) { return 0; }\n")
    if not (subprocess.call(["gcc"] + sanitize + [str(hello), "-o", str(tmp_path / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp_path / "hello")]) == 0):
        sanitize = []
    print("sampler_surface_check is built %s" % ("with " + " ".join(sanitize) if sanitize else "WITHOUT the sanitizers: this machine does not link them"))
    exe = tmp_path / "sampler_surface_check"
    subprocess.check_call(["gcc"] + flags + sanitize + [os.path.join(ROOT, "tests", "sampler_surface_check.c"), os.path.join(ROOT, "oracle", "zo_oracle.c"),
                                                         "-lm", "-o", str(exe)])
    return exe


def _fnv1a(data):
    h = 0xCBF29CE484222325
    for k in range(0, len(data), 1 << 16):
        for b in data[k:k + (1 << 16)]:
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_oracle_sampler_and_surface_exports_under_the_sanitizers(L, oracle_lib, tmp_path):
    """tests/sampler_surface_check.c with oracle/zo_oracle.c under -fsanitize=address,undefined,float-cast-overflow over every sampler and
    surface table and every image set, non-finite operands included: a clean exit - no texel indexed outside its chain, no undefined cast.
    Runs on the CPU, stand-alone; a thinned sample of each job's results is compared with the library's through a hash."""
    import struct
    import subprocess
    exe = _sanitized_oracle_check(tmp_path)
    jobs, want = [], []
    plain = ["tex_footprint", "bary_screen", "bary_homog", "interp", "compute_normal", "model_point"]

    def add_plain(name, t):
        jobs.append(struct.pack("<III", 0, plain.index(name), len(t)) + np.ascontiguousarray(t, dtype=np.uint32).tobytes())
        want.append((name, T.oracle_batch(L, name, t)))

    def add_tex(tex, o, slot, srgb, t):
        b = b""
        for s in range(7):
            im = tex.slots[s]
            if tex.is_image(s):
                b += struct.pack("<IIII", 1, im.shape[1], im.shape[0], 1) + im.tobytes()
            else:
                b += struct.pack("<IIII", 1, 1, 1, 0) + im.tobytes()
        jobs.append(struct.pack("<I", 1) + b + struct.pack("<III", slot, int(srgb), len(t)) + np.ascontiguousarray(t, dtype=np.uint32).tobytes())
        want.append(("tex_material", tex.oracle_material(o, t)) if slot == 7 else ("tex_image", tex.oracle_image(o, slot, t, srgb)))

    for w, h in T.IMAGE_SETS:
        add_plain("tex_footprint", T.tex_footprint(w, h))
        for srgb in (True, False):
            tex, slot = T.single_image(w, h, srgb)
            o = tex.oracle(oracle_lib)
            add_tex(tex, o, slot, srgb, T.tex_cases(w, h))
            o.close()
    for tex in (T.material_three_sizes(), T.material_lead_not_zero(), T.material_one_size(128, 4)):
        o = tex.oracle(oracle_lib)
        add_tex(tex, o, 7, True, T.material_cases(tex))
        o.close()
    for name, t in (("bary_screen", T.bary_screen(L)), ("bary_homog", T.bary_homog()), ("interp", T.vectors12()), ("compute_normal", T.compute_normal()),
                    ("model_point", T.model_point())):
        add_plain(name, t)
    with open(tmp_path / "jobs.bin", "wb") as f:
        f.write(struct.pack("<I", len(jobs)) + b"".join(jobs))
    run = subprocess.run([str(exe), str(tmp_path / "jobs.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(jobs)
    # (64-bit FNV-1a on both sides; only the small jobs, to keep this quick)
    for line, (name, out) in zip(lines, want):
        j, got_name, n, h = line.split()
        assert got_name == name and int(n) == len(out)
        if out.nbytes <= 1 << 18:
            nan = np.isnan(out.view(np.float32))
            if not nan.any():                                 # (a NaN's payload may differ between two builds of one source)
                assert _fnv1a(out.tobytes()) == h, line


def test_a_constant_image_filtered_is_not_always_its_texel(L, oracle_lib):
    """What the kernels do with an image whose texels are all equal - every tap is the texel t exactly, the N-tap average is
    ((t + t + ...) / N), NaN coordinates give NaN - against the collapsed texel, on the oracle: one and two taps never differ (t, and
    2t / 2, are exact), more taps differ in the last bits for some sRGB codes, UNORM alpha never (integers), and a non-finite coordinate gives
    NaN where the collapsed slot gives the texel.  This is why the rule has to be written down (oracle/CONTRACT.md)."""
    t = T.constant_image_cases()
    head = np.tile(np.array([T.CONSTANT_SIDE, T.CONSTANT_SIDE, T.levels_of(T.CONSTANT_SIDE, T.CONSTANT_SIDE)], dtype=np.uint32), (len(t), 1))
    N = T.oracle_batch(L, "tex_footprint", np.concatenate([head, t[:, 2:]], axis=1))[:, 0]
    finite = np.isfinite(T.u2f(t[:, :2])).all(axis=1)
    assert set(N[finite].tolist()) == set(range(1, 17))
    differ = np.zeros(17, dtype=np.int64)
    for code in T.CONSTANT_CODES:
        _, filtered, collapsed = T.constant_image(code, oracle_lib, t)
        f, c = T.u2f(filtered), T.u2f(collapsed)
        assert np.isnan(f[~finite]).all() and np.isfinite(c).all() and (c == c[0]).all()
        d = (filtered[finite] != collapsed[finite])
        assert not d[:, 3].any(), "alpha: a filtered code is the code"
        assert not d[N[finite] <= 2].any()
        assert (np.abs(f[finite].astype(np.float64) - c[finite]) <= 16 * EPS * c[finite]).all(), "N - 1 additions and a division, half an ulp each"
        np.add.at(differ, N[finite], d.any(axis=1))
    print("constant image: codes (of %d) whose filtered rgb differs from the texel, by N: %s" % (len(T.CONSTANT_CODES), differ[1:].tolist()))
    assert differ[3:].sum() > 0
