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
