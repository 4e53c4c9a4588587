"""Input tables for the per-call comparison of the product's device functions with the CPU oracle.

Seeded and deterministic; tests/test_gpu_device_functions.py (GPU, bits equal) and tests/test_device_function_tables.py (CPU: the tables'
own coverage claims, the oracle against float64) draw the same arrays.  Every table is a uint32 array of shape (cases, words): floats travel
as their bits, so signalling NaNs, negative zero and denormals arrive as written.  Layouts: tests/device_probe/probe.hip.
"""
import functools

import numpy as np

U = np.uint32
INF, NAN_Q, NAN_S = 0x7F800000, 0x7FC00000, 0x7F800001


def f2u(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(U)


def u2f(u):
    return np.ascontiguousarray(u, dtype=U).view(np.float32)


def around(x, k=2):
    """the floats within k ulp of each finite x (bit neighbours of the magnitude, the sign kept; stops at zero and at infinity)"""
    b = f2u(np.atleast_1d(x)).astype(np.int64)
    sign, mag = b & 0x80000000, b & 0x7FFFFFFF
    out = [sign | np.clip(mag + d, 0, INF) for d in range(-k, k + 1)]
    return np.concatenate(out).astype(U)


@functools.lru_cache(maxsize=None)
def generic():
    """Both signs, every exponent 0..255, eight fixed mantissas and 64 random ones per exponent: zeros, denormals, infinities, quiet and
    signalling NaNs included (36 864 bit patterns)."""
    rng = np.random.default_rng(20240)
    fixed = np.array([0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF], dtype=np.int64)
    rows = []
    for sign in (0, 1):
        for e in range(256):
            m = np.concatenate([fixed, rng.integers(0, 1 << 23, 64)])
            rows.append((sign << 31) | (e << 23) | m)
    g = np.concatenate(rows).astype(U)
    g.setflags(write=False)
    return g


SPECIALS = np.array([0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3D23D70A, 0x3F000000, 0x40000000, INF, 0xFF800000, NAN_Q, 0xFFC00000,
                     NAN_S, 0x00000001, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=U)   # 0.04 = 0x3D23D70A


def _col(*parts):
    return np.concatenate([np.asarray(p, dtype=U).ravel() for p in parts]).reshape(-1, 1)


def _mixed(rng, shape):
    """half drawn from the generic table, half ordinary magnitudes in [-2, 2]"""
    g = generic()
    a = g[rng.integers(0, len(g), shape)]
    b = f2u(rng.uniform(-2.0, 2.0, shape).astype(np.float32)).reshape(shape)
    return np.where(rng.random(shape) < 0.5, a, b).astype(U)


# ------------------------------------------------------------------------------------------------------------------ zr_math.h

def rsqrt():
    return _col(generic(), around(u2f([0x00800000, INF, 0x3F800000, 0x40800000]), 2), SPECIALS)


TWO_OVER_PI = np.float32(0.636619772367581343)


def sincos_k(x_bits):
    """k = rint(x * 2/pi) as zr_sincos forms it (fp32 product, round to nearest even)"""
    with np.errstate(all="ignore"):
        return np.rint(u2f(x_bits) * TWO_OVER_PI)


@functools.lru_cache(maxsize=None)
def sincos():
    ks = list(range(65)) + [2.0 ** j for j in range(7, 34)]
    near = np.array([k * (np.pi / 2) for k in ks], dtype=np.float64).astype(np.float32)
    edge24 = np.float32(2.0 ** 24 * np.pi / 2)               # k reaches 2^24: from here the float k is no longer every integer
    edge31 = np.float32(2.0 ** 31 * np.pi / 2)               # k reaches 2^31 (x ~ 3.37e9): a cast of k to int is out of range from here
    pos = np.concatenate([around(near, 2), around(edge24, 8), around(edge31, 16), around(np.float32(2.0 ** 24), 2),
                          f2u(np.array([1e5, 1e10, 1e12, 1e15, 1e20, 3.3e9, 3.4e9, 565.48, 700.0], dtype=np.float32))])
    rng = np.random.default_rng(20251)          # ordinary angles: the documented domain and the decade on either side of its end
    dense = np.concatenate([rng.uniform(-h, h, 3000) for h in (4.0, 700.0, 1e4, 1.1e5)]).astype(np.float32)
    t = np.concatenate([generic(), pos, pos | U(0x80000000), f2u(dense), SPECIALS]).astype(U)
    t.setflags(write=False)
    return t.reshape(-1, 1)


def exp2():
    halves = np.arange(-127.0, 128.5, 0.5, dtype=np.float32)
    edges = around(np.array([-126.0, -125.5, 127.5, 128.0, -149.0, -150.0], dtype=np.float32), 2)
    return _col(generic(), f2u(halves), edges, SPECIALS)


def log2():
    split = np.float32(1.41421356237)
    scaled = np.concatenate([around(np.float32(split * np.float32(2.0 ** e)), 2) for e in (-126, -64, -1, 0, 1, 64, 127)])
    return _col(generic(), around(np.float32(1.0), 2), scaled, around(u2f([0x00800000]), 2), np.arange(1, 64, dtype=U), SPECIALS)


def unorm8_quotients():
    """c / 255 for c = 0..255, correctly rounded (what the decode LUTs hold)"""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pow_():
    """zr_pow at its call sites: the display gamma pow(Final, 0.4545) over every kind of float, and GetSpecularOcclusion's
    pow(NdotV + AO, r * r) with r = c / 255 and the base on a grid of [0, 2] that includes 0 (so pow(0, 0) occurs)."""
    g = generic()
    gamma = np.stack([g, np.full(len(g), f2u(np.float32(0.4545))[0], dtype=U)], axis=1)
    r = unorm8_quotients()
    rr = (r * r).astype(np.float32)
    base = np.concatenate([np.arange(129, dtype=np.float32) / np.float32(64.0), u2f(around(np.float32(1.0), 2)), u2f([1, 0x00800000])])
    bb, ee = np.meshgrid(base, rr, indexing="ij")
    occl = np.stack([f2u(bb.ravel()), f2u(ee.ravel())], axis=1)
    t = np.concatenate([gamma, occl]).astype(U)
    t.setflags(write=False)
    return t


def pow5():
    return _col(generic(), SPECIALS)


def saturate():
    return _col(generic(), SPECIALS)


def clamp():
    """NaN (quiet and signalling), both zeros and the bounds themselves in each of the three positions, then the two bound pairs the
    shaders use over every kind of t"""
    s = SPECIALS
    a, b, c = np.meshgrid(s, s, s, indexing="ij")
    cube = np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1)
    g = generic()
    pairs = []
    for lo, hi in ((0.0, 1.0), (0.04, 1.0)):
        pairs.append(np.stack([g, np.full(len(g), f2u(np.float32(lo))[0], U), np.full(len(g), f2u(np.float32(hi))[0], U)], axis=1))
    return np.concatenate([cube] + pairs).astype(U)


def unorm():
    rows = []
    g = generic()
    for mx in (3.0, 255.0, 1023.0):
        thr = ((np.arange(int(mx) + 1, dtype=np.float64) + 0.5) / mx).astype(np.float32)
        c = np.concatenate([around(thr, 2), around(np.array([0.0, 1.0], dtype=np.float32), 2), g, SPECIALS])
        rows.append(np.stack([c, np.full(len(c), f2u(np.float32(mx))[0], U)], axis=1))
    return np.concatenate(rows).astype(U)


def f16_codes():
    return np.arange(65536, dtype=U).reshape(-1, 1)


def f32_to_f16():
    """for every non-negative finite half value, the float midway to its successor (a rounding tie) and its two neighbours, both signs;
    the largest half's successor is 65536, so the overflow tie 65520 is among them"""
    h = np.arange(0, 0x7C00, dtype=np.uint16)
    lo = h.view(np.float16).astype(np.float64)
    hi = np.concatenate([lo[1:], [65536.0]])
    mid = ((lo + hi) * 0.5).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (lo + hi) * 0.5)          # the midpoints are floats
    m = around(mid, 1)
    return _col(m, m | U(0x80000000), generic(), SPECIALS)


def unorm8():
    return np.arange(256, dtype=U).reshape(-1, 1)


def div():
    """'/' as the device compiler expands it: denormal operands and quotients, 0/0, x/0, inf/inf, NaN operands"""
    rng = np.random.default_rng(20241)
    g = generic()
    a, b = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    pairs = [np.stack([a.ravel(), b.ravel()], axis=1), np.stack([g, rng.permutation(g)], axis=1), np.stack([g, rng.permutation(g)], axis=1)]
    # quotients that land in the denormal range or on the overflow threshold: numerator and denominator with far-apart exponents
    x = rng.uniform(1.0, 2.0, 8192).astype(np.float32)
    y = rng.uniform(1.0, 2.0, 8192).astype(np.float32)
    e = rng.integers(-149, -120, 8192)
    pairs.append(np.stack([f2u(np.ldexp(x, e // 2).astype(np.float32)), f2u(np.ldexp(y, -(e - e // 2)).astype(np.float32))], axis=1))
    pairs.append(np.stack([f2u(np.ldexp(x, 64).astype(np.float32)), f2u(np.ldexp(y, rng.integers(-66, -62, 8192)).astype(np.float32))], axis=1))
    return np.concatenate(pairs).astype(U)


def sqrt():
    return _col(generic(), SPECIALS)


def vectors(words, n=20000, seed=20242):
    return _mixed(np.random.default_rng(seed + words), (n, words))


# ------------------------------------------------------------------------------------------------------------------ vertex stage (zr_dev.h)

def instance_record():
    """XkInstanceData: Position[3], Rotation[3], PScale, TexIndex.  Every angle of the zr_sincos table in each of the three slots (the
    other two ordinary), with scales {1, 0, -1, denormal, 1e30} and positions that include NaN and infinities."""
    rng = np.random.default_rng(20243)
    ang = sincos()[:, 0]
    rows = []
    scales = f2u(np.array([1.0, 0.0, -1.0, 1e-40, 1e30], dtype=np.float32))
    for slot in range(3):
        t = np.zeros((len(ang), 8), dtype=U)
        t[:, 0:3] = f2u(rng.uniform(-50, 50, (len(ang), 3)).astype(np.float32)).reshape(-1, 3)
        t[:, 3:6] = f2u(rng.uniform(-7, 7, (len(ang), 3)).astype(np.float32)).reshape(-1, 3)
        t[:, 3 + slot] = ang
        t[:, 6] = scales[np.arange(len(ang)) % len(scales)]
        odd = np.arange(len(ang)) % 11 == 0
        t[odd, 0:3] = SPECIALS[rng.integers(0, len(SPECIALS), (int(odd.sum()), 3))]
        t[:, 7] = rng.integers(0, 256, len(ang))
        rows.append(t)
    return np.concatenate(rows)


def _records(rng, n):
    """ZrInstance words: R[9], t[3], s, pad[3]"""
    r = np.zeros((n, 16), dtype=U)
    r[:, :13] = _mixed(rng, (n, 13))
    return r


def vs_position():
    rng = np.random.default_rng(20244)
    n = 20000
    return np.concatenate([_mixed(rng, (n, 3)), _records(rng, n)], axis=1)


def vs_normal():
    rng = np.random.default_rng(20245)
    n = 20000
    flag = (np.arange(n) % 2).astype(U).reshape(-1, 1)
    return np.concatenate([_mixed(rng, (n, 3)), _records(rng, n), _mixed(rng, (n, 16)), flag], axis=1)


@functools.lru_cache(maxsize=None)
def clip_vertices():
    """clip coordinates on and within 1 ulp of every frustum plane and of the guard band (4 w), for w ordinary, zero, negative zero,
    denormal and negative; plus non-finite ones"""
    ws = u2f(np.array([0x3F800000, 0x3F000000, 0x42C80000, 0x3A83126F, 0, 0x80000000, 1, 0x00400000, 0xBF800000], dtype=U))
    out = []
    for w in ws:
        w = np.float32(w)
        xy = np.unique(np.concatenate([around(w, 1), around(-w, 1), around(np.float32(4.0) * w, 1), around(np.float32(-4.0) * w, 1),
                                       f2u(np.array([0.0, 0.5 * w, 5.0 * w], dtype=np.float32))]))
        zs = np.unique(np.concatenate([around(np.float32(0.0), 1), [0x80000000, 0x80000001], around(w, 1), f2u(np.array([0.5 * w, 2.0 * w], dtype=np.float32))]))
        for x in xy:
            for z in zs:
                out.append((x, f2u(np.float32(0.25) * w)[0], z, f2u(w)[0]))
                out.append((f2u(np.float32(-0.25) * w)[0], x, z, f2u(w)[0]))
    for s in (INF, 0xFF800000, NAN_Q, NAN_S, 0x7F7FFFFF):
        for k in range(4):
            v = [f2u(np.float32(0.1))[0], f2u(np.float32(0.2))[0], f2u(np.float32(0.5))[0], 0x3F800000]
            v[k] = s
            out.append(tuple(v))
    rng = np.random.default_rng(20250)              # ordinary vertices, inside the guard band and around it
    w = rng.uniform(0.1, 50.0, 600).astype(np.float32)
    xy = (rng.uniform(-4.5, 4.5, (600, 2)).astype(np.float32) * w[:, None]).astype(np.float32)
    z = (rng.uniform(-0.05, 1.2, 600).astype(np.float32) * w).astype(np.float32)
    v = np.concatenate([np.array(out, dtype=U), f2u(np.column_stack([xy, z, w])).reshape(-1, 4)])
    v.setflags(write=False)
    return v


def classify():
    """triangles of clip_vertices(): every vertex three times over (vertex_flags alone decides), with an inside vertex twice, and random triples"""
    rng = np.random.default_rng(20246)
    v = clip_vertices()
    inside = np.tile(np.array([0, 0, 0x3F000000, 0x3F800000], dtype=U), (len(v), 1))
    same = np.concatenate([v, v, v], axis=1)
    one = np.concatenate([v, inside, inside], axis=1)
    idx = rng.integers(0, len(v), (40000, 3))
    rnd = np.concatenate([v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]], axis=1)
    return np.concatenate([same, one, rnd]).astype(U)


def projectable(v):
    """what project()'s callers guarantee of each corner of a triangle that classify() put on the fast path: finite, z >= 0, w > 0, inside
    the guard band (the edge of that set included)"""
    c = u2f(v).reshape(-1, 4)
    with np.errstate(all="ignore"):
        g = np.float32(4.0) * c[:, 3]
        return (np.isfinite(c).all(axis=1) & ~(c[:, 2] < 0) & (c[:, 3] > 0) & ~(np.abs(c[:, 0]) > g) & ~(np.abs(c[:, 1]) > g))


def project():
    v = clip_vertices()
    v = v[projectable(v)]
    rows = []
    for hw, hh in ((640.0, 360.0), (0.5, 0.5), (2048.0, 2048.0), (127.5, 72.5)):
        rows.append(np.concatenate([v, np.tile(f2u(np.array([hw, hh], dtype=np.float32)), (len(v), 1))], axis=1))
    return np.concatenate(rows).astype(U)


# ------------------------------------------------------------------------------------------------------------------ shading (zr_shade.h)

def _unit_grid():
    one = np.float32(1.0)
    return np.concatenate([np.array([0.0, 1e-40, 1e-3, 0.25, 0.5, 0.75], dtype=np.float32), u2f(around(one, 1))[:2], u2f([NAN_Q])])


def _rough_grid():
    q = unorm8_quotients()
    return np.concatenate([q[[0, 1, 2, 3, 64, 127, 128, 254, 255]], np.array([0.001, 0.01], dtype=np.float32)])


def _grid(*axes):
    m = np.meshgrid(*axes, indexing="ij")
    return np.stack([f2u(a.ravel()) for a in m], axis=1)


def F_Schlick():
    """its two uses: (0.04, 1, LdotH) in DefaultLitBxDF and (1, fd90, u) in Fr_DisneyDiffuse, fd90 in [0, 2.5]"""
    u = _unit_grid()
    a = _grid(np.array([0.04], dtype=np.float32), np.array([1.0], dtype=np.float32), u)
    b = _grid(np.array([1.0], dtype=np.float32), np.linspace(0.0, 2.5, 41, dtype=np.float32), u)
    return np.concatenate([a, b])


def Fr_DisneyDiffuse():
    u = _unit_grid()
    return _grid(u, u, u, _rough_grid())


def V_SmithGGXCorrelated():
    u = _unit_grid()
    return _grid(u, u, _rough_grid())


def D_GGX():
    """NdotH = 1 with r = 0 is 0 / 0"""
    rng = np.random.default_rng(20247)
    dense = np.concatenate([_unit_grid(), rng.uniform(0, 1, 300).astype(np.float32)])
    return _grid(dense, np.concatenate([_rough_grid(), unorm8_quotients()]))


def shadow_maps(dim):
    """the maps of a shadow_tap table: random depths in [0, 1], the cleared map (all 1), and a constant map whose texels are the very
    value the cases use for sz (the `dist < sz` tie)"""
    rng = np.random.default_rng(20248 + dim)
    return {"random": rng.uniform(0, 1, (dim, dim)).astype(np.float32), "cleared": np.ones((dim, dim), dtype=np.float32),
            "tie": np.full((dim, dim), SHADOW_TIE, dtype=np.float32)}


SHADOW_TIE = np.float32(0.625)


def shadow_tap(dim):
    """cases sx, sy, sz, sw, ox, oy for a map of edge dim: the interior, every edge and corner (texel centres +- 2 texels around 0 and 1,
    where the clamp acts), sz at +-1 +- ulp, at the tie value and around it, sw zero, negative and denormal, the PCF's offsets"""
    rng = np.random.default_rng(20249 + dim)
    d = np.float32(dim)
    dxy = np.float32(1.5) * np.float32(1.0) / d
    edge = np.concatenate([(np.arange(-2, 3, dtype=np.float32) * np.float32(0.5)) / d, np.float32(1.0) + (np.arange(-2, 3, dtype=np.float32) * np.float32(0.5)) / d])
    xs = np.concatenate([edge, rng.uniform(0, 1, 24).astype(np.float32), np.array([-3.0, 7.0, np.nan, np.inf], dtype=np.float32)])
    szs = np.concatenate([u2f(around(np.float32(1.0), 1)), u2f(around(np.float32(-1.0), 1)), u2f(around(SHADOW_TIE, 1)),
                          np.array([0.0, 0.3, 0.9, np.nan], dtype=np.float32)])
    sws = u2f(np.array([0x3F800000, 0, 0x80000000, 0xBF800000, 1, NAN_Q], dtype=U))
    offs = (dxy * np.arange(-2, 3, dtype=np.float32)).astype(np.float32)
    base = _grid(xs, xs, szs, sws)
    k = rng.integers(0, 5, (len(base), 2))
    return np.concatenate([base, f2u(offs[k[:, 0]]).reshape(-1, 1), f2u(offs[k[:, 1]]).reshape(-1, 1)], axis=1)


# ------------------------------------------------------------------------------------------------------------------ the registry

# the probe's function ids (the enum of tests/device_probe/probe.hip, in order); the oracle's batch export is zo_kat_<name>_batch
PROBE_FUNCTIONS = ["rsqrt", "sincos", "exp2", "log2", "pow", "pow5", "saturate", "clamp", "unorm", "f16_to_f32", "f32_to_f16", "unorm8",
                   "div", "sqrt", "dot", "cross", "normalize", "tangent_normal", "mat4_point",
                   "instance_record", "vs_position", "vs_normal", "classify", "project",
                   "F_Schlick", "Fr_DisneyDiffuse", "V_SmithGGXCorrelated", "D_GGX", "shadow_tap"]
WORDS = {"rsqrt": (1, 1), "sincos": (1, 2), "exp2": (1, 1), "log2": (1, 1), "pow": (2, 1), "pow5": (1, 1), "saturate": (1, 1), "clamp": (3, 1),
         "unorm": (2, 1), "f16_to_f32": (1, 1), "f32_to_f16": (1, 1), "unorm8": (1, 1), "div": (2, 1), "sqrt": (1, 1), "dot": (6, 1),
         "cross": (6, 3), "normalize": (3, 3), "tangent_normal": (3, 3), "mat4_point": (19, 4), "instance_record": (8, 16),
         "vs_position": (19, 3), "vs_normal": (36, 3), "classify": (12, 1), "project": (6, 4), "F_Schlick": (3, 1),
         "Fr_DisneyDiffuse": (4, 1), "V_SmithGGXCorrelated": (3, 1), "D_GGX": (2, 1), "shadow_tap": (6, 1)}
# which output words are floats (a NaN there matches any NaN); the others are integers and must be equal
FLOAT_WORDS = {n: [True] * WORDS[n][1] for n in PROBE_FUNCTIONS}
FLOAT_WORDS.update({"unorm": [False], "f32_to_f16": [False], "classify": [False], "project": [False, False, True, True]})
# the table generator of a function, where it is not named after it
TABLE_OF = {"pow": "pow_", "f16_to_f32": "f16_codes", "dot": "vectors6", "cross": "vectors6", "normalize": "vectors3", "tangent_normal": "vectors3",
            "mat4_point": "vectors19"}


def vectors3():
    return vectors(3)


def vectors6():
    return vectors(6)


def vectors19():
    return vectors(19)


def oracle_batch(L, name, table, shadow_map=None):
    """the oracle's results for a table: one ctypes call"""
    import ctypes as C
    table = np.ascontiguousarray(table, dtype=U)
    assert table.ndim == 2 and table.shape[1] == WORDS[name][0], (name, table.shape)
    out = np.zeros((len(table), WORDS[name][1]), dtype=U)
    f = getattr(L, "zo_kat_%s_batch" % name)
    f.restype = None
    if name == "shadow_tap":
        mp = np.ascontiguousarray(shadow_map, dtype=np.float32)
        assert mp.ndim == 2 and mp.shape[0] == mp.shape[1]
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        f(table.ctypes.data, out.ctypes.data, len(table), mp.ctypes.data, mp.shape[0])
    else:
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        f(table.ctypes.data, out.ctypes.data, len(table))
    return out


# ------------------------------------------------------------------------------------------------------------------ functions that read a scene
# cube_sample, the PCF block and shade_surface read a cubemap, a shadow map and an XkView besides their case.  A Scene holds those; the GPU
# test hands it to the probe (zp_run_scene) and to an oracle context (zo_set_cubemap, zo_set_frame, zo_kat_set_shadowmap).

PROBE_FUNCTIONS += ["cube_sample", "pcf_taps", "shade", "shade_masked"]
WORDS.update({"cube_sample": (4, 3), "pcf_taps": (3, 1), "shade": (23, 10), "shade_masked": (23, 10)})
FLOAT_WORDS.update({n: [True] * WORDS[n][1] for n in ("cube_sample", "pcf_taps", "shade", "shade_masked")})
IDENTITY = np.eye(4, dtype=np.float32).ravel()


def cube_faces(dim, seed=20260):
    """six dim x dim RGBA8 faces of random texels, with the extreme codes 0 and 255 present"""
    rng = np.random.default_rng(seed + dim)
    f = rng.integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
    f[0, 0, 0] = 0
    f[5, -1, -1] = 255
    return f


class Scene:
    def __init__(self, map_dim=8, shadow_map=None, cube_dim=2, SB=IDENTITY, view=None):
        from zeldaengine_amd import abi
        self.map_dim = map_dim
        self.map = np.ascontiguousarray(np.ones((map_dim, map_dim), np.float32) if shadow_map is None else shadow_map, dtype=np.float32)
        assert self.map.shape == (map_dim, map_dim)
        self.cube_dim = cube_dim
        self.faces = cube_faces(cube_dim)
        self.SB = np.ascontiguousarray(SB, dtype=np.float32)
        self.view = np.zeros((), dtype=abi.XkView) if view is None else view
        self.dxy = np.float32(1.5) * np.float32(1.0) / np.float32(map_dim)

    def oracle(self, pyoracle):
        """an oracle context holding this scene; the view's CubemapMaxMips is the chain's length, as zo_set_cubemap sets it"""
        o = pyoracle.Oracle(16, 16, self.map_dim)
        o.set_cubemap(list(self.faces))
        cam, sh, v = o.get_frame()
        self.levels = int(v["LightsCount"][3])
        self.view["LightsCount"][3] = self.levels
        o.set_frame(cam, sh, self.view)
        assert o.L.zo_kat_set_shadowmap(o.h, self.map.ctypes.data, self.map_dim) == 0
        self.mips = o.cube_mips(self.cube_dim)
        assert len(self.mips) == self.levels
        self.lut = np.array([o.L.zo_kat_srgb8_to_linear(c) for c in range(256)], dtype=np.float32)
        return o

    def oracle_batch(self, o, name, table):
        import ctypes as C
        table = np.ascontiguousarray(table, dtype=U)
        assert table.ndim == 2 and table.shape[1] == WORDS[name][0], (name, table.shape)
        out = np.zeros((len(table), WORDS[name][1]), dtype=U)
        L = o.L
        vp = C.c_void_p
        if name == "cube_sample":
            L.zo_kat_cube_sample_batch.argtypes = [vp, vp, vp, C.c_uint32]
            L.zo_kat_cube_sample_batch(o.h, table.ctypes.data, out.ctypes.data, len(table))
        elif name == "pcf_taps":
            L.zo_kat_pcf_batch.argtypes = [vp, vp, C.c_float, vp, vp, C.c_uint32]
            L.zo_kat_pcf_batch(o.h, self.SB.ctypes.data, float(self.dxy), table.ctypes.data, out.ctypes.data, len(table))
        else:
            L.zo_kat_shade_batch.argtypes = [vp, vp, C.c_float, C.c_int, vp, vp, C.c_uint32]
            L.zo_kat_shade_batch(o.h, self.SB.ctypes.data, float(self.dxy), int(name == "shade_masked"), table.ctypes.data, out.ctypes.data, len(table))
        return out


def cube_sample(dim):
    """directions on every face, on the face ties (|x| = |y|, |y| = |z|, |x| = |z|, all three, either sign), the zero vector, NaN and
    infinite components; lod below 0, at each integer level, between levels, above the last level, NaN"""
    rng = np.random.default_rng(20261 + dim)
    levels = int(np.log2(dim)) + 1
    one = np.float32(1.0)
    near1 = u2f(around(one, 1))
    dirs = [rng.uniform(-1, 1, (300, 3)).astype(np.float32)]
    tie = []
    for a in (-1.0, 1.0):
        for b in (-1.0, 1.0):
            for c in (0.3, -0.3, 1.0, -1.0, 0.0):
                tie += [(a, b, c), (a, c, b), (c, a, b)]
            for m in near1:                                   # one ulp either side of a tie
                tie += [(a, b * m, 0.5), (0.5, a, b * m), (a * m, 0.5, b)]
    dirs.append(np.array(tie, dtype=np.float32))
    dirs.append(np.array([(0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, 1, 0), (1, np.nan, 0), (0, 1, np.nan), (np.inf, 1, 0), (np.inf, np.inf, 1),
                          (1e-40, 0, 0), (3e38, 3e38, -3e38), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)], dtype=np.float32))
    # the edge of a face: sc / ma = +-1 puts the footprint on the last texel and past it (clamp to edge)
    dirs.append(np.array([(1, 1 - 2.0 ** -k, s * (1 - 2.0 ** -j)) for k in (1, 4, 12, 24) for j in (1, 4, 12, 24) for s in (-1, 1)], dtype=np.float32))
    d = np.concatenate(dirs)
    lods = np.concatenate([np.arange(levels + 2, dtype=np.float32) - 1, np.array([-0.0, 0.25, 0.5, levels - 1.5, 1e9, -1e9, np.inf, -np.inf, np.nan], dtype=np.float32),
                           u2f(around(np.float32(max(levels - 1, 1)), 1))])
    di, li = np.meshgrid(np.arange(len(d)), np.arange(len(lods)), indexing="ij")
    return np.concatenate([f2u(d[di.ravel()]).reshape(-1, 3), f2u(lods[li.ravel()]).reshape(-1, 1)], axis=1)


def pcf_columns(sx, dim):
    """the texel columns cx0[k], cx1[k] of the PCF's five x offsets for float32 sx, as shade_surface forms them (fp32: sx + off, then one
    fma); returns (cx0, cx1, pattern, p1, p3)"""
    d = np.float64(dim)
    dxy = np.float32(1.5) * np.float32(1.0) / np.float32(dim)
    cx0, cx1 = [], []
    with np.errstate(all="ignore"):
        for k in range(5):
            off = np.float32(dxy * np.float32(k - 2))
            u = ((sx.astype(np.float32) + off).astype(np.float32).astype(np.float64) * d - 0.5).astype(np.float32)
            fu = np.floor(u)
            cl = lambda f: np.where(np.isnan(f), 0, np.clip(f, 0, dim - 1)).astype(np.int64)      # noqa: E731
            cx0.append(cl(fu)); cx1.append(cl(fu + np.float32(1)))
    cb = cx0[0]
    p1, p3 = cx0[1] == cb + 2, cx0[3] == cb + 5
    pattern = ((cx1[0] == cb + 1) & ((cx0[1] == cb + 1) | p1) & (cx1[1] == cx0[1] + 1) & (cx0[2] == cb + 3) & (cx1[2] == cb + 4) &
               ((cx0[3] == cb + 4) | p3) & (cx1[3] == cx0[3] + 1) & (cx0[4] == cb + 6) & (cx1[4] == cb + 7))
    return cx0, cx1, pattern, p1, p3


def pcf_points(dim):
    """P for the PCF block under SB = identity-with-a-chosen-w (sx = P.x / w ...): x across the interior in tenth-texel steps over two
    texels at three places (both values of p1 and of p3 occur), x at and beyond both map edges (the pattern fails, the per-texel path runs),
    y likewise but coarser, z at +-1 +- ulp, at the tie value and around it, and inside"""
    d = np.float32(dim)
    steps = np.arange(0, 20, dtype=np.float32) / np.float32(10.0)
    xs = [(np.float32(c) + steps + np.float32(0.5)) / d for c in ((3.0, dim / 2.0, dim - 6.0) if dim > 8 else (3.0,))]
    xs.append((np.arange(-4, 9, dtype=np.float32) * np.float32(0.5)) / d)                       # the left edge and beyond
    xs.append(np.float32(1.0) + (np.arange(-8, 5, dtype=np.float32) * np.float32(0.5)) / d)     # the right edge and beyond
    xs.append(np.array([np.nan, -50.0, 50.0], dtype=np.float32))
    x = np.concatenate(xs).astype(np.float32)
    y = np.concatenate([(np.arange(-3, 4, dtype=np.float32) * np.float32(0.7)) / d, np.float32(1.0) + (np.arange(-3, 4, dtype=np.float32) * np.float32(0.7)) / d,
                        np.array([0.31, 0.52, 0.77], dtype=np.float32)]).astype(np.float32)
    z = np.concatenate([u2f(around(np.float32(1.0), 1)), u2f(around(np.float32(-1.0), 1)), u2f(around(SHADOW_TIE, 1)), np.array([0.3, 0.9], dtype=np.float32)])
    return _grid(x, y, z)


# w of the shadow-space position: the last entry of SB (column-major m[15]) with the other three of its row zero
PCF_W = {"one": 1.0, "two": 2.0, "zero": 0.0, "negative": -1.0, "denormal": 1e-40}


def pcf_SB(w):
    m = IDENTITY.copy()
    m[15] = np.float32(w)
    return m


# BiasMat * shadowmapSpace of the shade tables: an orthographic light looking down -z over [-4, 4]^2, depth 0.5 - z / 8: the surface
# points land inside the map with sz inside (-1, 1), so the PCF runs
SHADE_SB = np.array([0.125, 0, 0, 0,  0, 0.125, 0, 0,  0, 0, -0.125, 0,  0.5, 0.5, 0.5, 1], dtype=np.float32)
ROUGHNESS_SWITCH = np.float32(0.001)          # max(Roughness, 0.001) of ComputeReflectionMipFromRoughness


def _decode_normal(code):
    """a GBufferA normal code (10 bits per component) as the lighting pass unpacks it: c / 1023 * 2 - 1"""
    c = np.asarray(code, dtype=np.float32) / np.float32(1023.0)
    return (c * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def shade_view(nDir, nPoint, roll=0, poison=False):
    """an XkView with nDir directional and nPoint point lights.  The surface points of shade_cases() sit at the origin (and nearby), so a
    light placed at (d, 0, 0) is at distance exactly d from the origin: the first point lights are, in an order rolled by `roll`, at the
    origin itself (d2 = 0); at exactly the falloff distance and within +-1e-5, +-1e-6, +-2e-7 relative of it (both sides of the
    d2 > falloff^2 * 1.000001 early-out, which the oracle does not have); with falloff negative and infinite.  The rest are random lights
    of which some reach the origin and some do not.  poison: also lights whose contribution is NaN for every surface - falloff 0 and NaN,
    colours that hold inf and NaN (within reach and out of reach: `lfinite` false, no skip) - and an infinite directional colour.  Those
    go into views of their own, because a NaN sum matches any NaN and would hide the other lights' terms."""
    from zeldaengine_amd import abi
    rng = np.random.default_rng(20262)
    v = np.zeros((), dtype=abi.XkView)
    v["LightsCount"][:] = (nDir, nPoint, 0, 0)
    dirs = [((0.3, -0.5, -0.8), (1.0, 0.9, 0.8, 2.0)), ((-0.2, 0.1, 0.97), (0.2, 0.4, np.inf if poison else 0.7, 1.0))]
    for i in range(nDir):
        v["DirectionalLights"][i]["Direction"][:3] = dirs[i][0]
        v["DirectionalLights"][i]["Color"][:] = dirs[i][1]
    special = []
    f = np.float32(2.5)
    for rel in (0.0, 1e-5, -1e-5, 1e-6, -1e-6, 2e-7, -2e-7):
        special.append(((np.float32(np.float64(f) * (1.0 + rel)), 0.0, 0.0), f, (1.0, 0.8, 0.6, 3.0)))
    special.append(((0.0, 0.0, 0.0), np.float32(3.0), (1.0, 1.0, 1.0, 2.0)))                    # at the surface point itself
    for fo in (-1.0, np.inf):
        special.append(((0.5, 0.7, 0.4), np.float32(fo), (0.9, 0.7, 0.5, 2.0)))
    special.append(((1e20, 0.0, 0.0), np.float32(2.0), (0.9, 0.7, 0.5, 2.0)))                   # so far away that d2 overflows
    if poison:
        bad = [((0.5, 0.7, 0.4), np.float32(fo), (0.9, 0.7, 0.5, 2.0)) for fo in (0.0, np.nan)]
        for col in ((np.inf, 1.0, 1.0, 1.0), (1.0, np.nan, 1.0, 1.0), (1.0, 1.0, 1.0, np.inf), (1.0, 1.0, -np.inf, 2.0)):
            bad.append(((0.4, -0.3, 0.6), np.float32(4.0), col))
            bad.append(((9.0, 9.0, 9.0), np.float32(1.0), col))                                  # out of reach, colour not finite: no skip
        special = bad + special
    special = special[roll % len(special):] + special[:roll % len(special)]
    for i in range(nPoint):
        L = v["PointLights"][i]
        if i < len(special):
            pos, fo, col = special[i]
        else:
            pos = rng.uniform(-3, 3, 3)
            fo = np.float32(rng.uniform(0.5, 6.0))
            col = (*rng.uniform(0, 1, 3), rng.uniform(0.5, 4.0))
        L["Position"][:3] = pos
        L["Direction"][3] = fo
        L["Color"][:] = col
    return v


def shade_cases(nPoint, seed=0):
    """cases of shade_surface: cam, BaseColor, Metallic, Roughness, N, AO, P, 8 mask words.  Surfaces: Roughness {0, 1/255, the
    max(r, 0.001) switch and its neighbours, 0.5, 1} x Metallic {0, 1/2, 1} x AO {0, 1} x BaseColor {0, 0.04 +- ulp, 1}; geometry: normals
    decoded from GBuffer codes (extremes included), N perpendicular to V, N = -V, the camera at P; P at the origin (where shade_view's
    lights are exact) and nearby.  Masks by case: all ones (beyond nPoint too), empty, only the last valid bit, only bits beyond nPoint,
    random."""
    rng = np.random.default_rng(20263 + seed)
    q = unorm8_quotients()
    rough = np.concatenate([[0.0, q[1]], u2f(around(ROUGHNESS_SWITCH, 1)), [0.5, 1.0]]).astype(np.float32)
    metal = np.array([0.0, 0.5, 1.0], dtype=np.float32)
    ao = np.array([0.0, 1.0], dtype=np.float32)
    base = np.concatenate([[0.0], u2f(around(np.float32(0.04), 1)), [1.0]]).astype(np.float32)
    cam0 = np.array([1.5, -2.0, 2.5], dtype=np.float32)
    origin = np.zeros(3, dtype=np.float32)
    geo = []                                         # (cam, N, P)
    for code in ((1023, 512, 512), (0, 0, 0), (1023, 1023, 1023), (512, 512, 1023), (511, 512, 0), (700, 300, 900)):
        geo.append((cam0, _decode_normal(code), origin))
    geo.append((cam0, np.array([2.0, 1.5, 0.0], dtype=np.float32), origin))                      # N . V = 0 exactly: 1.5 * 2 - 2 * 1.5
    geo.append((cam0, -cam0, origin))                                                            # N = -V
    geo.append((origin, np.array([0.0, 0.0, 1.0], dtype=np.float32), origin))                    # cam == P
    geo.append((cam0, np.array([0.0, 0.0, 0.0], dtype=np.float32), origin))                      # a zero normal
    geo.append((cam0, np.array([0.1, 0.2, 0.97], dtype=np.float32), np.array([0.25, -0.5, 0.125], dtype=np.float32)))
    geo.append((cam0, np.array([-0.6, 0.3, 0.7], dtype=np.float32), np.array([-1.0, 2.0, 0.5], dtype=np.float32)))
    rows = []
    for cam, N, P in geo:
        for r in rough:
            for m in metal:
                for a in ao:
                    for b in base:
                        rows.append(np.concatenate([cam, [b, b * np.float32(0.5), b], [m, r], N, [a], P]))
    t = np.zeros((len(rows), 23), dtype=U)
    t[:, :15] = f2u(np.array(rows, dtype=np.float32)).reshape(-1, 15)
    kind = np.arange(len(t)) % 5
    words = (max(nPoint, 1) + 31) // 32
    m = np.zeros((len(t), 8), dtype=U)
    m[kind == 0] = 0xFFFFFFFF
    if nPoint:
        m[kind == 2, (nPoint - 1) >> 5] = U(1) << U((nPoint - 1) & 31)
    beyond = np.zeros(8, dtype=U)
    for bit in range(nPoint, 256):
        beyond[bit >> 5] |= U(1) << U(bit & 31)
    m[kind == 3] = beyond
    rnd = rng.integers(0, 1 << 32, (len(t), 8), dtype=np.uint64).astype(U)
    rnd[:, words:] = rng.integers(0, 2, (len(t), 1)).astype(U) * rnd[:, words:]               # half of them with bits beyond the last word too
    m[kind == 4] = rnd[kind == 4]
    t[:, 15:] = m
    return t


def shade_all_ones(table):
    t = table.copy()
    t[:, 15:] = 0xFFFFFFFF
    return t


# (nDir, nPoint, poison): every pair of counts with finite lights; the NaN-making lights in three views of their own
SHADE_VIEWS = [(nd, npt, False) for nd in (0, 1, 2) for npt in (0, 1, 31, 32, 33, 64, 256)] + [(2, 1, True), (1, 33, True), (0, 256, True)]
