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


# ------------------------------------------------------------------------------------------------------------------ the sampler (zr_texture.h)
# tex_footprint reads its case alone.  tex_image, tex_material and tex_packed read a material's images besides the case: a Textures holds
# seven slots, the GPU test hands them to the probe (zp_run_textures) and to an oracle context (zo_kat_set_image), whose mip chains both use.

PROBE_FUNCTIONS += ["tex_footprint", "tex_image", "tex_material", "tex_packed", "bary_screen", "bary_homog", "interp", "compute_normal",
                    "model_point", "f32_to_f16_hw", "f16_to_f32_hw"]
WORDS.update({"tex_footprint": (7, 4), "tex_image": (6, 4), "tex_material": (6, 28), "tex_packed": (6, 13), "bary_screen": (11, 3),
              "bary_homog": (16, 3), "interp": (12, 4), "compute_normal": (16, 3), "model_point": (20, 3), "f32_to_f16_hw": (1, 1),
              "f16_to_f32_hw": (1, 1)})
FLOAT_WORDS.update({n: [True] * WORDS[n][1] for n in PROBE_FUNCTIONS[-11:]})
FLOAT_WORDS.update({"tex_footprint": [False, True, True, True], "f32_to_f16_hw": [False]})
TABLE_OF.update({"interp": "vectors12", "f32_to_f16_hw": "f32_to_f16", "f16_to_f32_hw": "f16_codes"})
# the oracle's export where it is not zo_kat_<name>_batch: the half conversions are the existing batches
ORACLE_OF = {"f32_to_f16_hw": "f32_to_f16", "f16_to_f32_hw": "f16_to_f32"}
_oracle_batch_plain = oracle_batch


def oracle_batch(L, name, table, shadow_map=None):     # noqa: F811
    if name in ORACLE_OF:
        assert WORDS[ORACLE_OF[name]] == WORDS[name]
        return _oracle_batch_plain(L, ORACLE_OF[name], table)
    return _oracle_batch_plain(L, name, table, shadow_map)


def vectors12():
    return vectors(12)


# (w, h) of the single-image runs.  16384 is the largest side the product's host accepts.
IMAGE_SETS = [(1, 1), (1, 16), (16, 1), (2, 2), (33, 7), (48, 20), (64, 64), (128, 4), (16384, 1), (1, 16384)]
MAX_ANISO = 16


def levels_of(w, h):
    return int(max(w, h)).bit_length()


def level_size(w, h, level):
    return max(1, w >> level), max(1, h >> level)


def noise_image(w, h, seed=0):
    """(h, w, 4) random RGBA8 with the codes 0 and 255 present where there is room"""
    rng = np.random.default_rng(20270 + 131 * w + h + seed)
    im = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if w * h >= 2:
        im.reshape(-1, 4)[0] = 0
        im.reshape(-1, 4)[-1] = 255
    return im


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _pow2_below(x):
    """the power of two 2^-k nearest 1 / x from below (a float with one mantissa bit)"""
    return np.float32(2.0 ** -int(np.ceil(np.log2(x))))


def footprint_breakpoints(w, h):
    """(rows of dudx, dvdx, dudy, dvdy, N, major, ulps): for N = 1..16 a footprint whose Pmax^2 / Pmin^2 is EXACTLY N^2 - the major axis
    along u with derivative N h t, the minor along v with derivative w t, t a power of two: both products with the image's size are
    N w h t and w h t, exact in float32, and so are their squares and N^2 times the lesser (test_device_function_tables.py checks this in
    rational arithmetic) - then the same with the major derivative moved by -2..2 ulp.  Either screen axis as the major one; N = 1 is the
    tie rx2 == ry2, which goes to x."""
    rows = []
    for t in (_pow2_below(w * h), np.float32(_pow2_below(w * h) * np.float32(8.0))):
        for N in range(1, MAX_ANISO + 1):
            major, minor = np.float32(np.float32(N * h) * t), np.float32(np.float32(w) * t)
            for d in range(-2, 3):
                m = u2f(np.array([int(f2u(major)[0]) + d], dtype=U))[0]
                rows.append((m, 0.0, 0.0, minor, N, 0, d))            # x is the major axis: (dudx, dvdx) = (major, 0), (dudy, dvdy) = (0, minor)
                rows.append((0.0, minor, m, 0.0, N, 1, d))            # y is
    return np.array(rows, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def footprints(w, h):
    """the derivative quadruples (dudx, dvdx, dudy, dvdy) of an image set's tables, as float32 rows"""
    rng = np.random.default_rng(20271 + 131 * w + h)
    L = levels_of(w, h)
    W, H = np.float64(w), np.float64(h)
    rows = [footprint_breakpoints(w, h)[:, :4].astype(np.float32)]
    sp = []
    d = np.float32(1.0 / 64)
    sp += [(d, 0, 0, 0), (0, d, 0, 0), (0, 0, d, 0), (0, 0, 0, d), (0, 0, 0, 0), (-0.0, 0, 0, -0.0), (-d, -0.0, 0, d)]     # rmin2 = 0 (N = 16); both 0; -0
    # lambda on every integer of the chain (and one below, one above) +- 2 ulp: an isotropic footprint of 2^l texels, and a 4:1 one of 4 * 2^l
    for l in range(-1, L + 1):
        for du in u2f(around(np.float32(2.0 ** l / W), 2)):
            sp += [(du, 0, 0, np.float32(2.0 ** l / H)), (0, np.float32(2.0 ** l / H), du, 0)]
        for du in u2f(around(np.float32(4.0 * 2.0 ** l / W), 2)):
            sp += [(du, 0, 0, np.float32(2.0 ** l / H))]
    # denormal products (squares that underflow), products that overflow
    for a in (1e-19, 1e-20, 1e-22, 1e-23, 1e-30, 1e-40):
        sp += [(a, 0, 0, a), (a, a, 0, 1e-21), (0, 1e-22, a, 0), (a, 0, 0, 0.01)]
    for a in (3e38, -3e38, 1e19, 2e19):
        sp += [(a, 0, 0, a), (a, 0, 0, 0.01), (0.01, 0, 0, a), (a, a, a, a), (0, a, 1e-3, 0)]
    for s in (np.inf, -np.inf, np.nan):
        for k in range(4):
            for base in ((0.01, 0.0, 0.0, 0.02), (0.0, 0.0, 0.0, 0.0), (0.05, 0.01, -0.01, 0.002)):
                v = list(base)
                v[k] = s
                sp.append(tuple(v))
    sp += [(np.inf, 0, 0, np.inf), (np.nan, np.nan, np.nan, np.nan), (np.inf, np.inf, np.inf, np.inf)]
    rows.append(np.array(sp, dtype=np.float32))
    # ordinary footprints: a scale from an eighth of a texel to beyond the whole image, any direction, ratios from 1 to beyond 16
    n = 1500
    scale = 2.0 ** rng.uniform(-3.0, L + 0.5, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    ratio = rng.choice([1.0, 1.2, 1.37, 1.8, 2.4, 2.9, 3.6, 4.5, 5.5, 6.4, 7.5, 8.6, 9.5, 10.4, 11.3, 12.5, 13.6, 14.4, 15.6, 17.0, 40.0], n)
    major = np.stack([np.cos(ang) / W, np.sin(ang) / H], axis=1) * scale[:, None]
    minor = np.stack([-np.sin(ang) / W, np.cos(ang) / H], axis=1) * (scale / ratio)[:, None]
    swap = (np.arange(n) % 2 == 0)[:, None]
    rows.append(np.concatenate([np.where(swap, minor, major), np.where(swap, major, minor)], axis=1).astype(np.float32))
    f = np.concatenate(rows).astype(np.float32)
    f.setflags(write=False)
    return f


def tex_footprint(w, h):
    f = footprints(w, h)
    head = np.tile(np.array([w, h, levels_of(w, h)], dtype=U), (len(f), 1))
    return np.concatenate([head, f2u(f).reshape(-1, 4)], axis=1)


def _axis_coordinates(n, rng):
    """coordinates along an axis of n texels: every texel centre and every texel edge k / n +- 1 ulp of levels 0 and 1; 0, 1, -0; the
    largest negative float (u - floor(u) rounds to exactly 1); values in [-3, 4]; 2^23 + 0.5, 1e30, 3e38; +-inf, NaN"""
    out = []
    for m in (n, max(1, n >> 1)):
        k = np.arange(m + 1, dtype=np.float64)
        out.append(f2u(((k[:-1] + 0.5) / m).astype(np.float32)))
        out.append(around((k / m).astype(np.float32), 1))
    out.append(np.array([0, 0x3F800000, 0x80000000, 0x80000001, 0x3F7FFFFF, 0xBF800000, 0x3F000000], dtype=U))
    out.append(f2u(rng.uniform(-3.0, 4.0, 400).astype(np.float32)))
    out.append(f2u(np.array([2.0 ** 23 + 0.5, -(2.0 ** 23 + 0.5), 1e30, -1e30, 3e38, np.inf, -np.inf, np.nan, 1e-40, -1e-40], dtype=np.float32)))
    return np.unique(np.concatenate(out))


WRAP_COORDS = np.array([0, 0x80000000, 0x80000001, 0x3F7FFFFF, 0x3F800000, 0x3F000000], dtype=U)     # 0, -0, -tiny, 1 - ulp, 1, 0.5


@functools.lru_cache(maxsize=None)
def tex_cases(w, h, cap=250000):
    """cases u, v, dudx, dvdx, dudy, dvdy for a w x h image: every coordinate of _axis_coordinates on either axis and every footprint of
    footprints() at least once, paired by a seeded shuffle; then the wrap block - the coordinates next to 0 and 1 on both axes under a
    single-tap footprint on every level of the chain, so that both wraps of both axes are reached on every level."""
    rng = np.random.default_rng(20272 + 131 * w + h)
    cu, cv, f = _axis_coordinates(w, rng), _axis_coordinates(h, rng), f2u(footprints(w, h)).reshape(-1, 4)
    n = min(cap - 2000, max(len(cu), len(cv), len(f), 6000) * 2)
    assert n >= max(len(cu), len(cv), len(f)), (w, h)

    def spread(m):
        return rng.permutation(np.concatenate([np.arange(m), rng.integers(0, m, n - m)]))
    body = np.concatenate([cu[spread(len(cu))].reshape(-1, 1), cv[spread(len(cv))].reshape(-1, 1), f[spread(len(f))]], axis=1)
    wrap = []
    for l in range(levels_of(w, h)):
        for lam in (l, l + 0.5):
            fp = f2u(np.array([2.0 ** lam / w, 0, 0, 2.0 ** lam / h], dtype=np.float32))
            for a in WRAP_COORDS:
                for b in WRAP_COORDS:
                    wrap.append(np.concatenate([[a, b], fp]))
    t = np.concatenate([body, np.array(wrap, dtype=U)]).astype(U)
    assert len(t) <= cap
    t.setflags(write=False)
    return t


def tap_addresses(w, h, case_bits, lam):
    """for single-tap cases (N = 1): the level pair and, on level l0, floor(x) and floor(y) of zr_texture.h's addressing (x = fma(u - floor u, w_l, -0.5)),
    restated for the coverage claims only.  Returns l0, l1, fx, fy, w_l0, h_l0."""
    L = levels_of(w, h)
    c = u2f(case_bits[:, :2]).reshape(-1, 2)
    with np.errstate(all="ignore"):
        l0 = np.floor(lam).astype(np.int64)
        l1 = np.minimum(l0 + 1, L - 1)
        wl, hl = np.maximum(1, w >> l0), np.maximum(1, h >> l0)
        r = (c - np.floor(c)).astype(np.float32).astype(np.float64)
        x = (r[:, 0] * wl - 0.5).astype(np.float32)          # the product is exact in float64: one rounding, as the fma
        y = (r[:, 1] * hl - 0.5).astype(np.float32)
        return l0, l1, np.floor(x), np.floor(y), wl, hl


class Textures:
    """A material's seven slots: an (h, w, 4) uint8 image, a 4-tuple of codes (a constant slot), or None (the engine's default texel is
    not needed here: a constant of zeros).  Slot 0 is sRGB, the others UNORM, as BaseScene.frag samples them."""

    def __init__(self, slots):
        assert len(slots) == 7
        self.slots = [np.ascontiguousarray(s, dtype=np.uint8) if s is not None else np.zeros(4, np.uint8) for s in slots]

    def is_image(self, s):
        return self.slots[s].ndim == 3

    def oracle(self, pyoracle):
        """an oracle context holding the slots; every image stays an image (as_image), every constant is a 1 x 1 image that collapses.
        Leaves the chains (the oracle's), the decode table and the decoded constants for the probe."""
        o = pyoracle.Oracle(8, 8, 8)
        L = o.L
        self.lut = np.array([L.zo_kat_srgb8_to_linear(c) for c in range(256)], dtype=np.float32)
        self.chains, self.constants = [None] * 7, np.zeros((7, 4), dtype=np.float32)
        for s, im in enumerate(self.slots):
            if self.is_image(s):
                h, w = im.shape[:2]
                assert L.zo_kat_set_image(o.h, s, im.ctypes.data, w, h, int(s == 0), 1) == levels_of(w, h)
                mips = o.tex_mips(im, s == 0)
                assert len(mips) == levels_of(w, h) and all(m.shape[:2] == level_size(w, h, l)[::-1] for l, m in enumerate(mips))
                self.chains[s] = np.concatenate([m.ravel() for m in mips])
            else:
                assert L.zo_kat_set_image(o.h, s, im.ctypes.data, 1, 1, int(s == 0), 0) == 1
                zero = np.zeros((1, 6), dtype=U)
                self.constants[s] = u2f(self.oracle_image(o, s, zero, srgb=(s == 0)))[0]
        return o

    def oracle_image(self, o, slot, table, srgb):
        table = np.ascontiguousarray(table, dtype=U)
        out = np.zeros((len(table), 4), dtype=U)
        o.L.zo_kat_tex_image_batch(o.h, slot, int(srgb), table.ctypes.data, out.ctypes.data, len(table))
        return out

    def oracle_material(self, o, table):
        table = np.ascontiguousarray(table, dtype=U)
        out = np.zeros((len(table), 28), dtype=U)
        o.L.zo_kat_tex_material_batch(o.h, table.ctypes.data, out.ctypes.data, len(table))
        return out


def single_image(w, h, srgb, seed=0):
    """a Textures whose only image sits in slot 0 (sampled as sRGB) or slot 1 (UNORM); returns it and the slot"""
    slot = 0 if srgb else 1
    s = [None] * 7
    s[slot] = noise_image(w, h, seed)
    return Textures(s), slot


# The material sets.  Slots equal in w and h but not in levels cannot exist: the level count is a function of the size
# (floor(log2(max(w, h))) + 1, on the product's host as in the oracle), so that row of the grouping test has no case.
def material_one_size(w, h):
    return Textures([noise_image(w, h, seed=s) for s in range(7)])


def material_three_sizes():
    """64 x 64, 33 x 7 and 16 x 1 across the slots, constant slots between them: three grouping turns"""
    return Textures([noise_image(64, 64, 0), (10, 200, 30, 255), noise_image(33, 7, 2), noise_image(64, 64, 3), (255, 0, 128, 7), noise_image(16, 1, 5),
                     noise_image(33, 7, 6)])


def material_lead_not_zero():
    """slot 0 constant: the first group is led by slot 1; two sizes, two turns"""
    return Textures([(180, 90, 45, 255), noise_image(48, 20, 1), noise_image(48, 20, 2), (128, 128, 255, 255), noise_image(2, 2, 4), None, noise_image(2, 2, 6)])


def material_cases(tex, cap=60000):
    """the cases of a material: the tables of its distinct image sizes, thinned to `cap` rows in all"""
    sizes = sorted({tex.slots[s].shape[1::-1] for s in range(7) if tex.is_image(s)})
    parts = []
    for w, h in sizes:
        t = tex_cases(w, h)
        k = max(1, -(-len(t) * len(sizes) // cap))
        parts.append(t[::k])
    return np.concatenate(parts)


# ------------------------------------------------------------------------------------------------------------------ the surface stage (zr_surface.h)

def compute_normal():
    """pos_dx, pos_dy, s1, t1, s2, t2, fragN, ts.  The determinant s1 t2 - s2 t1 exactly 0 by constant UVs, by collinear UVs (0.25, 0.5) /
    (0.5, 1) and, with it non-zero, a zero position derivative; denormal; of either sign; T parallel to N; fragN zero, denormal, infinite,
    NaN; ts = (0, 0, 1), the default normal map's; 2 000 ordinary fragments (derivatives of a hundredth, a unit normal, a tangent-space
    normal in the upper hemisphere); then generic vectors."""
    uvs = [(0, 0, 0, 0), (0.25, 0.5, 0.5, 1.0), (-0.25, 0.5, 0.5, -1.0), (0.01, 0.0, 0.0, 0.01), (0.0, 0.01, 0.01, 0.0), (0.013, -0.004, 0.002, 0.009),
           (1e-20, 0, 0, 1e-20), (1e-20, 0, 0, -1e-20), (1e-23, 0, 0, 1e-23), (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0), (3e38, 0, 0, 3e38)]
    pds = [((0.01, 0.0, 0.002), (0.0, 0.01, 0.001)), ((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (0.0, 0.01, 0.001)), ((0.5, 0.25, -0.125), (0.0, 0.0, 0.0)),
           ((1e-30, 0, 0), (0, 1e-30, 0))]
    ns = [(0, 0, 1), (0.3, -0.5, 0.8), (0.5, 0.25, -0.125), (0.01, 0.0, 0.002), (0, 0, 0), (1e-40, 0, 0), (1e-30, 1e-30, 0), (np.inf, 0, 0),
          (np.nan, 0, 1), (0, 0, -3e38)]
    tss = [(0, 0, 1), (0.3, -0.2, 0.93), (-0.0, 0.0, 1.0), (1, 0, 0)]
    rows = [pdx + pdy + uv + n + ts for uv in uvs for pdx, pdy in pds for n in ns for ts in tss]
    rng = np.random.default_rng(20276)
    n = 2000
    nrm = rng.normal(size=(n, 3))
    tsn = rng.normal(size=(n, 3)) * (0.4, 0.4, 1.0)
    tsn[:, 2] = np.abs(tsn[:, 2]) + 0.2
    plain = np.concatenate([rng.uniform(-0.02, 0.02, (n, 6)), rng.uniform(-0.02, 0.02, (n, 4)), nrm / np.linalg.norm(nrm, axis=1, keepdims=True),
                            tsn / np.linalg.norm(tsn, axis=1, keepdims=True)], axis=1).astype(np.float32)
    return np.concatenate([f2u(np.array(rows, dtype=np.float32)).reshape(-1, 16), f2u(plain).reshape(-1, 16), vectors(16)])


PROJECT_TARGETS = ((640.0, 360.0), (0.5, 0.5), (2048.0, 2048.0), (127.5, 72.5))        # project()'s (hw, hh) blocks, in its order
MAX_PIXEL = 16383
PROJECT_SATURATED = 1 << 30       # |X| or |Y| from here on: project() has clamped an infinite coordinate


def bary_screen(L):
    """X0, Y0, a1, b1, a2, b2, rw0, rw1, rw2, px, py.  The set-ups are pixel_geom's, formed (here, in float32, from integer differences that
    float32 holds exactly) from triples of project()'s results over its own table - a fast-path triangle holds only such corners; pixels
    around the first corner and at 0 and 16383, each with its quad partners px ^ 1 and py ^ 1; then rw sums that are 0, denormal, huge.
    Corners whose project() saturates are left out: a denormal w makes rw infinite and snaps X, Y to INT_MIN (320 of the table's 5 984
    rows, all with w = 2^-149), and px * 256 + 128 - X0 then leaves int in the product's bary_screen as in the oracle's - signed overflow,
    undefined on both sides, so there is nothing to compare.  The coverage test asserts the bound on what remains."""
    rng = np.random.default_rng(20273)
    sv = oracle_batch(L, "project", project())
    per = len(sv) // len(PROJECT_TARGETS)
    rows = []
    for b in range(len(PROJECT_TARGETS)):
        blk = sv[b * per:(b + 1) * per]
        X, Y, rw = blk[:, 0].astype(np.int32).astype(np.int64), blk[:, 1].astype(np.int32).astype(np.int64), u2f(blk[:, 3])
        keep = (np.abs(X) < PROJECT_SATURATED) & (np.abs(Y) < PROJECT_SATURATED)
        X, Y, rw, n = X[keep], Y[keep], rw[keep], int(keep.sum())
        i = rng.integers(0, n, (1500, 3))
        x, y = X[i], Y[i]
        A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        with np.errstate(all="ignore"):
            invA = np.float32(1.0) / A.astype(np.float32)
            a1, b1 = (y[:, 2] - y[:, 0]).astype(np.float32) * invA, (x[:, 0] - x[:, 2]).astype(np.float32) * invA
            a2, b2 = (y[:, 0] - y[:, 1]).astype(np.float32) * invA, (x[:, 1] - x[:, 0]).astype(np.float32) * invA
        r = rw[i].copy()
        kind = np.arange(len(i)) % 12
        for k, v in ((8, (0.0, 0.0, 0.0)), (9, (1e-40, 1e-41, 0.0)), (10, (3e38, 3e38, 3e38)), (11, (1.0, -1.0, 0.0))):
            r[kind == k] = np.array(v, dtype=np.float32)
        px = np.clip((x[:, 0] >> 8) + rng.integers(-3, 4, len(i)), 0, MAX_PIXEL)
        py = np.clip((y[:, 0] >> 8) + rng.integers(-3, 4, len(i)), 0, MAX_PIXEL)
        px[kind == 1], py[kind == 1] = 0, 0
        px[kind == 2], py[kind == 2] = MAX_PIXEL, MAX_PIXEL
        head = np.column_stack([x[:, 0].astype(np.int32).view(U), y[:, 0].astype(np.int32).view(U), f2u(a1), f2u(b1), f2u(a2), f2u(b2), f2u(r).reshape(-1, 3)])
        for qx, qy in ((px, py), (px ^ 1, py), (px, py ^ 1)):
            rows.append(np.column_stack([head, qx.astype(U), qy.astype(U)]))
    return np.concatenate(rows).astype(U)


def bary_homog():
    """three clip-space corners from clip_vertices() (w <= 0 on one and on two of them among the triples), hw, hh, px, py with the quad
    partners; three equal corners (every k is 0: the denominator is 0)"""
    rng = np.random.default_rng(20274)
    v = clip_vertices()
    rows = []
    for hw, hh in PROJECT_TARGETS:
        i = rng.integers(0, len(v), (1500, 3))
        i[::50, 1] = i[::50, 0]
        i[::50, 2] = i[::50, 0]
        tri = np.concatenate([v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]], axis=1)
        px = rng.integers(0, max(1, int(2 * hw)), len(i))
        py = rng.integers(0, max(1, int(2 * hh)), len(i))
        px[1::50], py[1::50] = MAX_PIXEL, MAX_PIXEL
        t = np.tile(f2u(np.array([hw, hh], dtype=np.float32)), (len(i), 1))
        for qx, qy in ((px, py), (px ^ 1, py), (px, py ^ 1)):
            rows.append(np.column_stack([tri, t, qx.astype(U), qy.astype(U)]))
    return np.concatenate(rows).astype(U)


def stage_roll(angle=0.37):
    """glm::rotate(mat4(1), angle, z) with a translation, column-major"""
    c, s = np.float32(np.cos(angle)), np.float32(np.sin(angle))
    return np.array([c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, 0.5, -2.0, 0.25, 1], dtype=np.float32)


def model_point():
    """M, p, m_identity.  The flag is what the host sets when M is bit for bit the identity, and the short cut p + 0 is M * vec4(p, 1)
    for a p whose components are all finite or all NaN: flag 1 rows hold exactly that.  Through the matrix an infinite component gives
    inf * 0 = NaN, and one NaN component makes all three NaN, where the short cut keeps the others; neither reaches it.  Its callers pass
    the position of a corner of a triangle that won a pixel (classify() lets only finite clip coordinates through, so the position is
    finite) and normalize(normal) - finite, all NaN, or NaN with zeros from an infinite component, whose only reader, compute_normal,
    normalises first and so sees NaN either way.  Flag 0: the identity over every p, a stage roll, an identity whose
    translation is -0 (not the identity bit for bit), generic matrices."""
    g = generic()
    fin = g[np.isfinite(u2f(g))]
    nan = g[np.isnan(u2f(g))]
    rng = np.random.default_rng(20275)

    def rows(M, p, flag):
        return np.concatenate([np.tile(f2u(M), (len(p), 1)), p, np.full((len(p), 1), flag, dtype=U)], axis=1)
    p1 = np.concatenate([np.stack([fin, rng.permutation(fin), rng.permutation(fin)], axis=1), np.stack([nan, rng.permutation(nan), rng.permutation(nan)], axis=1)])
    p0 = np.stack([g, rng.permutation(g), rng.permutation(g)], axis=1)
    neg0 = IDENTITY.copy()
    neg0[12:15] = -0.0
    v = vectors(19)
    return np.concatenate([rows(IDENTITY, p1, 1), rows(IDENTITY, p0, 0), rows(stage_roll(), p0[::4], 0), rows(neg0, p0[::4], 0),
                           np.concatenate([v, np.zeros((len(v), 1), dtype=U)], axis=1)]).astype(U)


# ---- a constant image that is still an image (oracle/CONTRACT.md, "a constant image")
CONSTANT_CODES = (1, 37, 90, 143, 201, 254)
CONSTANT_SIDE = 4


def constant_image_cases():
    """u, v inside the image and NaN, under the exact-breakpoint footprints of every N in 1..16 (x the major axis)"""
    bp = footprint_breakpoints(CONSTANT_SIDE, CONSTANT_SIDE)
    f = f2u(bp[(bp[:, 5] == 0) & (bp[:, 6] == 0), :4].astype(np.float32)).reshape(-1, 4)
    uv = np.array([[0x3E99999A, 0x3F333333], [NAN_Q, 0x3F333333], [0x3E99999A, INF]], dtype=U)          # (0.3, 0.7), a NaN u, an infinite v
    return np.concatenate([np.concatenate([np.tile(c, (len(f), 1)), f], axis=1) for c in uv]).astype(U)


def constant_image(code, pyoracle, table):
    """a Textures whose slot 0 is a 4 x 4 image of (code, 255 - code, code / 2, 255) throughout; the oracle's samples of `table` with the
    slot kept an image (filtered) and collapsed to its texel"""
    im = np.empty((CONSTANT_SIDE, CONSTANT_SIDE, 4), np.uint8)
    im[:] = (code, 255 - code, code // 2, 255)
    tex = Textures([im] + [None] * 6)
    o = tex.oracle(pyoracle)
    filtered = tex.oracle_image(o, 0, table, True)
    assert o.L.zo_kat_set_image(o.h, 0, im.ctypes.data, CONSTANT_SIDE, CONSTANT_SIDE, 1, 0) == levels_of(CONSTANT_SIDE, CONSTANT_SIDE)
    collapsed = tex.oracle_image(o, 0, table, True)
    o.close()
    return tex, filtered, collapsed
