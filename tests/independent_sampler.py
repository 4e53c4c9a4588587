"""An independent float64 restatement of the texture sampling rules the oracle follows (test infrastructure; numpy only).

Written from the Vulkan specification's wording, not from oracle/zo_oracle.c, and organised differently (whole-array numpy for the
mip chains, scalar float64 for one sample, and whole-array forms of the same rules for a frame's pixels), so that an error in the
oracle's float32 code is not repeated here:

* "Image Sample Operations" chapter of the specification:
  - sRGB decode / encode                         ("sRGB EOTF" of the Khronos Data Format specification)
  - unnormalised coordinates u = s * width, linear filtering takes texels i0 = floor(u - 1/2), i1 = i0 + 1 with weight
    frac(u - 1/2); REPEAT wraps i mod size; CLAMP_TO_EDGE clamps i to [0, size - 1]
  - mip level selection: lambda from the footprint, d_lo = floor(lambda), d_hi = d_lo + 1, weight frac(lambda)
  - "Texel Anisotropic Filtering": N = min(ceil(Pmax / Pmin), maxAniso), lambda = log2(Pmax / N), N samples spread along the
    major axis at (i / (N + 1) - 1/2), averaged
  - cube map face selection table (major axis, sc, tc, ma; ties: z over y over x), s = 1/2 (sc / |ma|) + 1/2
* vkCmdBlitImage with VK_FILTER_LINEAR (RHIGenerateMipmaps, ZE:6348-6433): destination texel centre (x + 1/2) maps to
  u = (x + 1/2) * srcW / dstW in the source level, which is then filtered linearly with CLAMP_TO_EDGE.

Choices the specification leaves open and the oracle fixes (oracle/zo_oracle.c header): maxAnisotropy 16; cube faces are filtered
with CLAMP_TO_EDGE inside the selected face (no seam filtering); cubemap levels halve by a 2x2 box, which is what the LINEAR blit of
an even-sized level is.
"""
import math

import numpy as np

F = np.float64
MAX_ANISO = 16


def srgb_decode(c8):
    c = np.asarray(c8, F) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def srgb_encode_real(l):
    """linear [0, 1] -> the real-valued 8-bit code before rounding"""
    l = np.clip(np.asarray(l, F), 0.0, 1.0)
    return 255.0 * np.where(l <= 0.0031308, 12.92 * l, 1.055 * l ** (1.0 / 2.4) - 0.055)


def decode(img8, srgb):
    """(h, w, 4) uint8 -> float64 RGBA as the sampler sees it (alpha is never sRGB)"""
    out = np.asarray(img8, F) / 255.0
    if srgb:
        out[..., :3] = srgb_decode(np.asarray(img8)[..., :3])
    return out


def blit_half_real(level8, srgb):
    """One vkCmdBlitImage(LINEAR) step to the next mip: returns the REAL-valued 8-bit codes (h', w', 4) before rounding."""
    src = decode(level8, srgb)
    sh, sw = src.shape[:2]
    dh, dw = max(1, sh // 2), max(1, sw // 2)

    def taps(dn, sn):
        u = (np.arange(dn, dtype=F) + 0.5) * (sn / dn) - 0.5
        i0 = np.floor(u)
        w = u - i0
        return np.clip(i0, 0, sn - 1).astype(int), np.clip(i0 + 1, 0, sn - 1).astype(int), w
    x0, x1, wx = taps(dw, sw)
    y0, y1, wy = taps(dh, sh)
    rows0 = src[y0][:, x0] * (1 - wx)[None, :, None] + src[y0][:, x1] * wx[None, :, None]
    rows1 = src[y1][:, x0] * (1 - wx)[None, :, None] + src[y1][:, x1] * wx[None, :, None]
    lin = rows0 * (1 - wy)[:, None, None] + rows1 * wy[:, None, None]
    out = lin * 255.0
    if srgb:
        out[..., :3] = srgb_encode_real(lin[..., :3])
    return out


def wrap_repeat(i, n):
    return int(i) % n


def bilinear_repeat(level, u, v):
    """level: decoded float64 (h, w, 4); normalised (u, v); REPEAT addressing"""
    h, w = level.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    i0, j0 = math.floor(x), math.floor(y)
    a, b = x - i0, y - j0
    t = lambda i, j: level[wrap_repeat(j, h), wrap_repeat(i, w)]
    return (t(i0, j0) * (1 - a) + t(i0 + 1, j0) * a) * (1 - b) + (t(i0, j0 + 1) * (1 - a) + t(i0 + 1, j0 + 1) * a) * b


def trilinear(levels, lam, u, v):
    d = int(math.floor(lam))
    hi = min(d + 1, len(levels) - 1)
    f = lam - d
    return bilinear_repeat(levels[d], u, v) * (1 - f) + bilinear_repeat(levels[hi], u, v) * f


def aniso_parameters(w, h, duv, n_levels):
    """-> N, lambda, major axis derivative (du, dv), margin: the distance of Pmax / Pmin from the nearest integer below 16 (a sample
    whose ratio sits on such a boundary may legitimately take N or N + 1 taps in float32)"""
    dudx, dvdx, dudy, dvdy = [float(x) for x in duv]
    px, py = math.hypot(dudx * w, dvdx * h), math.hypot(dudy * w, dvdy * h)
    pmax, pmin = max(px, py), min(px, py)
    if pmax == 0.0:
        return 1, 0.0, (0.0, 0.0), 1.0
    ratio = pmax / pmin if pmin > 0 else math.inf
    n = MAX_ANISO if ratio >= MAX_ANISO else max(1, math.ceil(ratio))
    margin = 1.0 if (ratio >= MAX_ANISO + 0.5 or ratio == 1.0) else abs(ratio - round(ratio))
    lam = math.log2(pmax / n)
    lam = min(max(lam, 0.0), n_levels - 1.0)
    major = (dudx, dvdx) if px >= py else (dudy, dvdy)
    return n, lam, major, margin


def sample_2d(levels8, srgb, uv, duv):
    """texture(sampler2D, uv) with explicit derivatives; levels8: the mip chain as uint8 arrays"""
    levels = [decode(l, srgb) for l in levels8]
    h, w = levels[0].shape[:2]
    n, lam, (du, dv), margin = aniso_parameters(w, h, duv, len(levels))
    acc = np.zeros(4, F)
    for i in range(1, n + 1):
        off = i / (n + 1) - 0.5
        acc += trilinear(levels, lam, uv[0] + du * off, uv[1] + dv * off)
    return acc / n, n, lam, margin


# Cube Map Face Selection (the specification's table): face index, sc, tc, ma
def cube_face(r):
    rx, ry, rz = [float(x) for x in r]
    ax, ay, az = abs(rx), abs(ry), abs(rz)
    if az >= ax and az >= ay:
        return (4, rx, -ry, az) if rz >= 0 else (5, -rx, -ry, az)
    if ay >= ax:
        return (2, rx, rz, ay) if ry >= 0 else (3, rx, -rz, ay)
    return (0, -rz, -ry, ax) if rx >= 0 else (1, rz, -ry, ax)


def bilinear_clamp(face, s, t):
    d = face.shape[0]
    x, y = s * d - 0.5, t * d - 0.5
    i0, j0 = math.floor(x), math.floor(y)
    a, b = x - i0, y - j0
    cl = lambda i: min(max(i, 0), d - 1)
    g = lambda i, j: face[cl(j), cl(i)]
    return (g(i0, j0) * (1 - a) + g(i0 + 1, j0) * a) * (1 - b) + (g(i0, j0 + 1) * (1 - a) + g(i0 + 1, j0 + 1) * a) * b


def sample_cube(levels8, r, lod):
    """textureLod(samplerCube, r, lod).rgb; levels8[l]: (6, d, d, 4) uint8, sRGB"""
    f, sc, tc, ma = cube_face(r)
    s, t = 0.5 * sc / ma + 0.5, 0.5 * tc / ma + 0.5
    lam = min(max(float(lod), 0.0), len(levels8) - 1.0)
    d = int(math.floor(lam))
    hi = min(d + 1, len(levels8) - 1)
    w = lam - d
    lo_c = bilinear_clamp(srgb_decode(levels8[d][f][..., :3]), s, t)
    hi_c = bilinear_clamp(srgb_decode(levels8[hi][f][..., :3]), s, t)
    return lo_c * (1 - w) + hi_c * w


def cube_half_real(level8):
    """next cubemap level as real-valued codes: 2x2 box in linear light (colour), plain mean (alpha)"""
    lin = srgb_decode(level8[..., :3])
    d = level8.shape[1]
    nd = max(1, d // 2)
    ix = np.minimum(np.arange(nd) * 2 + 1, d - 1)
    i0 = np.arange(nd) * 2
    box = lambda a: (a[:, i0][:, :, i0] + a[:, i0][:, :, ix] + a[:, ix][:, :, i0] + a[:, ix][:, :, ix]) / 4.0
    return srgb_encode_real(box(lin)), box(np.asarray(level8[..., 3], F))


# ---------------------------------------------------------------------------------------------------------------- whole-array forms
# The same rules over arrays of samples (a frame's pixels), for the frame statements of tests/independent_eval.py.  Written again
# rather than looped over the scalar forms above, which tests/test_oracle_textured.py holds them to.  `control` names a misreading
# the engine's text rules out (the negative controls of that module): "no_aniso" (N = 1), "clamp" (CLAMP_TO_EDGE instead of REPEAT),
# "y_faces_tc_flipped" (the +-Y rows of the face table with tc negated); "srgb_space_blit" is mip_chain()'s.

def mip_chain(img8, srgb, control=None):
    """RHIGenerateMipmaps' chain of an (h, w, 4) uint8 image: floor(log2(max(w, h))) + 1 levels, each the rounding of blit_half_real
    of the level before (round to nearest; a real value within float noise of a half rounds up)"""
    img8 = np.asarray(img8, np.uint8)
    h, w = img8.shape[:2]
    n = int(math.floor(math.log2(max(w, h)))) + 1
    chain = [img8]
    for _ in range(1, n):
        real = blit_half_real(chain[-1], srgb and control != "srgb_space_blit")
        chain.append(np.clip(np.floor(real + 0.5 + 1e-7), 0, 255).astype(np.uint8))
    return chain


def cube_chain(faces8):
    """the cubemap's chain from six (d, d, 4) uint8 faces: floor(log2(d)) + 1 levels of (6, d', d', 4), each the rounding of cube_half_real"""
    lvl = np.stack([np.asarray(f, np.uint8) for f in faces8])
    chain = [lvl]
    for _ in range(1, int(math.floor(math.log2(lvl.shape[1]))) + 1):
        rgb, alpha = cube_half_real(chain[-1])
        chain.append(np.clip(np.floor(np.concatenate([rgb, alpha[..., None]], axis=-1) + 0.5 + 1e-7), 0, 255).astype(np.uint8))
    return chain


def aniso_parameters_array(w, h, duv, n_levels, control=None):
    """aniso_parameters() over (n, 4) derivatives (dudx, dvdx, dudy, dvdy) -> N, lambda, major (n, 2), margin, Pmax / Pmin"""
    duv = np.asarray(duv, F)
    px, py = np.hypot(duv[:, 0] * w, duv[:, 1] * h), np.hypot(duv[:, 2] * w, duv[:, 3] * h)
    pmax, pmin = np.maximum(px, py), np.minimum(px, py)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(pmin > 0, pmax / np.where(pmin > 0, pmin, 1.0), np.inf)
        n = np.where(ratio >= MAX_ANISO, MAX_ANISO, np.maximum(1, np.ceil(np.minimum(ratio, MAX_ANISO)))).astype(np.int64)
        if control == "no_aniso":
            n = np.ones_like(n)
        margin = np.where((ratio >= MAX_ANISO + 0.5) | (ratio == 1.0), 1.0, np.abs(ratio - np.round(np.minimum(ratio, 1e9))))
        lam = np.clip(np.log2(pmax / n), 0.0, n_levels - 1.0)
    zero = pmax == 0.0
    n[zero], lam[zero], margin[zero] = 1, 0.0, 1.0
    major = np.where((px >= py)[:, None], duv[:, 0:2], duv[:, 2:4])
    major[zero] = 0.0
    return n, lam, major, margin, ratio


def _bilinear_array(level, u, v, control=None):
    h, w = level.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    i0, j0 = np.floor(x), np.floor(y)
    a, b = (x - i0)[:, None], (y - j0)[:, None]
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    if control == "clamp":
        wi, wj = lambda i: np.clip(i, 0, w - 1), lambda j: np.clip(j, 0, h - 1)
    else:
        wi, wj = lambda i: np.mod(i, w), lambda j: np.mod(j, h)
    t = lambda i, j: level[wj(j), wi(i)]
    return (t(i0, j0) * (1 - a) + t(i0 + 1, j0) * a) * (1 - b) + (t(i0, j0 + 1) * (1 - a) + t(i0 + 1, j0 + 1) * a) * b


def _trilinear_array(levels, lam, u, v, control=None):
    d = np.floor(lam).astype(np.int64)
    hi = np.minimum(d + 1, len(levels) - 1)
    f = lam - d
    out = np.zeros((len(lam), 4))
    for l in range(len(levels)):
        wgt = np.where(d == l, 1.0 - f, 0.0) + np.where(hi == l, f, 0.0)
        k = np.nonzero(wgt != 0.0)[0]
        if len(k):
            out[k] += _bilinear_array(levels[l], u[k], v[k], control) * wgt[k, None]
    return out


def sample_2d_array(levels8, srgb, uv, duv, control=None, decoded=None):
    """sample_2d() over (n, 2) coordinates and (n, 4) derivatives -> (n, 4) values, N, lambda, margin, Pmax / Pmin.
    decoded: the chain already through decode() (callers that sample one chain many times)"""
    levels = decoded if decoded is not None else [decode(l, srgb) for l in levels8]
    h, w = levels[0].shape[:2]
    uv = np.asarray(uv, F)
    n, lam, major, margin, ratio = aniso_parameters_array(w, h, duv, len(levels), control)
    acc = np.zeros((len(uv), 4))
    for i in range(1, MAX_ANISO + 1):
        k = np.nonzero(n >= i)[0]
        if not len(k):
            break
        off = i / (n[k] + 1.0) - 0.5
        acc[k] += _trilinear_array(levels, lam[k], uv[k, 0] + major[k, 0] * off, uv[k, 1] + major[k, 1] * off, control)
    return acc / n[:, None], n, lam, margin, ratio


def cube_face_array(r, control=None):
    """cube_face() over (n, 3) directions -> face, sc, tc, ma"""
    r = np.asarray(r, F)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    ax, ay, az = np.abs(rx), np.abs(ry), np.abs(rz)
    zm, ym = (az >= ax) & (az >= ay), ay >= ax
    yflip = -1.0 if control == "y_faces_tc_flipped" else 1.0
    face = np.where(zm, np.where(rz >= 0, 4, 5), np.where(ym, np.where(ry >= 0, 2, 3), np.where(rx >= 0, 0, 1)))
    sc = np.select([face == 4, face == 5, face == 2, face == 3, face == 0], [rx, -rx, rx, rx, -rz], rz)
    tc = np.select([face == 4, face == 5, face == 2, face == 3, face == 0], [-ry, -ry, yflip * rz, -yflip * rz, -ry], -ry)
    ma = np.select([zm, ym], [az, ay], ax)
    return face, sc, tc, ma


def _bilinear_clamp_array(faces, f, s, t):
    d = faces.shape[1]
    x, y = s * d - 0.5, t * d - 0.5
    i0, j0 = np.floor(x), np.floor(y)
    a, b = (x - i0)[:, None], (y - j0)[:, None]
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    g = lambda i, j: faces[f, np.clip(j, 0, d - 1), np.clip(i, 0, d - 1)]
    return (g(i0, j0) * (1 - a) + g(i0 + 1, j0) * a) * (1 - b) + (g(i0, j0 + 1) * (1 - a) + g(i0 + 1, j0 + 1) * a) * b


def sample_cube_array(levels8, r, lod, control=None, decoded=None):
    """sample_cube() over (n, 3) directions and (n,) lods -> (n, 3); decoded: [srgb_decode(level[..., :3]) for level in levels8]"""
    levels = decoded if decoded is not None else [srgb_decode(l[..., :3]) for l in levels8]
    f, sc, tc, ma = cube_face_array(r, control)
    with np.errstate(divide="ignore", invalid="ignore"):
        s, t = 0.5 * sc / ma + 0.5, 0.5 * tc / ma + 0.5
    ok = np.isfinite(s) & np.isfinite(t)
    s, t = np.where(ok, s, 0.5), np.where(ok, t, 0.5)
    lam = np.clip(np.nan_to_num(np.asarray(lod, F), nan=0.0), 0.0, len(levels) - 1.0) * np.ones(len(f))
    d = np.floor(lam).astype(np.int64)
    hi = np.minimum(d + 1, len(levels) - 1)
    w = lam - d
    out = np.zeros((len(f), 3))
    for l in range(len(levels)):
        wgt = np.where(d == l, 1.0 - w, 0.0) + np.where(hi == l, w, 0.0)
        k = np.nonzero(wgt != 0.0)[0]
        if len(k):
            out[k] += _bilinear_clamp_array(levels[l], f[k], s[k], t[k]) * wgt[k, None]
    return out
