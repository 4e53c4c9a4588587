"""A second, independent evaluation of the engine's shaders — float64 numpy, libm transcendentals, the GLSL's own evaluation order.

TEST INFRASTRUCTURE.  Written from the reference's GLSL text alone (SH = Engine/ZeldaEngine/Shaders): SH/Base.vert:23-32,
SH/BaseInstanced.vert:38-76, SH/BaseScene.frag:26-48, SH/BaseLighting.frag:147-254 and the functions of SH/Common.glsl they call
— NOT from oracle/zo_oracle.c or the HIP kernels under csrc/, whose author might have misread a shader line identically in both.  It
shares no code with them: different language, different precision (float64), different transcendentals (libm), naive evaluation
order, exact sRGB / UNORM / fp16 conversions by definition instead of by table.

What it takes as GIVEN: which primitive owns each pixel and, for the lighting pass, the GBuffer, the shadow map and the frame's
matrices.  These are no longer unchecked: tests/independent_geometry.py states the uniforms (UpdateUniformBuffer), the camera pass's
winner and depth and the shadow map in float64 from the host code and the Vulkan text, and tests/test_oracle_geometry.py /
tests/test_gpu_independent.py hold the oracle and the HIP renderer to it outside a derived ambiguity mask; the GPU test also feeds that
statement's winners to base_scene() below, so the chain runs without the oracle.  Still unpinned: the 1/256-pixel snap, the clipper's
re-snapped intersections and the depth-bias r of a clipped primitive (the implementation's choices).  What it recomputes: the vertex
stage, perspective-correct interpolation, the 2x2-quad derivatives, ComputeNormal, every output of BaseScene.frag with its format
conversion, and the whole lighting shader per pixel.  Material slots are either constant texels or images sampled through
tests/independent_sampler.py (its own mip chains, the quad's derivatives, REPEAT, the specification's anisotropic scheme), and the
reflection cubemap either one colour per face or a chain sampled at ComputeReflectionMipFromRoughness; for sampled slots base_scene()
also states the range the value spans over the snap and float32 error budget and which pixels' tap count is not decided
(tests/test_oracle_textured.py).  Still unpinned on the texture side: cube seam filtering (CLAMP_TO_EDGE inside a face, a stated
choice).  The skydome and background passes are tests/independent_sky.py's; the debug views are lighting()'s switch and gbuffer_vis().
"""
import numpy as np

import independent_sampler as isamp

F64 = np.float64


def mat(m16):
    """column-major float[16] (GLSL / glm layout) -> 4x4 matrix in the usual row, column indexing"""
    return np.asarray(m16, dtype=F64).reshape(4, 4).T


def normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def dot(a, b):
    return np.sum(a * b, axis=-1)


def saturate(x):
    return np.clip(x, 0.0, 1.0)


def srgb_to_linear(c8):
    """VK_FORMAT_R8G8B8A8_SRGB decode of an 8-bit channel (the sRGB EOTF)"""
    x = np.asarray(c8, dtype=F64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


# ----------------------------------------------------------------------------------------------- vertex stage

def make_rot_matrix(R):
    """MakeRotMatrix, SH/Common.glsl:60-87 / SH/BaseInstanced.vert:38-64.  GLSL `m[i] = vec4(...)` sets COLUMN i."""
    def cols(c0, c1, c2):
        return np.array([c0, c1, c2], dtype=F64).T          # columns -> matrix
    s, c = np.sin(R[0]), np.cos(R[0])
    mx = cols((c, 0.0, s), (0.0, 1.0, 0.0), (-s, 0.0, c))
    s, c = np.sin(R[1]), np.cos(R[1])
    my = cols((c, s, 0.0), (-s, c, 0.0), (0.0, 0.0, 1.0))
    s, c = np.sin(R[2]), np.cos(R[2])
    mz = cols((1.0, 0.0, 0.0), (0.0, c, s), (0.0, -s, c))
    return mz @ my @ mx                                      # mat3(rotMat)


def vertex_stage(verts, inst, model, view, proj):
    """Base.vert:23-32 (inst is None) / BaseInstanced.vert:66-76 for one draw instance -> (clip (n,4), world pos (n,3), normal (n,3), uv (n,2))"""
    pos = np.asarray(verts["Position"], dtype=F64)
    nrm = normalize(np.asarray(verts["Normal"], dtype=F64))
    ones = np.ones((len(pos), 1))
    if inst is not None:
        rot = make_rot_matrix(np.asarray(inst["InstanceRotation"], dtype=F64))
        pos = (pos * F64(inst["InstancePScale"])) @ rot + np.asarray(inst["InstancePosition"], dtype=F64)      # row vector * mat3
    wpos = (np.hstack([pos, ones]) @ model.T)
    clip = wpos @ view.T @ proj.T
    wn = (np.hstack([nrm, ones]) @ model.T)[:, :3]           # vec4(normalize(inNormal), 1.0): the w = 1 is the shader's own
    if inst is not None:
        wn = wn @ rot
    return clip, wpos[:, :3], wn, np.asarray(verts["TexCoord"], dtype=F64)


# ----------------------------------------------------------------------------------------------- BaseScene.frag

def compute_normal(pos_dx, pos_dy, st1, st2, frag_normal, tex_normal):
    """ComputeNormal(fragPosition, fragTexCoord, fragNormal, texNormal), SH/Common.glsl:113-127"""
    with np.errstate(invalid="ignore", divide="ignore"):
        T = (st2[..., 1:2] * pos_dx - st1[..., 1:2] * pos_dy) / (st1[..., 0:1] * st2[..., 1:2] - st2[..., 0:1] * st1[..., 1:2])
    N = normalize(frag_normal)
    T = normalize(T - N * dot(N, T)[..., None])
    B = normalize(np.cross(N, T))
    n = normalize(tex_normal)
    ts = normalize(2.0 * n - 1.0)
    return normalize(T * ts[..., 0:1] + B * ts[..., 1:2] + N * ts[..., 2:3])        # TBN * v, TBN = mat3(T, B, N) (columns)


# The sampled slots' error budget.  An implementation's fragment sees UV0 and the quad differences st1 / st2 after
# two steps this statement does not take: the 1/256-pixel vertex snap and float32 interpolation.
F32_INTERP = 8 * 2.0 ** -24      # |uv| relative: three products and two sums (half an ulp each) over barycentrics good to ~4 ulp
SNAP = 1.0 / 256.0               # pixels
GUARD = 4.0                      # the clipper's guard band, in viewports


# the clip volume with the guard band: 0 <= z <= w, |x|, |y| <= GUARD w (the planes a clipper may cut with)
_PLANES = [np.array(p, dtype=F64) for p in ((0, 0, 1, 0), (0, 0, -1, 1), (-1, 0, 0, GUARD), (1, 0, 0, GUARD), (0, -1, 0, GUARD),
                                            (0, 1, 0, GUARD))]


def clipped_altitude(tri, W, H):
    """the smallest altitude (pixels) over every three vertices of the triangle's polygon after clipping (Sutherland-Hodgman)"""
    poly = [p for p in tri]
    for pl in _PLANES:
        out = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            da, db = float(pl @ a), float(pl @ b)
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                out.append(a + (b - a) * (da / (da - db)))
        poly = out
        if len(poly) < 3:
            return 0.0
    sp = np.array([[(p[0] / p[3] + 1.0) * 0.5 * W, (p[1] / p[3] + 1.0) * 0.5 * H] for p in poly])
    best = np.inf
    n = len(sp)
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                e = [sp[j] - sp[i], sp[k] - sp[j], sp[i] - sp[k]]
                area2 = abs(e[0][0] * e[1][1] - e[0][1] * e[1][0])
                best = min(best, area2 / max(np.hypot(*e[m]) for m in range(3)))
    return float(best)


def altitudes(c3, W, H):
    """per triangle: its smallest screen altitude, or for a clipped one the clipped polygon's (see clipped_altitude).
    -> altitudes (T,), clipped (T,): the triangle crosses the near or far plane, w = 0 or the guard band"""
    w = c3[..., 3]
    clipped = np.any((w <= 0.0) | (c3[..., 2] < 0.0) | (c3[..., 2] > w) | (np.abs(c3[..., 0]) > GUARD * w) | (np.abs(c3[..., 1]) > GUARD * w), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sp = (c3[..., :2] / w[..., None] + 1.0) * 0.5 * np.array([W, H])
        e = [sp[:, (j + 1) % 3] - sp[:, j] for j in range(3)]
        area2 = np.abs(e[0][:, 0] * e[1][:, 1] - e[0][:, 1] * e[1][:, 0])
        alt = np.min([area2 / np.hypot(*ej.T) for ej in e], axis=0)
    alt = np.where(np.isfinite(alt), alt, 0.0)
    for k in np.nonzero(clipped)[0]:
        alt[k] = clipped_altitude(c3[k], W, H)
    return alt, clipped


def _sampled_slot(chain, srgb, UV0, st1, st2, tri_uv, alt_px, control):
    """texture(sampler, UV0) with the quad's derivatives, and the range the float64 value spans over the error budget.
    -> value (k, 4), range (k, 4), ambiguous (k,): Pmax / Pmin within the derivative error of an integer below 16 (N or N + 1 taps)"""
    dec = [isamp.decode(l, srgb) for l in chain]
    duv = np.hstack([st1, st2])
    val, _, _, margin, ratio = isamp.sample_2d_array(chain, srgb, UV0, duv, control, dec)
    e_uv = F32_INTERP * np.abs(tri_uv).max(axis=1)                               # (k, 2): interpolation error of u and v
    with np.errstate(divide="ignore", invalid="ignore"):
        # the two derivative vectors: a float32 quad difference (two interpolation errors) relative to the shorter one, plus what
        # moving the triangle's vertices by half a snap step each does to its screen gradient: 2 x (SNAP / 2) over its smallest altitude
        rel = 2.0 * np.hypot(*e_uv.T) / np.minimum(np.hypot(*st1.T), np.hypot(*st2.T)) + SNAP / alt_px
    rel = np.where(np.isfinite(rel), rel, np.inf)
    bad = rel > 0.2
    r = np.where(bad, 0.0, rel)[:, None]
    # uv: the snap budget, the interpolation error, and the tap positions (off * major axis, |off| < 1/2) moved by the derivative error
    d_uv = (np.abs(st1) + np.abs(st2)) * (SNAP + 0.5 * r) + e_uv
    lo, hi = val.copy(), val.copy()
    for su, sv in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        v = isamp.sample_2d_array(chain, srgb, UV0 + d_uv * (su, sv), duv, control, dec)[0]
        lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    for a, b in ((1, -1), (-1, 1), (1, 1), (-1, -1)):                              # Pmax / Pmin and lambda at their extremes
        v = isamp.sample_2d_array(chain, srgb, UV0, np.hstack([st1 * (1 + a * r), st2 * (1 + b * r)]), control, dec)[0]
        lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    # Pmax / Pmin moves by a factor within (1 +- r) / (1 -+ r), i.e. by less than 2.5 r of itself for r <= 0.2
    amb = bad | ((ratio < isamp.MAX_ANISO) & (margin <= 2.5 * rel * ratio))
    return val, hi - lo, amb


def base_scene(draws, cam, prim_ids, W, H, control=None):
    """BaseScene.frag:26-48 for every covered pixel.

    draws: list of dicts in the engine's draw order {verts, idx, instances (or None), texel (7 RGBA8 tuples), prim_base, images (optional:
    7 entries, each None - the slot's constant texel - or an (h, w, 4) uint8 image sampled through its mip chain)}
    cam: XkUniformBufferMVP (numpy record); prim_ids: (H, W) winning primitive per pixel (0xFFFFFFFF: none)
    control: a misreading for the negative controls - "slot0_unorm", or one of independent_sampler's
    -> dict of float arrays over the covered pixels + their (y, x) coordinates; for sampled slots also "range_<target>" (the span of
    the float64 value over the error budget, per channel) and "ambiguous" (per pixel)
    """
    model, view, proj = mat(cam["Model"]), mat(cam["View"]), mat(cam["Proj"])
    ys, xs = np.nonzero(prim_ids != 0xFFFFFFFF)
    out = {k: np.zeros((len(ys), n)) for k, n in (("scene_color", 4), ("a", 4), ("b", 4), ("c", 4), ("d", 4), ("d_per_pixel", 3), ("normal", 3), ("vertex_color", 3), ("ao_rgb", 3),
                                                   ("range_scene_color", 4), ("range_b", 4), ("range_c", 4))}
    out["ambiguous"] = np.zeros(len(ys), bool)
    out["clipped"] = np.zeros(len(ys), bool)          # the pixel's triangle crosses the near / far plane, w = 0 or the guard band
    pid = prim_ids[ys, xs].astype(np.int64)
    for d in draws:
        n_tris = len(d["idx"]) // 3
        n_inst = 1 if d["instances"] is None else len(d["instances"])
        sel = np.nonzero((pid >= d["prim_base"]) & (pid < d["prim_base"] + n_tris * n_inst))[0]
        if not len(sel):
            continue
        local = pid[sel] - d["prim_base"]
        inst_i, tri = local // n_tris, local % n_tris
        tex = np.asarray(d["texel"], dtype=F64)              # 7 x RGBA8
        images = d.get("images") or [None] * 7
        chains = [None if im is None else isamp.mip_chain(im, i == 0 and control != "slot0_unorm", control) for i, im in enumerate(images)]
        for ii in np.unique(inst_i):
            m = sel[inst_i == ii]
            t = tri[inst_i == ii]
            clip, wp, wn, uv = vertex_stage(d["verts"], None if d["instances"] is None else d["instances"][ii], model, view, proj)
            corner = np.asarray(d["idx"], dtype=np.int64).reshape(-1, 3)[t]                 # (k, 3)
            c3 = clip[corner]                                                                # (k, 3, 4)
            A = np.stack([c3[..., 0], c3[..., 1], c3[..., 3]], axis=1)                       # rows x, y, w; columns = corners
            Ainv = np.linalg.inv(A)

            def weights(px, py):
                # the pixel centre in NDC (viewport 0, 0, W, H): the point of the triangle's plane that projects there is
                # sum(l_i * clip_i) with A l ~ (u, v, 1); normalised weights are the perspective-correct barycentrics
                u, v = (px + 0.5) / W * 2.0 - 1.0, (py + 0.5) / H * 2.0 - 1.0
                l = np.einsum("kij,kj->ki", Ainv, np.stack([u, v, np.ones_like(u)], axis=1))
                return l / l.sum(axis=1, keepdims=True)

            def varyings(px, py):
                l = weights(px, py)
                return (np.einsum("ki,kij->kj", l, wp[corner]), np.einsum("ki,kij->kj", l, wn[corner]), np.einsum("ki,kij->kj", l, uv[corner]))
            px, py = xs[m].astype(F64), ys[m].astype(F64)
            P0, N0, UV0 = varyings(px, py)
            out["vertex_color"][m] = np.einsum("ki,kij->kj", weights(px, py), np.asarray(d["verts"]["Color"], dtype=F64)[corner])
            # dFdx / dFdy: differences inside the 2x2 quad, the partner invocation extrapolating THIS triangle (helper lane)
            sx, sy = np.where(xs[m] & 1, 1.0, -1.0), np.where(ys[m] & 1, 1.0, -1.0)
            Ph, _, UVh = varyings(px - sx, py)
            Pv, _, UVv = varyings(px, py - sy)
            pos_dx, pos_dy = (P0 - Ph) * sx[:, None], (P0 - Pv) * sy[:, None]
            st1, st2 = (UV0 - UVh) * sx[:, None], (UV0 - UVv) * sy[:, None]
            k = len(m)
            smp, rng = np.broadcast_to(tex / 255.0, (k, 7, 4)).copy(), np.zeros((k, 7, 4))
            if control != "slot0_unorm":
                smp[:, 0, :3] = srgb_to_linear(tex[0, :3])          # sampler1 is R8G8B8A8_SRGB (ZE:5878); the others UNORM
            if any(c is not None for c in chains):
                # the smallest altitude of the triangle, or of the polygon the clipper leaves of it (its re-snapped vertices move the
                # interpolation plane as the snap moves a triangle's): a clipped triangle is no longer excused as a whole
                ut, inv = np.unique(t, return_inverse=True)
                alt, cut = altitudes(clip[np.asarray(d["idx"], dtype=np.int64).reshape(-1, 3)[ut]], W, H)
                alt = alt[inv.reshape(-1)]
                out["clipped"][m] = cut[inv.reshape(-1)]
                for i, ch in enumerate(chains):
                    if ch is not None:
                        smp[:, i], rng[:, i], amb = _sampled_slot(ch, i == 0 and control != "slot0_unorm", UV0, st1, st2, uv[corner], alt, control)
                        out["ambiguous"][m] |= amb
            base_color, metallic, rough = smp[:, 0, :3], smp[:, 1, 0], smp[:, 2, 0]
            tex_n, ao, emissive, mask = smp[:, 3, :3], smp[:, 4, 0], smp[:, 5, :3], smp[:, 6, 0]
            normal = compute_normal(pos_dx, pos_dy, st1, st2, N0, tex_n)
            packed = (normalize(normal) + 1.0) / 2.0
            out["scene_color"][m] = np.hstack([emissive, mask[:, None]])
            out["a"][m] = np.hstack([packed, np.ones((k, 1))])
            out["normal"][m] = normal                                       # ComputeNormal()'s result as Base.frag uses it (forward variant)
            out["ao_rgb"][m] = smp[:, 4, :3]                                # Base.frag's AmbientOcclution.rgb (its debug view 5)
            out["b"][m] = np.stack([metallic, np.ones(k), np.maximum(0.01, rough), np.ones(k)], axis=1)
            out["c"][m] = np.hstack([base_color, ao[:, None]])
            out["d"][m] = np.hstack([P0, np.ones((k, 1))])
            out["d_per_pixel"][m] = np.abs(pos_dx) + np.abs(pos_dy)       # how far the position moves per pixel step (x plus y)
            out["range_scene_color"][m] = np.hstack([rng[:, 5, :3], rng[:, 6, :1]])
            out["range_b"][m] = np.stack([rng[:, 1, 0], np.zeros(k), rng[:, 2, 0], np.zeros(k)], axis=1)
            out["range_c"][m] = np.hstack([rng[:, 0, :3], rng[:, 4, :1]])
    out["yx"] = (ys, xs)
    return out


def check_sampled_targets(mine, got):
    """GBuffer targets 1, 3 and 4 (scene colour, B, C) against base_scene()'s values: every channel of every unambiguous pixel within
    the range its float64 value spans over the error budget plus one code of output rounding (constant slots: range 0 - exact to the
    rounding).  got: the (k, 4) codes at mine["yx"].  -> dict ok, ambiguous (fraction), worst (largest error / tolerance), bad (pixel-target pairs outside)"""
    amb = mine["ambiguous"]
    worst, bad = 0.0, 0
    for k in ("scene_color", "b", "c"):
        err = np.abs(got[k] - mine[k] * 255.0)
        tol = mine["range_" + k] * 255.0 + 1.0
        r = (err / tol)[~amb]
        if r.size:
            worst = max(worst, float(r.max()))
            bad += int((r > 1.0).any(axis=1).sum())
    return {"ok": bad == 0, "ambiguous": float(amb.mean()) if len(amb) else 0.0, "worst": worst, "bad": bad}


# ----------------------------------------------------------------------------------------------- formats

def unorm(x, bits):
    """float -> UNORM code (round to nearest; ties are the implementation's business: compare within one code)"""
    mx = (1 << bits) - 1
    with np.errstate(invalid="ignore"):
        return np.floor(np.clip(np.nan_to_num(x, nan=0.0), 0.0, 1.0) * mx + 0.5).astype(np.int64)


def unpack_rgba8(w):
    w = np.asarray(w, dtype=np.uint32)
    return np.stack([(w >> s) & 255 for s in (0, 8, 16, 24)], axis=-1).astype(np.int64)


def unpack_a2r10g10b10(w):
    """VK_FORMAT_A2R10G10B10_UNORM_PACK32: B bits 0-9, G 10-19, R 20-29, A 30-31 -> (R, G, B, A) codes"""
    w = np.asarray(w, dtype=np.uint32)
    return np.stack([(w >> 20) & 1023, (w >> 10) & 1023, w & 1023, w >> 30], axis=-1).astype(np.int64)


def unpack_rgba16f(w):
    """(H, W) uint64 (four fp16) -> float64 (H, W, 4) and the raw codes"""
    codes = np.stack([(np.asarray(w, dtype=np.uint64) >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32, 48)], axis=-1).astype(np.uint16)
    return codes.view(np.float16).astype(F64), codes


def f16_ordinal(codes):
    """fp16 bit patterns -> integers ordered like the values (so that |a - b| counts representable steps)"""
    c = np.asarray(codes, dtype=np.int64)
    return np.where(c & 0x8000, -(c & 0x7FFF), c & 0x7FFF)


# ----------------------------------------------------------------------------------------------- BaseLighting.frag

def texture_linear_clamp(img, u, v):
    """texture(sampler2D, uv).r of a one-channel image: LINEAR filter, CLAMP_TO_EDGE (the shadow map's sampler, ZE:2532-2537)"""
    H, W = img.shape
    x, y = u * W - 0.5, v * H - 0.5
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    x0, y0 = np.floor(x), np.floor(y)
    a, b = x - x0, y - y0
    xi0, xi1 = np.clip(x0, 0, W - 1).astype(np.int64), np.clip(x0 + 1, 0, W - 1).astype(np.int64)
    yi0, yi1 = np.clip(y0, 0, H - 1).astype(np.int64), np.clip(y0 + 1, 0, H - 1).astype(np.int64)
    top = img[yi0, xi0] * (1 - a) + img[yi0, xi1] * a
    bot = img[yi1, xi0] * (1 - a) + img[yi1, xi1] * a
    return np.where(ok, top * (1 - b) + bot * b, np.nan)


def cube_face_constant(face_colors_srgb8, R):
    """textureLod(samplerCube, R, lod) for a cubemap whose six faces are each ONE colour (so no filter or mip choice matters):
    face selection by the major axis (Vulkan: +X, -X, +Y, -Y, +Z, -Z; z wins ties over y over x), R8G8B8A8_SRGB decode."""
    ax, ay, az = np.abs(R[..., 0]), np.abs(R[..., 1]), np.abs(R[..., 2])
    face = np.where((az >= ax) & (az >= ay), np.where(R[..., 2] >= 0, 4, 5),
                    np.where(ay >= ax, np.where(R[..., 1] >= 0, 2, 3), np.where(R[..., 0] >= 0, 0, 1)))
    lin = srgb_to_linear(np.asarray(face_colors_srgb8, dtype=F64)[:, :3])
    return lin[face]


def f_schlick(f0, f90, u):
    return f0 + (f90 - f0) * np.power(1.0 - u, 5.0)


def bxdf(diffuse_color, roughness, LoH, NoV, NoL, NoH):
    """DefaultLitBxDF, SH/Common.glsl:259-282 -> Diffuse + Specular"""
    F0 = 0.04
    F90 = saturate(50.0 * F0)
    F = f_schlick(F0, F90, LoH)
    a2 = roughness * roughness
    ggxv = NoL * np.sqrt(NoV * NoV * (1.0 - a2) + a2)
    ggxl = NoV * np.sqrt(NoL * NoL * (1.0 - a2) + a2)
    ggx = ggxv + ggxl
    with np.errstate(invalid="ignore", divide="ignore"):
        vis = np.where(ggx > 0.0, 0.5 / ggx, 0.0)
        f = (NoH * a2 - NoH) * NoH + 1.0
        D = a2 / (3.14159265359 * f * f)      # the shader's PI literal
    Fr = F * D * vis
    e_bias = 0.0 * (1.0 - roughness) + 0.5 * roughness
    e_factor = 1.0 * (1.0 - roughness) + (1.0 / 1.51) * roughness
    fd90 = e_bias + 2.0 * LoH * LoH * roughness
    Fd = f_schlick(1.0, fd90, NoL) * f_schlick(1.0, fd90, NoV) * e_factor
    return diffuse_color * (1.0 - F)[..., None] * Fd[..., None] + Fr[..., None]


def reflection_mip(roughness, cubemap_max_mip, control=None):
    """ComputeReflectionMipFromRoughness, SH/Common.glsl:191-198 (REFLECTION_CAPTURE_ROUGHEST_MIP 1, ..._ROUGHNESS_MIP_SCALE 1.2)"""
    level_from_1x1 = 1.0 - 1.2 * np.log2(np.maximum(roughness, 0.001))
    return (cubemap_max_mip if control == "cube_lod_max_mip" else cubemap_max_mip - 1.0) - level_from_1x1


# What the normal's error does to the reflected direction.  The normal reaches the deferred lighting pass as A2R10G10B10 codes: half a
# code is 1 / 1023 per component, sqrt(3) / 1023 in length; refract() moves R by at most about twice that for a unit V.  The forward
# variant's normal is unquantised, but a float32 implementation's differs from this statement's by less (the snap and float32 rounding).
R_ERR = 2.0 * np.sqrt(3.0) / 1023.0


def cube_boundary(R):
    """lookups whose face R does not decide: the two largest |R| components closer than R_ERR can move them (twice R_ERR)"""
    a = np.sort(np.abs(R), axis=-1)
    return (a[..., 2] - a[..., 1]) <= 2.0 * R_ERR


def pcf(P, shadow_map, view, pcf_eps=0.0):
    """ComputeShadowCoord + ComputePCF(sampler, ShadowCoord / ShadowCoord.w, 2), SH/Common.glsl:294-342, at the positions P (..., 3)"""
    bias = np.array([[0.5, 0, 0, 0.5], [0, 0.5, 0, 0.5], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=F64)      # BiasMat (columns as written in the GLSL)
    SB = bias @ mat(view["ShadowmapSpace"])
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = np.concatenate([P, np.ones(P.shape[:-1] + (1,))], axis=-1) @ SB.T
        sc = sc / sc[..., 3:4]
        SD = shadow_map.shape[0]
        dx = 1.5 * 1.0 / SD
        total = np.zeros(P.shape[:-1])
        for x in range(-2, 3):
            for y in range(-2, 3):
                f = np.ones(P.shape[:-1])
                inside = (sc[..., 2] > -1.0) & (sc[..., 2] < 1.0)
                dist = texture_linear_clamp(shadow_map.astype(F64), sc[..., 0] + dx * x, sc[..., 1] + dx * y)
                f = np.where(inside & (sc[..., 3] > 0.0) & (dist < sc[..., 2] + pcf_eps), 0.1, f)
                total += f
        return total / 25.0


def refract_view(N, P, view):
    """refract(V, normalize(N), 1.00 / 1.52) with V = normalize(cameraInfo.xyz - P)"""
    V = normalize(np.asarray(view["CameraInfo"], dtype=F64)[:3] - P)
    eta = 1.00 / 1.52
    with np.errstate(invalid="ignore", divide="ignore"):
        Nn = normalize(N)
        dNI = dot(Nn, V)
        k = 1.0 - eta * eta * (1.0 - dNI * dNI)
        return np.where((k < 0.0)[..., None], 0.0, eta * V - (eta * dNI + np.sqrt(np.maximum(k, 0.0)))[..., None] * Nn)


def quad_vertex_colour(W, H):
    """fragColor of the lighting quad (debug view 6): Background.vert's six vertices (two triangles, colours red / blue / green and
    red / green / blue) drawn at w = 1, interpolated with the barycentrics of each pixel centre in the triangle that contains it"""
    pos = np.array([(-1.0, -1.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0), (1.0, 1.0), (1.0, -1.0)])
    col = np.array([(1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    X, Y = (xx + 0.5) / W * 2.0 - 1.0, (yy + 0.5) / H * 2.0 - 1.0
    out = np.zeros((H, W, 3))
    done = np.zeros((H, W), bool)
    for t in (0, 1):
        p, c = pos[3 * t:3 * t + 3], col[3 * t:3 * t + 3]
        A = np.array([[p[0, 0], p[1, 0], p[2, 0]], [p[0, 1], p[1, 1], p[2, 1]], [1.0, 1.0, 1.0]])
        lam = np.einsum("ij,jhw->ihw", np.linalg.inv(A), np.stack([X, Y, np.ones_like(X)]))
        inside = np.all(lam >= -1e-12, axis=0) & ~done
        out[inside] = np.einsum("ihw,ic->hwc", lam, c)[inside]
        done |= inside
    return out


# ----------------------------------------------------------------------------------------------- comparisons of lit frames

def _within_one(a, b):
    return np.all(np.abs(a - b) <= 1, axis=-1)


R_OFFSETS = [np.eye(3)[i] * s * R_ERR for i in range(3) for s in (-1.0, 1.0)]


def check_lit(have, shade, R, mask=None, r_spread=False):
    """the lit colour within one LSB on 99.9 % of the pixels, with the PCF ties of tests/test_oracle_independent.py; lookups on a cube
    face boundary (cube_boundary) excused.  shade(eps, r_offset) -> codes.  r_spread: also accept what R moved by ie.R_ERR along
    each axis spans (the forward variant, whose normal is this statement's own).  -> (fraction ok, cube-excused fraction, PCF on-edge
    fraction)"""
    want, pcf = shade(0.0, None), [shade(-4e-7, None), shade(4e-7, None)]
    on_edge = (pcf[0] != pcf[1]).any(axis=-1)
    spread = pcf + ([shade(0.0, off) for off in R_OFFSETS] if r_spread else [])
    lo, hi = np.minimum.reduce(spread + [want]) - 1, np.maximum.reduce(spread + [want]) + 1
    moved = (lo + 1 != hi - 1).any(axis=-1)
    ok = _within_one(have[..., :3], want) | (moved & np.all((have[..., :3] >= lo) & (have[..., :3] <= hi), axis=-1))
    boundary = cube_boundary(R)
    sel = ~boundary if mask is None else (~boundary & mask)
    return float(ok[sel].mean()), float(boundary[mask if mask is not None else slice(None)].mean()), float(on_edge.mean())


def lighting(gb, shadow_map, view, cube, W, H, pcf_eps=0.0, forward=False, control=None, out=None, r_offset=None, debug_view=0):
    """BaseLighting.frag:147-254 for every pixel of the W x H quad, the switch on SPEC_CONSTANTS included (debug_view).
    forward=True: Base.frag:46-123 instead - the same text except that N is used as ComputeNormal() returned it, AO is not saturated,
    there is no Mask, and case 0 shows FinalColor * ShadowFactor (after the gamma); gb then holds the fragment's unquantised inputs.

    gb: dict scene_color / a / b / c (float RGBA as texture() returns them) and d (fp16 values), each (H, W, 4); view: XkView record
    cube: the six face colours of a cubemap whose faces are each ONE colour (no filter or lod choice matters), or the cubemap's mip
    chain (independent_sampler.cube_chain): textureLod at ComputeReflectionMipFromRoughness(Roughness, SKY_MAXMIPS), SKY_MAXMIPS =
    view.LightsCount[3].  control: "cube_lod_max_mip" or one of independent_sampler's (negative controls).  out: a dict that receives
    R (the reflected direction the cubemap is sampled with).  r_offset: a vector added to R before the cubemap lookup (a caller that
    wants to know what R's own error does evaluates with offsets of that size, as with pcf_eps)
    pcf_eps: added to the reference depth of the 25 shadow comparisons - the shader's one discontinuity: a caller that wants to know
    which pixels sit on it evaluates with +-eps and looks at the spread
    debug_view: 0-8 and >= 10 (the default case, FinalColor * ShadowFactor); view 9 is gbuffer_vis()'s, which this calls with
    FinalColor.  Forward: Base.frag:123-143's own table (base colour without gamma, AmbientOcclution.rgb = gb["ao_rgb"], the
    interpolated vertex colour gb["vertex_color"], and case 9 = the default).
    -> (H, W, 3) float colour before the UNORM store
    """
    PI = 3.14159265359
    base_color = gb["c"][..., :3]
    metallic = saturate(gb["b"][..., 0])
    roughness = np.maximum(0.01, saturate(gb["b"][..., 2]))
    normal = gb["a"][..., :3] * 2.0 - 1.0
    ao = gb["c"][..., 3] if forward else saturate(gb["c"][..., 3])
    mask = gb["scene_color"][..., 3]
    N = normal if forward else normalize(normal)
    P = gb["d"][..., :3]
    cam = np.asarray(view["CameraInfo"], dtype=F64)[:3]
    V = normalize(cam - P)
    NdotV = saturate(dot(N, V))

    shadow = pcf(P, shadow_map, view, pcf_eps)

    direct = np.zeros(P.shape)
    diffuse_color = base_color * (1.0 - metallic)[..., None]
    n_dir, n_point = int(view["LightsCount"][0]), int(view["LightsCount"][1])
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n_dir):
            Lt = view["DirectionalLights"][i]
            L = normalize(np.asarray(Lt["Direction"], dtype=F64)[:3]) * np.ones(P.shape)
            Hh = normalize(V + L)
            b = bxdf(diffuse_color, roughness, saturate(dot(L, Hh)), NdotV, saturate(dot(N, L)), saturate(dot(N, Hh)))
            ndotl = np.clip(dot(normalize(N), L), 0.0, 1.0)
            apply = ndotl[..., None] * F64(Lt["Color"][3]) * np.asarray(Lt["Color"], dtype=F64)[:3]
            direct = direct + apply * b * shadow[..., None]
        for i in range(n_point):
            Lt = view["PointLights"][i]
            lp = np.asarray(Lt["Position"], dtype=F64)[:3]
            L = normalize(lp - P)
            Hh = normalize(V + L)
            b = bxdf(diffuse_color, roughness, saturate(dot(L, Hh)), NdotV, saturate(dot(N, L)), saturate(dot(N, Hh)))
            ndotl = np.clip(dot(normalize(N), L), 0.0, 1.0)
            falloff = F64(Lt["Direction"][3])
            dist = np.sqrt(dot(lp - P, lp - P))
            att = 1.0 - (np.clip(dist, 0.0, falloff) - 0.0) / (falloff - 0.0) * (1.0 - 0.0) + 0.0      # 1 - remap(dist, 0, falloff, 0, 1)
            apply = (ndotl * F64(Lt["Color"][3]))[..., None] * np.asarray(Lt["Color"], dtype=F64)[:3] * att[..., None]
            direct = direct + apply * b

        indirect = diffuse_color / PI * ao[..., None] * 0.3 * shadow[..., None]

        # ComputeF0(0.5, BaseColor, Metallic); EnvBRDFApprox; refract; cubemap; GetSpecularOcclusion
        bc = np.clip(base_color, 0.04, 1.0)
        dsf0 = 0.04 * 2.0 * 0.5
        refl_spec = (1.0 - metallic)[..., None] * dsf0 + metallic[..., None] * bc
        r = roughness[..., None] * np.array([-1.0, -0.0275, -0.572, 0.022]) + np.array([1.0, 0.0425, 1.04, -0.04])
        a004 = np.minimum(r[..., 0] * r[..., 0], np.exp2(-9.28 * NdotV)) * r[..., 0] + r[..., 1]
        AB = np.stack([-1.04 * a004 + r[..., 2], 1.04 * a004 + r[..., 3]], axis=-1)
        F90 = saturate(50.0 * refl_spec[..., 1])
        refl_brdf = refl_spec * AB[..., 0:1] + (F90 * AB[..., 1])[..., None]
        eta = 1.00 / 1.52
        Nn = normalize(N)
        dNI = dot(Nn, V)
        k = 1.0 - eta * eta * (1.0 - dNI * dNI)
        R = np.where((k < 0.0)[..., None], 0.0, eta * V - (eta * dNI + np.sqrt(np.maximum(k, 0.0)))[..., None] * Nn)
        if out is not None:
            out["R"] = R
        if r_offset is not None:
            R = R + np.asarray(r_offset, F64)
        if np.asarray(cube[0]).ndim == 4:
            lod = reflection_mip(roughness, float(np.uint32(view["LightsCount"][3])), control)
            refl_l = isamp.sample_cube_array(cube, R.reshape(-1, 3), lod.reshape(-1), control).reshape(R.shape) * 10.0
        else:
            refl_l = cube_face_constant(cube, R) * 10.0
        refl_v = saturate(np.power(NdotV + ao, roughness * roughness) - 1.0 + ao)
        refl = refl_l * refl_v[..., None] * refl_brdf

        if forward:
            final = np.power(direct + indirect + refl, 0.4545)
        else:
            final = (direct + indirect + refl) * mask[..., None]
            final = np.power(final, 0.4545)
    v3 = lambda x: np.repeat(np.asarray(x)[..., None], 3, axis=-1)      # noqa: E731  vec3(float)
    if forward:                                                         # Base.frag:123-143
        table = {1: base_color, 2: v3(metallic), 3: v3(roughness), 4: normal, 7: refl, 8: v3(shadow),
                 5: gb["ao_rgb"] if debug_view == 5 else None, 6: gb["vertex_color"] if debug_view == 6 else None}
        return table[debug_view] if debug_view in table else final * shadow[..., None]
    table = {0: final, 2: v3(metallic), 3: v3(roughness), 4: normal, 5: v3(ao), 7: refl, 8: v3(shadow)}       # BaseLighting.frag:228-253
    if debug_view in table:
        return table[debug_view]
    if debug_view == 1:
        return np.power(base_color, 0.4545)
    if debug_view == 6:
        return quad_vertex_colour(W, H)
    if debug_view == 9:
        return gbuffer_vis(gb, shadow_map, view, cube, W, H, final)["colour"]
    return final * shadow[..., None]


# ----------------------------------------------------------------------------------------------- BaseLighting.frag: GBufferVis

U32 = 2.0 ** -24
# The mosaic's thresholds: fragTexCoord = (x + 1/2) / W is one correctly rounded division; Step = (1 - zw / xy) / 3 and Step * (k - EmptyRatio)
# are at most five float32 roundings of quantities below 4: a pixel whose fragTexCoord lies within 8u of a threshold is not decided.
THRESHOLD_ULPS = 8.0
# The re-sampling position: UV = fragTexCoord * 3 / (1 - EmptyRatio) carries <= 4u of |UV|; bilinear weights are an implementation's
# sub-texel precision (this build: 8 bits, Vulkan's subTexelPrecisionBits), i.e. the position moves by up to 1/512 texel.
SUBTEXEL = 1.0 / 512.0


def gbuffer_vis(gb, shadow_map, view, cube, W, H, final, control=None, pcf_eps=4e-7, aniso=True):
    """GBufferVis(FinalColor), SH/BaseLighting.frag:42-145, word for word, for every pixel of the W x H quad.

    gb: the GBuffer as texture() sees its texels (lighting()'s dict: scene_color / a / b / c float, d fp16 values, (H, W, 4)).  The
    attachments are re-sampled with RHICreateSampler's state (ZE:6520-6560): LINEAR, REPEAT, anisotropyEnable with the device's
    maxAnisotropy, one mip level - through independent_sampler's scheme, N = ceil(Pmax / Pmin) taps along the major axis, the
    footprint 3 / (1 - EmptyRatio) texels per pixel on each axis.  aniso=False: one bilinear tap (oracle/CONTRACT.md row 7).
    final: FinalColor (H, W, 3).  control: "mosaic_no_aniso" or "cell6_step_y" (Step.y * 3 in the sixth cell: the shader has Step.x).
    -> dict: colour (H, W, 3), tol (H, W, 3) (the span over the error budget: sub-texel position, PCF ties), cell (H, W) (0-7 the
    branch, 8 its white frame, -1 FinalColor), excused (H, W) (fragTexCoord on a threshold, a refraction on a cube face boundary)
    """
    vi = np.asarray(view["ViewportInfo"], dtype=F64)
    ERx, ERy = vi[2] / vi[0], vi[3] / vi[1]
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    tx, ty = (xx + 0.5) / W, (yy + 0.5) / H
    Sx, Sy = (1.0 - ERx) / 3.0, (1.0 - ERy) / 3.0
    s6 = Sy if control == "cell6_step_y" else Sx
    branches = [((tx < Sx) & (ty < Sy), 1, 1), ((tx < Sx * 2) & (ty < Sy), 2, 1), ((tx < Sx * 3) & (ty < Sy), 3, 1),
                ((tx < Sx) & (ty < Sy * 2), 1, 2), ((tx < 1.0) & (ty < Sy * 2) & (tx > Sx * 2), 3, 2),
                ((tx < Sx) & (ty < s6 * 3), 1, 3),                                          # the shader's own `Step.x * 3.0f`
                ((tx < Sx * 2) & (tx > Sx) & (ty < Sy * 3) & (ty > Sy * 2), 2, 3),
                ((tx < Sx * 3) & (tx > Sx * 2) & (ty < Sy * 3) & (ty > Sy * 2), 3, 3)]
    cell = np.full((H, W), -1)
    for k, (cond, bx, by) in enumerate(branches):
        new = cond & (cell == -1)
        cell[new] = k
        cell[new & ((tx > Sx * (bx - ERx)) | (ty > Sy * (by - ERy)))] = 8
    thr_x = [Sx, Sx * 2, Sx * 3, 1.0] + [Sx * (k - ERx) for k in (1, 2, 3)]
    thr_y = [Sy, Sy * 2, Sy * 3, Sx * 3] + [Sy * (k - ERy) for k in (1, 2, 3)]
    excused = np.zeros((H, W), bool)
    for thr, t in ((thr_x, tx), (thr_y, ty)):
        for v in thr:
            excused |= np.abs(t - v) <= THRESHOLD_ULPS * U32
    colour, tol = np.array(final, dtype=F64), np.zeros((H, W, 3))
    colour[cell == 8] = 1.0
    colour[cell == 5] = 0.0
    ys, xs = np.nonzero((cell >= 0) & (cell <= 7) & (cell != 5))
    k = len(ys)
    if not k:
        return {"colour": colour, "tol": tol, "cell": cell, "excused": excused}
    UV = np.stack([tx[ys, xs] * 3.0 / (1.0 - ERx), ty[ys, xs] * 3.0 / (1.0 - ERy)], axis=1)
    duv = np.broadcast_to([3.0 / (1.0 - ERx) / W, 0.0, 0.0, 3.0 / (1.0 - ERy) / H], (k, 4))
    no_aniso = control == "mosaic_no_aniso" or not aniso
    shift = (SUBTEXEL + 4.0 * U32 * np.abs(UV) * np.array([W, H])) / np.array([W, H])
    c_k = cell[ys, xs]

    def evaluate(uv, eps):
        t = {n: isamp.sample_2d_array([gb[n]], 0, uv, duv, "no_aniso" if no_aniso else None, [np.asarray(gb[n], F64)])[0]
             for n in ("scene_color", "a", "b", "c", "d")}
        N = normalize(t["a"][:, :3] * 2.0 - 1.0)
        P = t["d"][:, :3]
        out = np.zeros((k, 3))
        sel = lambda c: c_k == c                                                      # noqa: E731
        out[sel(0)] = np.power(np.maximum(t["c"][:, :3], 0.0), 0.4545)[sel(0)]
        out[sel(1)] = saturate(t["b"][:, 0:1])[sel(1)]
        out[sel(2)] = np.maximum(0.01, saturate(t["b"][:, 2:3]))[sel(2)]
        out[sel(3)] = N[sel(3)]
        out[sel(4)] = saturate(t["c"][:, 3:4])[sel(4)]
        R = refract_view(N, P, view)
        if np.any(sel(6)):
            if np.asarray(cube[0]).ndim == 4:
                L = isamp.sample_cube_array(cube, R[sel(6)], np.zeros(int(sel(6).sum())))
            else:
                L = cube_face_constant(cube, R[sel(6)])
            out[sel(6)] = L * 10.0
        if np.any(sel(7)):
            out[sel(7)] = pcf(P[sel(7)], shadow_map, view, eps)[:, None]
        return out, R
    mid, R = evaluate(UV, 0.0)
    lo, hi = mid.copy(), mid.copy()
    for su, sv in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        v = evaluate(UV + shift * (su, sv), 0.0)[0]
        lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    for eps in (-pcf_eps, pcf_eps):
        v = evaluate(UV, eps)[0]
        lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    colour[ys, xs], tol[ys, xs] = mid, hi - lo
    excused[ys, xs] |= (c_k == 6) & cube_boundary(R)
    return {"colour": colour, "tol": tol, "cell": cell, "excused": excused}
