"""A second, independent statement of the frame's geometry path - the uniforms, the camera depth pass and the shadow map - in float64.

TEST INFRASTRUCTURE.  Written from the reference's host code and shaders (ZE = Engine/ZeldaEngine/ZeldaEngine.cpp, SH = its Shaders/):
UpdateUniformBuffer ZE:4585-4664, the pipeline state ZE:5100-5145, the shadow pass's viewport and depth bias ZE:3255-3287, SH/Base.vert,
SH/BaseInstanced.vert, SH/Shadowmap.vert, SH/ShadowmapInstanced.vert - and from the rasterisation chapter of the Vulkan 1.3
specification.  NOT from oracle/ or the HIP kernels under zeldaengine_amd/csrc/, and it imports nothing from them: the oracle and the
kernels share one author, so a line both of them misread the same way passes every parity test; this file is the other reading.

What it states:

* `frame_uniforms`: the three UBOs UpdateUniformBuffer writes (camera MVP, shadow MVP, XkView), with glm's right-handed, depth
  zero-to-one `lookAt` / `perspective` from their published definitions, `glm::rotate` about +Z for the stage roll, the `[1][1] *= -1`
  of both projections (the camera's only on the UBO copy: `ViewProjSpace` takes the unflipped one, ZE:4617-4629), `ShadowmapSpace`
  without the model matrix (ZE:4628), and the point-light spiral (ZE:4637-4646).
* `raster`: the whole scene rasterised with 2D-homogeneous edge functions (`independent_raster.covers_clip_space`'s formulation: no
  clipper is needed for triangles that cross w = 0), viewport (0, 0, W, H, 0, 1) with no y flip (ZE:3255-3262, 3396-3402), pixel centres
  at (x + 1/2, y + 1/2); camera pass: cull BACK, front = COUNTER_CLOCKWISE, LESS against the clear 1.0 so the first draw keeps a tie,
  depthClampEnable FALSE so fragments outside [0, 1] are discarded (ZE:5100-5145); shadow pass: cull NONE, depth bias
  o = 7.5 m + 1.25 r (vkCmdSetDepthBias(1.25, 0, 7.5), ZE:3280-3287) with m = max(|dz/dx|, |dz/dy|) and r = 2^(e - 23) (Vulkan 1.3
  "Depth Bias", D32_SFLOAT: e the largest exponent of the primitive's depths), the biased depth clamped to [0, 1], LESS_OR_EQUAL.
  Draw order is the engine's (non-instanced draws first, ZE:3445-3476), primitive ids are numbered instance-major inside a draw.

Where it cannot decide - the ambiguity mask.  The shaders run in float32 and Vulkan leaves sub-pixel precision to the implementation
(this build snaps to 1/256 px).  A pixel is excused only where a float32 implementation could legitimately decide
otherwise, and every bound below is derived, not tuned:

* coverage: the pixel centre lies within tau px of an edge of a triangle that covers or nearly covers it, with
  tau = 1/256 (the snap moves a vertex by at most 1/512 per axis, an edge by at most sqrt(2)/512 < 1/256)
      + the float32 error of the vertex transform, propagated to the edge function (see `_vertex_error` and `_setup`), per pixel
      + for a clipped triangle, the clipper's re-snapped intersection: another 1/256 + (K_EYE + K_PROJ) u GUARD max(W, H) px;
* depth: the nearest candidate could be overtaken - the second-nearest certain fragment, or any uncertain one (near an edge, near the
  depth clip, facing undecidable) - within the sum of their depth tolerances, each |grad z| tau plus the propagated vertex-depth error
  plus a few float32 ulps of the plane evaluation;
* shadow pass, a caster clipped in depth (near or far plane, or w <= 0): not excused, but held to a derived bias budget
  (`_clipped_bias`, which quotes Vulkan 1.3 "Depth Bias" and "Primitive Clipping"): r anywhere in [0, r_hi] - the polygon clipped to
  0 <= z <= w, any piece of it, the float32 rounding of an intersection depth across a power of two; an unclipped vertex beyond the far
  plane is not admissible - and m the plane's, within 3 dz / h of any fan of the clipped polygon (h its smallest altitude over every
  three vertices; a bound that fails when h is under the snap leaves the caster uncertain).  A texel stays excused only where such a
  caster's budget reaches below the nearest fragment's tolerance, as an uncertain fragment's would.  raster() reports what the old rule
  (every depth-clipped caster excused) excused because of clipping alone, "clip_excused".
"""
import math

import numpy as np

from independent_eval import make_rot_matrix, mat, vertex_stage

F64 = np.float64
U = 2.0 ** -24           # unit roundoff of float32
SNAP = 1.0 / 256.0       # sub-pixel precision chosen by this build (Vulkan: subPixelPrecisionBits, implementation-defined)
GUARD = 4.0              # the clipper's guard band, in viewports (this build's stated choice)
# The float32 error of the vertex stage, split where it enters (u = 2^-24, bounds relative to the sum of the magnitudes of the terms):
# K_EYE: the position in eye space, view * model * (instance transform): a 4-term dot product costs 4u (gamma_4); the instance transform
# (scale, mat3 row product, + position) 5u, model and view 4u each; their entries were computed in float32 - lookAt (normalize: sqrt,
# division; cross; dot) <= 6u, rotate / MakeRotMatrix (sin, cos, two products) <= 4u each: 27u, rounded up to 32u.  This error MOVES the
# vertex in 3D: its effect on the screen and on depth is propagated through the projection exactly (correlated in x, y, z, w).
K_EYE = 32.0
# K_PROJ: the projection's own rounding of each clip coordinate, independent per coordinate: a 4-term dot product 4u and the entries of
# perspective (tan, two divisions) <= 3u: 7u, rounded up to 8u.
K_PROJ = 8.0
# K_PLANE: the rasteriser's own float32 evaluation of depth: a plane anchored at one vertex, z0 + dzdx dx + dzdy dy, after a reciprocal
# and the setup products: <= 8u of |z| + |grad z| (distance to the anchor), the anchor inside the guard band.
K_PLANE = 8.0


# ---------------------------------------------------------------------------------------------------------------- glm, restated

def normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(np.dot(v, v))


def look_at(eye, center, up):
    """glm::lookAtRH: f = normalize(center - eye), s = normalize(cross(f, up)), u = cross(s, f); rows s, u, -f; translation -dot."""
    eye, center, up = (np.asarray(a, dtype=F64) for a in (eye, center, up))
    f = normalize(center - eye)
    s = normalize(np.cross(f, up))
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[0, 3], m[1, 3], m[2, 3] = -np.dot(s, eye), -np.dot(u, eye), np.dot(f, eye)
    return m


def perspective(fovy, aspect, z_near, z_far):
    """glm::perspectiveRH_ZO (GLM_FORCE_DEPTH_ZERO_TO_ONE, Vulkan): x' = x / (aspect tan(fovy/2)), y' = y / tan(fovy/2),
    z' = far / (near - far) z - far near / (far - near), w' = -z."""
    t = math.tan(fovy / 2.0)
    m = np.zeros((4, 4))
    m[0, 0] = 1.0 / (aspect * t)
    m[1, 1] = 1.0 / t
    m[2, 2] = z_far / (z_near - z_far)
    m[3, 2] = -1.0
    m[2, 3] = -(z_far * z_near) / (z_far - z_near)
    return m


def rotate_z(angle):
    """glm::rotate(mat4(1), angle, vec3(0, 0, 1)): the right-handed rotation about +Z"""
    c, s = math.cos(angle), math.sin(angle)
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    return m


def cube_mips(dim):
    """mipLevels of a cubemap face of dim x dim texels: floor(log2(dim)) + 1 (LoadTextureAsset, ZE:6887), 0 without a cubemap"""
    return int(math.floor(math.log2(dim))) + 1 if dim else 0


# ---------------------------------------------------------------------------------------------------------------- the uniforms

CONTROLS = ("shadow_without_model", "projection_y_unflipped", "spiral_roll_sign")


def frame_uniforms(cam, dir_lights, point_lights, W, H, roll_stage=0.0, roll_light=0.0, spot_lights=(), cube_dim=0, time=0.0, control=None):
    """UpdateUniformBuffer (ZE:4585-4664) for a frame of W x H pixels, in float64 from the float32 inputs.

    cam: abi.Camera; dir_lights / point_lights / spot_lights: XkLight arrays as submitted (UpdateWorld copies them into the View,
    ZE:4296-4308); cube_dim: the cubemap's face size (LightsCount.w = CubemapMaxMips).
    control: None, or one of CONTROLS - a deliberately wrong statement for the negative controls of the tests.
    -> {"cam": {Model, View, Proj}, "shadow": {Model, View, Proj}, "view": XkView fields}, matrices 4 x 4 in row, column indexing.
    """
    pos = np.array(cam.Position[:], dtype=F64)
    lookat = np.array(cam.Lookat[:], dtype=F64)
    fov, z_near, z_far = F64(cam.FOV), F64(cam.zNear), F64(cam.zFar)
    main_light = np.asarray(dir_lights[0]["Position"][:3], dtype=F64) if len(dir_lights) else np.zeros(3)    # View is zero-initialised
    local_to_world = rotate_z(roll_stage)                                                          # ZE:4609
    shadow_view = look_at(main_light, np.zeros(3), (0.0, 0.0, 1.0))                               # ZE:4610
    shadow_proj = perspective(math.radians(fov), 1.0, z_near, z_far)                              # ZE:4611: aspect 1, the camera's FOV
    camera_view = look_at(pos, lookat, (0.0, 0.0, 1.0))                                            # ZE:4614, CameraUp = +Z (ZE:4589)
    camera_proj = perspective(math.radians(fov), F64(W) / F64(H), z_near, z_far)                  # ZE:4615
    flip = np.diag([1.0, 1.0 if control == "projection_y_unflipped" else -1.0, 1.0, 1.0])          # proj[1][1] *= -1: column 1, row 1
    shadow_proj = flip @ shadow_proj                                                               # ZE:4612 (before ShadowmapSpace)
    cam_ubo = {"Model": local_to_world, "View": camera_view, "Proj": flip @ camera_proj}          # ZE:4617-4621 (the UBO's copy only)
    shadow_ubo = {"Model": np.eye(4) if control == "shadow_without_model" else local_to_world, "View": shadow_view, "Proj": shadow_proj}
    n_point = len(point_lights)
    sign = 1.0 if control == "spiral_roll_sign" else -1.0
    spiral = np.zeros((n_point, 4))
    for i in range(n_point):                                                                       # ZE:4637-4646
        deg = (i / n_point) * 360.0 + sign * roll_light * 100.0
        dist = (i / n_point) * 5.0 + 2.5
        spiral[i] = (math.sin(math.radians(deg)) * dist, math.cos(math.radians(deg)) * dist, 1.5, 1.0)
    view = {"ViewProjSpace": camera_proj @ camera_view,                                            # ZE:4627: the UNflipped projection
            "ShadowmapSpace": shadow_proj @ shadow_view,                                           # ZE:4628: no model matrix
            "LocalToWorld": local_to_world,
            "CameraInfo": np.array([*pos, fov]),
            "ViewportInfo": np.array([W, H, 0.0, 0.0]),                                            # no ImGui bars (ZE:4577-4578)
            "LightsCount": np.array([len(dir_lights), n_point, len(spot_lights), cube_mips(cube_dim)]),
            "PointPositions": spiral, "Time": F64(time), "zNear": z_near, "zFar": z_far}
    return {"cam": cam_ubo, "shadow": shadow_ubo, "view": view}


# ---------------------------------------------------------------------------------------------------------------- the vertex stage

def _vertex_error(verts, inst, ubo):
    """Bounds on the float32 error of the vertex stage: the same chain as the shader with every value and matrix entry replaced by its
    absolute value.  -> eye-space error per component (n, 3) (K_EYE), the projection's rounding per clip coordinate (n, 4) (K_PROJ)"""
    p = np.abs(np.asarray(verts["Position"], dtype=F64))
    if inst is not None:
        p = (p * abs(F64(inst["InstancePScale"]))) @ np.abs(make_rot_matrix(np.asarray(inst["InstanceRotation"], dtype=F64))) \
            + np.abs(np.asarray(inst["InstancePosition"], dtype=F64))
    eye = np.hstack([p, np.ones((len(p), 1))]) @ np.abs(ubo["Model"]).T @ np.abs(ubo["View"]).T
    return K_EYE * U * eye[:, :3], K_PROJ * U * (eye @ np.abs(ubo["Proj"]).T)


def _triangles(draws, ubo):
    """every primitive of the frame in draw order -> clip (T, 3, 4), eye-space error (T, 3, 3), projection rounding (T, 3, 4),
    primitive id (T,)"""
    clips, eyes, projs, ids = [], [], [], []
    for d in draws:
        idx = np.asarray(d["idx"], dtype=np.int64).reshape(-1, 3)
        insts = [None] if d["instances"] is None else list(d["instances"])
        for ii, inst in enumerate(insts):
            clip = vertex_stage(d["verts"], inst, ubo["Model"], ubo["View"], ubo["Proj"])[0]
            e_eye, e_proj = _vertex_error(d["verts"], inst, ubo)
            clips.append(clip[idx])
            eyes.append(e_eye[idx])
            projs.append(e_proj[idx])
            ids.append(d["prim_base"] + ii * len(idx) + np.arange(len(idx)))
    if not clips:
        return np.zeros((0, 3, 4)), np.zeros((0, 3, 3)), np.zeros((0, 3, 4)), np.zeros(0, dtype=np.int64)
    return np.concatenate(clips), np.concatenate(eyes), np.concatenate(projs), np.concatenate(ids)


# ---------------------------------------------------------------------------------------------------------------- the clipper, restated
# Vulkan 1.3, "Primitive Clipping": primitives are clipped to the clip volume -w <= x <= w, -w <= y <= w, z_m <= z <= w (z_m = 0), and
# "if the primitive is clipped, the new vertices ... are computed by linear interpolation in clip space".  This build clips x / y at a
# guard band of GUARD w instead (equivalent coverage); the float64 polygon below is what any such clipper approximates.

PLANES_DEPTH = ((0.0, 0.0, 1.0, 0.0), (0.0, 0.0, -1.0, 1.0), (0.0, 0.0, 0.0, 1.0))              # z >= 0, z <= w, w >= 0
PLANES_GUARD = ((1.0, 0.0, 0.0, GUARD), (-1.0, 0.0, 0.0, GUARD), (0.0, 1.0, 0.0, GUARD), (0.0, -1.0, 0.0, GUARD))


def clip_polygon(c, planes):
    """Sutherland-Hodgman in float64, in clip space: c (n, 4) -> the polygon (m, 4) inside every plane (a . c >= 0), m = 0 if nothing
    is left"""
    poly = np.asarray(c, dtype=F64)
    for a in planes:
        if len(poly) == 0:
            break
        d = poly @ np.asarray(a)
        out = []
        for i in range(len(poly)):
            j = (i + 1) % len(poly)
            if d[i] >= 0:
                out.append(poly[i])
            if (d[i] >= 0) != (d[j] >= 0):
                out.append(poly[i] + d[i] / (d[i] - d[j]) * (poly[j] - poly[i]))
        poly = np.array(out).reshape(-1, 4)
    return poly if len(poly) >= 3 else np.zeros((0, 4))


def min_altitude(poly, W, H):
    """the smallest altitude, in pixels, of any three vertices of a clipped polygon (w > 0): a fan of it, whichever vertex it starts
    from, and any other triangulation, is made of such triples.  0 for fewer than three vertices."""
    if len(poly) < 3:
        return 0.0
    p = np.stack([poly[:, 0] / poly[:, 3] * W / 2.0, poly[:, 1] / poly[:, 3] * H / 2.0], axis=1)
    best = np.inf
    n = len(p)
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                a, b, c = p[i], p[j], p[k]
                area2 = abs((b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]))
                longest = max(np.hypot(*(b - a)), np.hypot(*(c - b)), np.hypot(*(a - c)))
                best = min(best, area2 / longest if longest > 0 else 0.0)
    return float(best)


def _clipped_bias(c, gz, W, H, control=None):
    """The depth bias of a primitive clipped in depth, c (3, 4) its clip coordinates, gz = |grad z| of its plane per pixel.
    -> (r_hi, dm_clip): every admissible r lies in [0, r_hi]; an implementation's m of any piece of its fan is within dm_clip of the
    plane's (inf: not bounded, a piece may be degenerate after the snap).

    r (Vulkan 1.3 "Depth Bias"): "the minimum resolvable difference for a given polygon is dependent on the maximum exponent, e, in the
    range of z values spanned by the primitive", r = 2^(e - n), and the primitive is the one rasterised: "Primitive Clipping" clips it to
    z_m <= z_c <= w_c first.  So r is that of the polygon clipped to 0 <= z <= w, or of any piece of it (its depths lie in the polygon's
    range: r in [0, r_poly]), or the float32 rounding of an intersection depth across a power of two (r_hi = 2 r_poly there).  An
    UNCLIPPED vertex beyond the far plane (z / w up to far / (far - near)) is not part of that primitive: an implementation that clips
    z > w per fragment must still take r from depths <= 1, and r from such a vertex is not admissible.
    m: the plane's, which clipping does not change; a fan evaluates it on re-snapped pieces.  Each piece vertex is off the plane by at
    most |grad z| (sqrt(2)/512 px of snap + the intersection's float32 position) + its float32 depth; that moves the gradient by at most
    sum_i dz_i / h_i <= 3 dz / h, h the smallest altitude over every three vertices of the clipped polygon (clipped with and without
    the far plane: a per-fragment far clip fans the latter), less the same displacement twice; the setup's own rounding adds
    8u |grad z| L / h, L the polygon's diameter."""
    near = (0.0, 0.0, 1.0, 1.0) if control == "gl_near" else PLANES_DEPTH[0]
    depth = (near,) + PLANES_DEPTH[1:]
    poly = clip_polygon(c, depth)
    if len(poly) == 0:
        return 0.0, 0.0
    zmax = float(np.max(np.abs(poly[:, 2] / poly[:, 3])))
    # the float32 intersection depth: the clip coordinates' error and the lerp and the division
    zup = zmax * (1.0 + (K_EYE + K_PROJ + K_PLANE) * U) + (K_EYE + K_PROJ + K_PLANE) * U
    r_hi = math.ldexp(1.0, math.frexp(zup)[1] - 1 - 23)
    pieces = [clip_polygon(c, depth + PLANES_GUARD), clip_polygon(c, (near, PLANES_DEPTH[2]) + PLANES_GUARD)]
    pieces = [p for p in pieces if len(p)]
    if not pieces:
        return r_hi, 0.0
    h = min(min_altitude(p, W, H) for p in pieces)
    scr = np.vstack([np.stack([p[:, 0] / p[:, 3] * W / 2.0, p[:, 1] / p[:, 3] * H / 2.0], axis=1) for p in pieces])
    diam = float(np.max(np.hypot(*(scr[:, None, :] - scr[None, :, :]).transpose(2, 0, 1))))
    zfar = float(np.max(np.abs(np.vstack(pieces)[:, 2] / np.vstack(pieces)[:, 3])))
    e_pos = math.sqrt(2.0) / 512.0 + (K_EYE + K_PROJ) * U * GUARD * max(W, H)
    dz = gz * e_pos + (K_EYE + K_PROJ + K_PLANE) * U * zfar
    h_eff = h - 2.0 * e_pos
    if not h_eff > 0.0:
        return r_hi, np.inf
    return r_hi, 3.0 * dz / h_eff + K_PLANE * U * gz * diam / h_eff


def _ndc_pieces(c):
    """control "ndc_lerp": the clipper's intersections interpolated AFTER the perspective divide - (x/w, y/w, z/w) clipped linearly
    against 0 <= z <= 1 and the guard band, fanned - as primitives with w = 1"""
    with np.errstate(all="ignore"):
        ndc = np.hstack([c[:, :3] / c[:, 3:4], np.ones((3, 1))])
    if not np.all(np.isfinite(ndc)):
        return []
    poly = clip_polygon(ndc, PLANES_DEPTH[:2] + PLANES_GUARD)
    return [np.stack([poly[0], poly[i], poly[i + 1]]) for i in range(1, len(poly) - 1)]


# ---------------------------------------------------------------------------------------------------------------- rasterisation

def _setup(C, Ee, Dp, P, W, H):
    """Per triangle: M (rows x, y, w of the clip coordinates; columns the vertices), Minv, and the first-order effect of the vertex
    errors.  Perturbing vertex j's clip position by dM_j changes lambda = Minv (X, Y, 1) by -Minv dM lambda, and the plane
    z = g3 . (X, Y, 1), g3 = Z^T Minv, by sum_j lambda_j (dZ_j - g3 . dM_j).  dM_j is the projection's rounding Dp (independent per
    coordinate) plus P dp_j for the eye-space error dp_j (|dp_j| <= Ee_j per component, correlated through P).
    -> dict: M, Minv, L (T, 3, 3) with |d lambda| <= L |lambda|, cz (T, 3) with |dz| <= sum_j |lambda_j| cz_j, g3 (T, 3), Q = Minv P_xyw"""
    with np.errstate(all="ignore"):
        M = np.transpose(C[:, :, [0, 1, 3]], (0, 2, 1))
        det = np.linalg.det(M) if len(C) else np.zeros(0)
        ok = np.isfinite(det) & (det != 0) & np.all(np.isfinite(C), axis=(1, 2))
        Minv = np.zeros_like(M)
        Minv[ok] = np.linalg.inv(M[ok])
        Pxyw = P[[0, 1, 3], :3]
        Q = Minv @ Pxyw                                                          # (T, 3 lambda, 3 eye components)
        Dxyw = np.transpose(Dp[:, :, [0, 1, 3]], (0, 2, 1))                      # (T, 3 rows, 3 vertices)
        L = np.abs(Minv) @ Dxyw + np.abs(Q) @ np.transpose(Ee, (0, 2, 1))
        Z = C[:, :, 2]
        g3 = np.einsum("tj,tjc->tc", Z, Minv)
        rz = P[2, :3][None, :] - (g3[:, 0:1] * P[0, :3] + g3[:, 1:2] * P[1, :3] + g3[:, 2:3] * P[3, :3])      # d z / d(eye position)
        cz = (np.einsum("tc,tjc->tj", np.abs(rz), Ee) + Dp[:, :, 2] + np.abs(g3[:, 0:1]) * Dp[:, :, 0] + np.abs(g3[:, 1:2]) * Dp[:, :, 1]
              + np.abs(g3[:, 2:3]) * Dp[:, :, 3])
        snap = np.abs(C[:, :, 3]) * SNAP                                         # the snap (1/512 px) in clip x: |w| / (256 W)
        ddet = np.abs(det) * (np.einsum("tjc,tjc->t", np.abs(Q), Ee) + np.einsum("tjr,trj->t", np.abs(Minv), Dxyw)
                              + np.einsum("tj,tj->t", np.abs(Minv[:, :, 0]), snap / W) + np.einsum("tj,tj->t", np.abs(Minv[:, :, 1]), snap / H))
    return {"M": M, "det": det, "ok": ok, "Minv": Minv, "L": L, "cz": cz, "g3": g3, "ddet": ddet,
            "dsnap": np.abs(g3[:, 0:1]) * snap / W + np.abs(g3[:, 1:2]) * snap / H}


def _fragments(C, S, W, H, shadow, slope, tri_ok, facing_unsure, control=None):
    """All fragments - certain and uncertain - of the triangles `tri_ok` of C (clip, (T, 3, 4)); S = _setup(...).
    -> dict of flat arrays: pix, z (biased and clamped in the shadow pass), tol, certain, tri; in the shadow pass also z_old, tol_old,
    certain_old (the rule that excused every depth-clipped caster), certain_plain (those casters certain, with the old bias) and clipped
    (the fragment's caster is clipped in depth)"""
    Minv, L, cz, g3 = S["Minv"], S["L"], S["cz"], S["g3"]
    Z = C[:, :, 2]
    w = C[:, :, 3]
    big = float(max(W, H))
    out = {k: [] for k in ("pix", "z", "tol", "certain", "tri", "z_old", "tol_old", "certain_old", "certain_plain", "clipped")}
    ok = tri_ok.copy()
    with np.errstate(all="ignore"):
        # clipping: in depth (0 <= z <= w, w > 0), in x / y, and beyond the guard band
        depth_clipped = np.any((w <= 0) | (Z < 0) | (Z > w), axis=1)
        xy_clipped = np.any((np.abs(C[:, :, 0]) > w) | (np.abs(C[:, :, 1]) > w), axis=1)
        guard_clipped = np.any((np.abs(C[:, :, 0]) > GUARD * w) | (np.abs(C[:, :, 1]) > GUARD * w), axis=1)
        # a re-snapped intersection: 1/256 px, plus float32 arithmetic on a position up to GUARD max(W, H) px from the centre
        tau_clip = np.where(depth_clipped | guard_clipped, SNAP + (K_EYE + K_PROJ) * U * GUARD * big, 0.0)
        # the screen box: exact for triangles in front of the eye, the whole viewport for the others
        front = np.all(w > 0, axis=1)
        sx = np.where(front[:, None], (C[:, :, 0] / np.where(front[:, None], w, 1.0) + 1.0) * W / 2.0, 0.0)
        sy = np.where(front[:, None], (C[:, :, 1] / np.where(front[:, None], w, 1.0) + 1.0) * H / 2.0, 0.0)
        x0 = np.where(front, np.floor(sx.min(1)) - 1, 0).clip(0, W - 1).astype(np.int64)
        x1 = np.where(front, np.ceil(sx.max(1)) + 1, W - 1).clip(0, W - 1).astype(np.int64)
        y0 = np.where(front, np.floor(sy.min(1)) - 1, 0).clip(0, H - 1).astype(np.int64)
        y1 = np.where(front, np.ceil(sy.max(1)) + 1, H - 1).clip(0, H - 1).astype(np.int64)
        ok &= ~(front & ((sx.max(1) < -1) | (sx.min(1) > W + 1) | (sy.max(1) < -1) | (sy.min(1) > H + 1)))
        # the depth plane and the edge functions' gradients per pixel
        gx_px, gy_px = g3[:, 0] * 2.0 / W, g3[:, 1] * 2.0 / H
        gz = np.hypot(gx_px, gy_px)
        g = np.hypot(Minv[:, :, 0] * 2.0 / W, Minv[:, :, 1] * 2.0 / H)           # |grad lambda_k| per pixel
        if shadow:
            # r: the largest exponent of the vertex depths; m and its error on the unclipped plane
            zmax = np.max(np.abs(Z / np.where(w != 0, w, 1.0)), axis=1)
            e = np.frexp(np.where(zmax > 0, zmax, 1.0))[1] - 1                    # zmax = 1.f * 2^e
            r = np.where(zmax > 0, np.ldexp(1.0, e - 23), 0.0)
            m = np.maximum(np.abs(gx_px), np.abs(gy_px))
            # the slope's own error: the plane's coefficients move by sum_j (dz_j) Minv[j, :] (see _setup), the snap included
            dm = np.maximum(np.einsum("tj,tj->t", np.abs(Minv[:, :, 0]), cz + S["dsnap"]) * 2.0 / W,
                            np.einsum("tj,tj->t", np.abs(Minv[:, :, 1]), cz + S["dsnap"]) * 2.0 / H)
            bias = slope * m + 1.25 * r
            # 0.5 r: a float32 vertex depth may round across a power of two; an x / y clipped primitive has vertex depths between the
            # unclipped ones, so its r lies in [0, r]
            bias_tol = slope * dm + 0.5 * r + np.where(xy_clipped, 1.25 * r, 0.0)
            # the rule this statement had before: a depth-clipped caster excused outright (kept to report what it excused)
            bias_old, bias_tol_old = bias.copy(), bias_tol.copy()
            # a depth-clipped caster: r of the clipped polygon and m of the plane, with the fan's error (_clipped_bias)
            unbounded = np.zeros(len(C), dtype=bool)
            for t in np.nonzero(depth_clipped & ok)[0]:
                r_hi, dm_clip = _clipped_bias(C[t], gz[t], W, H, control)
                unbounded[t] = not np.isfinite(dm_clip)
                bias[t] = slope * m[t] + 0.625 * r_hi                             # any r in [0, r_hi]
                bias_tol[t] = slope * (dm[t] + dm_clip) + 0.625 * r_hi
                if control == "clipped_unbiased":
                    bias[t] = 0.0
                elif control == "far_vertex_r" and np.any(Z[t] > w[t]):
                    bias[t] = slope * m[t] + 1.25 * r[t]
                    bias_tol[t] = slope * (dm[t] + dm_clip) + 0.5 * r[t]
        z_lo = -1.0 if control == "gl_near" else 0.0                              # the clip volume's z_m
    for t_sel, x0s, y0s, gw, gh in _boxes(np.nonzero(ok)[0], x0, x1, y0, y1):
        gxs, gys = np.meshgrid(np.arange(gw), np.arange(gh))
        ix = x0s[:, None] + gxs.reshape(1, -1)
        iy = y0s[:, None] + gys.reshape(1, -1)
        valid = (ix <= x1[t_sel, None]) & (iy <= y1[t_sel, None])
        X = (ix + 0.5) * 2.0 / W - 1.0
        Y = (iy + 0.5) * 2.0 / H - 1.0
        Mi = Minv[t_sel]
        with np.errstate(all="ignore"):
            lam = Mi[:, :, 0, None] * X[:, None, :] + Mi[:, :, 1, None] * Y[:, None, :] + Mi[:, :, 2, None]        # (n, 3, P)
            alam = np.abs(lam)
            dlam = np.matmul(L[t_sel], alam)
            gs = g[t_sel][:, :, None]
            s = lam / gs
            tau = SNAP + tau_clip[t_sel, None, None] + dlam / gs
            pos = lam.sum(1) > 0
            inside = np.all(lam >= 0, axis=1) & pos
            near = np.all(s >= -tau, axis=1) & np.any(s <= tau, axis=1) & pos
            z = np.einsum("tkp,tk->tp", lam, Z[t_sel])
            tol = (gz[t_sel, None] * (SNAP + tau_clip[t_sel, None])
                   + np.einsum("tkp,tk->tp", alam, cz[t_sel])
                   + K_PLANE * U * (np.abs(z) + gz[t_sel, None] * GUARD * big))
            cand = (inside | near) & valid & (z > z_lo - tol) & (z < 1.0 + tol)
            certain = inside & ~near & (z >= z_lo + tol) & (z <= 1.0 - tol) & ~facing_unsure[t_sel, None]
            if shadow:
                z_raw = z
                z = np.clip(z_raw + bias[t_sel, None], 0.0, 1.0)
                z_old = np.clip(z_raw + bias_old[t_sel, None], 0.0, 1.0)
                tol_old = tol + bias_tol_old[t_sel, None]
                tol = tol + bias_tol[t_sel, None]
                certain_plain = certain
                certain_old = certain & ~depth_clipped[t_sel, None]
                certain = certain & ~unbounded[t_sel, None]
        tt, pp = np.nonzero(cand)
        out["pix"].append(iy[tt, pp] * W + ix[tt, pp])
        out["z"].append(z[tt, pp])
        out["tol"].append(tol[tt, pp])
        out["certain"].append(certain[tt, pp])
        out["tri"].append(t_sel[tt])
        if shadow:
            clipped = np.broadcast_to(depth_clipped[t_sel, None], cand.shape)
            for k, v in (("z_old", z_old), ("tol_old", tol_old), ("certain_old", certain_old), ("certain_plain", certain_plain),
                         ("clipped", clipped)):
                out[k].append(v[tt, pp])
    return {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in out.items()}


def _ndc_lerp(C, Ee, Dp, ids):
    """control "ndc_lerp": every depth-clipped triangle replaced by the pieces _ndc_pieces makes of it (their error: the projection's
    rounding of an NDC coordinate)"""
    with np.errstate(all="ignore"):
        clipped = np.any((C[:, :, 3] <= 0) | (C[:, :, 2] < 0) | (C[:, :, 2] > C[:, :, 3]), axis=1)
    keep = np.nonzero(~clipped)[0]
    extra = [(p, t) for t in np.nonzero(clipped)[0] for p in _ndc_pieces(C[t])]
    if not extra:
        return C[keep], Ee[keep], Dp[keep], ids[keep]
    P = np.array([p for p, _ in extra])
    src = np.array([t for _, t in extra])
    return (np.concatenate([C[keep], P]), np.concatenate([Ee[keep], np.zeros((len(P), 3, 3))]),
            np.concatenate([Dp[keep], K_PROJ * U * np.abs(P)]), np.concatenate([ids[keep], ids[src]]))


def _boxes(tris, x0, x1, y0, y1, budget=1 << 19):
    """groups of triangles evaluated on one grid: small boxes bucketed by power-of-two size, large ones alone in strips of rows
    -> (triangle indices, x origins, y origins, grid width, grid height)"""
    bw, bh = x1[tris] - x0[tris] + 1, y1[tris] - y0[tris] + 1
    pw = 1 << np.ceil(np.log2(np.maximum(bw, 1))).astype(np.int64)
    ph = 1 << np.ceil(np.log2(np.maximum(bh, 1))).astype(np.int64)
    small = pw * ph <= 4096
    for kw, kh in set(zip(pw[small].tolist(), ph[small].tolist())):
        sel = tris[small & (pw == kw) & (ph == kh)]
        step = max(1, budget // (kw * kh))
        for i in range(0, len(sel), step):
            t = sel[i:i + step]
            yield t, x0[t], y0[t], int(kw), int(kh)
    for t in tris[~small]:
        w_ = int(x1[t] - x0[t] + 1)
        rows = max(1, budget // w_)
        for ys in range(int(y0[t]), int(y1[t]) + 1, rows):
            yield np.array([t]), np.array([x0[t]]), np.array([ys]), w_, min(rows, int(y1[t]) - ys + 1)


SHADOW_CONTROLS = ("gl_near", "clipped_unbiased", "ndc_lerp", "far_vertex_r")


def raster(draws, ubo, W, H, shadow=False, slope=7.5, depth_op="less", cull="back", start=None, control=None):
    """Rasterise the whole frame in float64.

    draws: independent_scenes.Scene.draws(); ubo: frame_uniforms(...)["cam"] or ["shadow"] (W = H = the map size for the shadow pass)
    slope / depth_op / cull: the statement's depth-bias slope factor, the camera pass's compare op ("less" or "less_equal") and cull mode
    ("back" or "front"); anything but 7.5 / "less" / "back" is a deliberately wrong statement for the negative controls.
    start: None (the depth clear 1.0), or a depth buffer the draws are tested against and written over, as a later pass of the same
    render pass sees it (the skydome against the copied deferred depth): {"depth", "tol", "ambiguous"} (H, W), e.g. an earlier raster().
    Its values act as fragments drawn before every primitive (they keep a tie under LESS), and its ambiguous pixels stay ambiguous;
    "prim" is 0xFFFFFFFF and "covered" False where such a value still wins.
    control: None, or one of SHADOW_CONTROLS - a deliberately wrong reading of clipping for the negative controls (shadow pass).
    -> {"depth": (H, W) the winner's depth (camera) or the biased map value (shadow), 1.0 where nothing is drawn,
        "tol": (H, W) its tolerance, "prim": (H, W) winning primitive id, 0xFFFFFFFF for none (camera pass),
        "covered": (H, W), "ambiguous": (H, W) bool; shadow pass also "ambiguous_old" (the mask of the rule that excused every
        depth-clipped caster) and "clip_excused" (what that rule excused only because the caster was clipped)}
    """
    C, Ee, Dp, ids = _triangles(draws, ubo)
    if control == "ndc_lerp":
        C, Ee, Dp, ids = _ndc_lerp(C, Ee, Dp, ids)
    T = len(C)
    S = _setup(C, Ee, Dp, ubo["Proj"], W, H)
    det, ddet, ok = S["det"], S["ddet"], S["ok"].copy()
    # facing: sign(det) is the orientation of the visible part in NDC, and the viewport keeps it; Vulkan's
    # a = -1/2 sum(x_i y_i+1 - x_i+1 y_i) > 0 (COUNTER_CLOCKWISE front) is det < 0.  ddet: the first-order error of det,
    # det tr(Minv dM), with the snap (see _setup)
    facing_unsure = np.zeros(T, dtype=bool)
    if not shadow:
        facing_unsure = ok & (np.abs(det) <= ddet)
        ok &= ((det > 0) if cull == "front" else (det < 0)) | facing_unsure
        # an exact repeat of an earlier triangle (same clip coordinates: the same float32 inputs through the same matrices) ties
        # EXACTLY in any arithmetic: under LESS it never wins and adds no doubt; under LESS_OR_EQUAL the last repeat wins
        if T:
            _, first = np.unique(C.reshape(T, 12), axis=0, return_index=True)
            _, last = np.unique(C[::-1].reshape(T, 12), axis=0, return_index=True)
            keep = np.zeros(T, dtype=bool)
            keep[first if depth_op == "less" else T - 1 - last] = True
            ok &= keep
    f = _fragments(C, S, W, H, shadow, slope, ok, facing_unsure, control)
    n = W * H
    pix = f["pix"].astype(np.int64)
    prim = ids[f["tri"].astype(np.int64)] if len(pix) else np.zeros(0, dtype=np.int64)
    certain = f["certain"].astype(bool)
    compete = certain & f["clipped"].astype(bool) if shadow else None
    out = _resolve(n, pix, f["z"], f["tol"], certain, prim, shadow, depth_op, start, compete)
    if shadow:
        # the rule before (every depth-clipped caster excused), and the same casters certain under it: what clipping alone excused
        old = _resolve(n, pix, f["z_old"], f["tol_old"], f["certain_old"].astype(bool), prim, shadow, depth_op, start)
        plain = _resolve(n, pix, f["z_old"], f["tol_old"], f["certain_plain"].astype(bool), prim, shadow, depth_op, start)
        out["ambiguous_old"] = old["ambiguous"]
        out["clip_excused"] = old["ambiguous"] & ~plain["ambiguous"]
    return {k: v.reshape(H, W) if k != "prim" else v.reshape(H, W).astype(np.uint32) for k, v in out.items()}


def _resolve(n, pix, z, tol, certain, prim, shadow, depth_op, start, compete=None):
    """the fragments' depth test: the nearest certain fragment per pixel and the ambiguity mask (see raster).  compete: certain
    fragments whose lowest value counts as an uncertain fragment's does (the shadow pass's depth-clipped casters)"""
    if start is not None:
        # the starting depth buffer as certain fragments with primitive id -1: first in draw order, so they keep a tie under LESS
        d0 = np.asarray(start["depth"], dtype=F64).reshape(-1)
        s_pix = np.nonzero(d0 < 1.0)[0]
        pix = np.concatenate([pix, s_pix])
        z = np.concatenate([z, d0[s_pix]])
        tol = np.concatenate([tol, np.asarray(start["tol"], dtype=F64).reshape(-1)[s_pix]])
        certain = np.concatenate([certain, np.ones(len(s_pix), dtype=bool)])
        prim = np.concatenate([prim, np.full(len(s_pix), -1, dtype=np.int64)])
    # the nearest certain fragment per pixel (ties: the first drawn under LESS, the last under LESS_OR_EQUAL)
    c = np.nonzero(certain)[0]
    order = c[np.lexsort((prim[c] if depth_op == "less" else -prim[c], z[c], pix[c]))]
    depth, dtol = np.ones(n), np.zeros(n)
    win = np.full(n, 0xFFFFFFFF, dtype=np.int64)
    covered = np.zeros(n, dtype=bool)
    amb = np.zeros(n, dtype=bool)
    if len(order):
        p_sorted = pix[order]
        head = np.r_[True, p_sorted[1:] != p_sorted[:-1]]
        first = order[head]
        depth[pix[first]], dtol[pix[first]], win[pix[first]] = z[first], tol[first], prim[first]
        covered[pix[first]] = True
        if not shadow:
            # the second-nearest certain fragment could overtake the nearest
            s2 = order[np.r_[False, ~head[1:] & head[:-1]]]
            close = z[s2] - tol[s2] <= depth[pix[s2]] + dtol[pix[s2]]
            amb[pix[s2[close]]] = True
    # an uncertain fragment could come in front of (or, in the shadow pass, below the tolerance of) what the certain ones give; in the
    # shadow pass the map holds the least of the fragments' values, so a certain fragment of a depth-clipped caster (whose bias budget
    # can reach below the nearest one's tolerance) counts as well
    u = np.nonzero(~certain if compete is None else ~certain | compete)[0]
    if len(u):
        lowest = np.full(n, np.inf)
        np.minimum.at(lowest, pix[u], z[u] - tol[u])
        if shadow:
            amb |= lowest < depth - dtol
        else:
            amb |= lowest < depth + dtol
    if not shadow:
        covered &= depth < 1.0
    if start is not None:
        amb |= np.asarray(start["ambiguous"], dtype=bool).reshape(-1)
        covered &= win >= 0
        win[win < 0] = 0xFFFFFFFF
    return {"depth": depth, "tol": dtol, "prim": win, "covered": covered, "ambiguous": amb}


# ---------------------------------------------------------------------------------------------------------------- comparisons
# Used by tests/test_oracle_geometry.py (the oracle) and tests/test_gpu_independent.py (the HIP renderer): the same masks and
# tolerances for both.

# UNIFORM_ULPS: a float32 UpdateUniformBuffer lands within this many u of each row's magnitude: lookAt's entries carry <= 6u (see
# K_EYE), the products ViewProjSpace / ShadowmapSpace another 4u (a 4-term dot product), the rounding of each input 1u; 16u.
UNIFORM_ULPS = 16.0


def _rows_close(got, want, rows_of=lambda a: a):
    """|got - want| <= UNIFORM_ULPS u max|row of want| per row; a non-finite want (lookAt(0, 0), or up parallel to the view direction)
    must be non-finite in got as well"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)):
        return False
    if not fin.any():
        return True
    mag = np.max(np.abs(np.where(fin, want, 0.0)), axis=-1, keepdims=True)
    return bool(np.all(np.abs(np.where(fin, got - want, 0.0)) <= UNIFORM_ULPS * U * mag))


def check_uniforms(frame, fu, dir_lights, point_lights):
    """frame: (cam, shadow, view) records as zo_get_frame / zr_get_frame return them; fu: frame_uniforms(...) -> list of what differs"""
    cam, sh, view = frame
    bad = []
    for which, rec in (("cam", cam), ("shadow", sh)):
        for k in ("Model", "View", "Proj"):
            if not _rows_close(mat(rec[k]), fu[which][k]):
                bad.append("%s.%s" % (which, k))
    v = fu["view"]
    for k in ("ViewProjSpace", "ShadowmapSpace", "LocalToWorld"):
        if not _rows_close(mat(view[k]), v[k]):
            bad.append(k)
    if not _rows_close(view["CameraInfo"], v["CameraInfo"]):
        bad.append("CameraInfo")
    for k in ("ViewportInfo", "LightsCount"):
        if not np.array_equal(np.asarray(view[k], dtype=F64), np.asarray(v[k], dtype=F64)):
            bad.append(k)
    for k in ("zNear", "zFar", "Time"):
        if F64(view[k]) != v[k]:
            bad.append(k)
    n_dir, n_point = len(dir_lights), len(point_lights)
    if n_dir and view["DirectionalLights"][:n_dir].tobytes() != np.asarray(dir_lights).tobytes():
        bad.append("DirectionalLights")
    if n_point:
        got = view["PointLights"][:n_point]
        if not _rows_close(got["Position"], v["PointPositions"]):
            bad.append("PointLights.Position")
        for k in ("Color", "Direction", "LightInfo"):
            if not np.array_equal(got[k], np.asarray(point_lights)[k]):
                bad.append("PointLights." + k)
    return bad


def check_camera(st, depth, vis=None):
    """the camera pass against raster(): depth (H, W) float32 as read back (1.0 where nothing was drawn), vis the visibility buffer
    when there is one.  -> dict: ambiguous fraction, coverage / winner / depth mismatches outside the mask, worst |error| / tolerance"""
    amb = st["ambiguous"]
    depth = np.asarray(depth, dtype=F64)
    got_cov = (vis != 0xFFFFFFFF) if vis is not None else depth < 1.0
    cov_bad = int(((got_cov != st["covered"]) & ~amb).sum())
    prim_bad = int(((vis != st["prim"]) & ~amb).sum()) if vis is not None else 0
    m = st["covered"] & ~amb
    err = np.abs(depth - st["depth"])
    depth_bad = int((err[m] > st["tol"][m]).sum())
    empty_bad = int((depth[~st["covered"] & ~amb] != 1.0).sum())       # the deferred pass's depth clear (ZE:3517)
    worst = float((err[m] / st["tol"][m]).max()) if m.any() else 0.0
    return {"ambiguous": float(amb.mean()), "coverage": cov_bad, "prim": prim_bad, "depth": depth_bad + empty_bad, "worst": worst,
            "ok": cov_bad == 0 and prim_bad == 0 and depth_bad == 0 and empty_bad == 0}


def check_shadow(st, smap):
    """the shadow map against raster(shadow=True): every texel outside the mask within its tolerance (the clear is 1.0), and the
    covered / clear mask identical wherever the statement's value is not within its tolerance of the clear"""
    amb = st["ambiguous"]
    smap = np.asarray(smap, dtype=F64)
    err = np.abs(smap - st["depth"])
    bad = int(((err > st["tol"]) & ~amb).sum())
    decided = ~amb & (np.abs(st["depth"] - 1.0) > st["tol"])
    mask_bad = int((((smap < 1.0) != (st["depth"] < 1.0)) & decided).sum())
    m = st["covered"] & ~amb
    worst = float((err[m] / st["tol"][m]).max()) if m.any() else 0.0
    return {"ambiguous": float(amb.mean()), "depth": bad, "coverage": mask_bad, "worst": worst, "ok": bad == 0 and mask_bad == 0}
