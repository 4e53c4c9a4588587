"""A second, independent statement of the skydome and background passes, in float64.

TEST INFRASTRUCTURE.  Written from the reference's text (ZE = Engine/ZeldaEngine/ZeldaEngine.cpp, SH = its Shaders/): SH/Skydome.vert,
SH/Skydome.frag, SH/Background.vert, SH/Background.frag, the two pipelines (ZE:2657-2744), their draws after the lighting quad
(ZE:3482-3506, 3681-3699), the UBO they bind (BaseUniformBuffers: the camera's, with the stage roll, ZE:4617-4629, 5600-5618) and
RHICreateTextureResource's sRGB default (ZE:5855) - and from the Vulkan 1.3 rasterisation and texturing chapters.  NOT from oracle/ or
the HIP kernels under zeldaengine_amd/csrc/, and it imports nothing from them.  The rasteriser is tests/independent_geometry.py's, the
samplers tests/independent_sampler.py's, the error budget of sampled values tests/independent_eval.py's.

What it states:

* `skydome`: the dome mesh through the camera UBO (Model included), cull BACK with front = COUNTER_CLOCKWISE, depth LESS against the
  deferred depth the render pass copied in, depth writes on; UV interpolated perspective-correctly from the ORIGINAL clip coordinates
  (clipping does not change the attribute of a point of the primitive), the 2x2 quad's differences with the helper lane extrapolating
  the same triangle, texture() of the sRGB image's mip chain (LINEAR, REPEAT, anisotropic), then pow(colour, 0.4545).
* `background`: the full-screen quad at z = 1 with LESS_OR_EQUAL: drawn where the depth the dome left is still >= 1.  Background.vert
  puts uv (0, 0) at NDC (-1, -1), which the unflipped viewport maps to the TOP-left pixel: uv = ((x + 1/2) / W, (y + 1/2) / H), and its
  derivatives are (1/W, 0) and (0, 1/H).  Then the same sampler and gamma.
* `compose`: the two passes draw into the swapchain image after the lighting quad, in debug view 0 only (ZE:3681-3699).

Where it cannot decide - derived, not tuned:

* coverage and depth: independent_geometry.raster's mask (the snap, the float32 vertex error, the clipper's re-snapped intersections),
  with the deferred depth entering as fragments of known tolerance: a dome fragment within the sum of the two tolerances of the deferred
  depth is excused, and so is a pixel the geometry statement itself excused.  A triangle the near or far plane cuts is NOT excused as a
  whole: only pixels within tau of its edges, the edge the clipper made included (there |z| or |z - w| is within the depth tolerance).
* the sampled value: independent_eval's budget (snap, float32 interpolation, the derivatives' relative error, Pmax / Pmin within that
  error of an integer).  For a clipped triangle the derivatives' error comes from the clipped polygon: its vertices are re-snapped, so
  the smallest altitude over every three of its vertices (any fan the clipper may emit) stands in for the triangle's.
* the background: pixels whose dome depth lies within its tolerance of 1.0 (the far plane cuts the dome there).
"""
import numpy as np

import independent_eval as ie
import independent_geometry as ig
import independent_sampler as isamp

F64 = np.float64
GAMMA = 0.4545

# Controls: deliberately wrong statements for the negative controls of tests/test_oracle_sky.py.
CONTROLS = ("dome_without_model", "cull_front", "sky_unorm", "bg_v_flipped", "bg_clamp", "bg_lod0", "no_gamma")


def _gamma(x, control):
    return x if control == "no_gamma" else np.power(np.maximum(x, 0.0), GAMMA)


def _gamma_range(val, span, control):
    """the span of pow(v, 0.4545) for v within val +- span (the float64 value's span over the error budget, per channel)"""
    lo, hi = _gamma(np.maximum(val - span, 0.0), control), _gamma(val + span, control)
    mid = _gamma(val, control)
    return mid, np.maximum(hi - mid, mid - lo)


def _perspective_weights(c3, px, py, W, H):
    """perspective-correct barycentrics of the pixel centres (px, py) on the triangles c3 (k, 3, 4) - from the original clip coordinates"""
    A = np.stack([c3[..., 0], c3[..., 1], c3[..., 3]], axis=1)
    with np.errstate(all="ignore"):
        Ainv = np.linalg.inv(A)
        u, v = (px + 0.5) / W * 2.0 - 1.0, (py + 0.5) / H * 2.0 - 1.0
        l = np.einsum("kij,kj->ki", Ainv, np.stack([u, v, np.ones_like(u)], axis=1))
        return l / l.sum(axis=1, keepdims=True)


def skydome(mesh, image8, ubo, start, W, H, control=None):
    """The skydome pass (Skydome.vert / Skydome.frag, ZE:3482-3506) over the deferred depth.

    mesh: (XkVertex array, uint32 indices); image8: the (h, w, 4) uint8 sky image; ubo: independent_geometry.frame_uniforms(...)["cam"];
    start: the deferred depth as independent_geometry.raster returns it (depth, tol, ambiguous); control: one of CONTROLS or None.
    -> dict over the (H, W) frame: "covered" (the dome wins), "colour" (H, W, 3) before the UNORM store, "tol" (H, W, 3) its span
    over the error budget, "ambiguous" (coverage, depth or tap count undecided), "depth" / "depth_tol" / "depth_ambiguous" the depth
    the dome leaves behind (what the background is tested against), "clipped" (the winning triangle was cut by the clipper), "ratio"
    (Pmax / Pmin of the footprint: N = min(ceil(ratio), 16) taps)
    """
    verts, idx = mesh
    if control == "dome_without_model":
        ubo = dict(ubo, Model=np.eye(4))
    draws = [{"verts": verts, "idx": idx, "instances": None, "prim_base": 0}]
    st = ig.raster(draws, ubo, W, H, cull="front" if control == "cull_front" else "back", start=start)
    out = {"ratio": np.zeros((H, W)), "covered": st["covered"].copy(), "colour": np.zeros((H, W, 3)), "tol": np.zeros((H, W, 3)), "ambiguous": st["ambiguous"].copy(),
           "depth": st["depth"], "depth_tol": st["tol"], "depth_ambiguous": st["ambiguous"].copy(), "clipped": np.zeros((H, W), bool)}
    ys, xs = np.nonzero(st["covered"])
    if not len(ys):
        return out
    clip = ie.vertex_stage(verts, None, ubo["Model"], ubo["View"], ubo["Proj"])[0]
    uv = np.asarray(verts["TexCoord"], dtype=F64)
    corner = np.asarray(idx, dtype=np.int64).reshape(-1, 3)[st["prim"][ys, xs].astype(np.int64)]
    c3 = clip[corner]
    px, py = xs.astype(F64), ys.astype(F64)
    sx, sy = np.where(xs & 1, 1.0, -1.0), np.where(ys & 1, 1.0, -1.0)
    at = lambda qx, qy: np.einsum("ki,kij->kj", _perspective_weights(c3, qx, qy, W, H), uv[corner])      # noqa: E731
    UV0 = at(px, py)
    st1, st2 = (UV0 - at(px - sx, py)) * sx[:, None], (UV0 - at(px, py - sy)) * sy[:, None]
    srgb = control != "sky_unorm"
    chain = isamp.mip_chain(image8, srgb)
    tris, inv = np.unique(corner, axis=0, return_inverse=True)
    alt, clipped = ie.altitudes(clip[tris], W, H)
    val, span, amb = ie._sampled_slot(chain, srgb, UV0, st1, st2, uv[corner], alt[inv.reshape(-1)], None)
    mid, tol = _gamma_range(val[:, :3], span[:, :3], control)
    out["colour"][ys, xs], out["tol"][ys, xs] = mid, tol
    out["ambiguous"][ys, xs] |= amb
    out["clipped"][ys, xs] = clipped[inv.reshape(-1)]
    out["ratio"] = np.zeros((H, W))
    out["ratio"][ys, xs] = isamp.aniso_parameters_array(chain[0].shape[1], chain[0].shape[0], np.hstack([st1, st2]), len(chain))[4]
    return out


def background(image8, after, W, H, control=None):
    """The background pass (Background.vert / Background.frag): the full-screen quad at z = 1 with LESS_OR_EQUAL over the depth the
    dome left (`after`: skydome()'s depth / depth_tol / depth_ambiguous, or a geometry raster when there is no dome).
    -> dict "drawn", "colour", "tol", "ambiguous" over the (H, W) frame"""
    depth, dtol = after.get("depth"), after.get("depth_tol", after.get("tol"))
    amb = np.asarray(after.get("depth_ambiguous", after.get("ambiguous")), dtype=bool).copy()
    drawn = depth >= 1.0
    amb |= (depth < 1.0) & (1.0 - depth <= dtol)            # a depth within its tolerance of the quad's 1.0
    ys, xs = np.nonzero(drawn | amb)
    out = {"drawn": drawn, "colour": np.zeros((H, W, 3)), "tol": np.zeros((H, W, 3)), "ambiguous": amb}
    if not len(ys):
        return out
    u, v = (xs + 0.5) / W, (ys + 0.5) / H
    if control == "bg_v_flipped":
        v = 1.0 - v
    UV0 = np.stack([u, v], axis=1)
    k = len(ys)
    st1, st2 = np.broadcast_to([1.0 / W, 0.0], (k, 2)).copy(), np.broadcast_to([0.0, 1.0 / H], (k, 2)).copy()
    chain = isamp.mip_chain(image8, True)
    quad_uv = np.broadcast_to(np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), (k, 3, 2))
    alt = np.full(k, min(W, H) / np.sqrt(2.0))              # the quad's triangles: half a W x H rectangle, vertices on the viewport's corners
    with np.errstate(all="ignore"):
        val, span, a = ie._sampled_slot(chain, True, UV0, st1, st2, quad_uv, alt, "clamp" if control == "bg_clamp" else None)
    if control == "bg_lod0":                                # the same budget, the value of level 0 alone
        val = isamp.sample_2d_array(chain[:1], True, UV0, np.zeros((k, 4)))[0]
    mid, tol = _gamma_range(val[:, :3], span[:, :3], control)
    out["colour"][ys, xs], out["tol"][ys, xs] = mid, tol
    out["ambiguous"][ys, xs] |= a
    return out


def compose(lit, sky, bg, debug_view):
    """What the swapchain image holds after the lighting quad (deferred or forward) and, in debug view 0 only, the two passes.
    lit: (H, W, 3) the quad's colour; sky / bg: skydome() / background() or None.
    -> colour (H, W, 3), tol (H, W, 3) (0 where the lit value stands: its own checks apply), overlay (H, W) bool, ambiguous (H, W)"""
    H, W = lit.shape[:2]
    colour, tol = np.array(lit, dtype=F64), np.zeros((H, W, 3))
    overlay, amb = np.zeros((H, W), bool), np.zeros((H, W), bool)
    if debug_view != 0:
        return colour, tol, overlay, amb
    if bg is not None:
        d = bg["drawn"]
        colour[d], tol[d] = bg["colour"][d], bg["tol"][d]
        overlay |= d
        amb |= bg["ambiguous"]
    if sky is not None:
        s = sky["covered"]
        colour[s], tol[s] = sky["colour"][s], sky["tol"][s]
        overlay |= s
        amb |= sky["ambiguous"]
    return colour, tol, overlay, amb


def check_overlay(codes, colour, tol, overlay, amb):
    """the drawn sky / background pixels against the statement: every unexcused channel within its span plus one code of the UNORM
    store, alpha 255.  codes: (H, W, 4) the frame.  -> dict ok, bad, worst (error / tolerance), excused (fraction of the overlay)"""
    m = overlay & ~amb
    err = np.abs(codes[..., :3].astype(F64) - np.clip(colour, 0.0, 1.0) * 255.0)
    lim = tol * 255.0 + 1.0
    r = (err / lim)[m]
    bad = int((r > 1.0).any(axis=-1).sum()) if r.size else 0
    return {"ok": bad == 0 and bool((codes[..., 3][m] == 255).all()), "bad": bad, "worst": float(r.max()) if r.size else 0.0,
            "excused": float((overlay & amb).sum() / max(1, (overlay | amb).sum())), "n": int(m.sum())}
