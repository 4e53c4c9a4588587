"""The HIP renderer held DIRECTLY to the independent float64 statements - never through the oracle.

Every other GPU test compares the renderer with oracle/ bit for bit; the oracle and the kernels share one author.  Here the renderer's
uniforms (zr_get_frame), depth plane (gbuffer(0)) and shadow map are compared with tests/independent_geometry.py under the same masks
and tolerances as the oracle in tests/test_oracle_geometry.py (the renderer has no visibility buffer: coverage plus depth), and the
float64 winner of every unambiguous pixel drives tests/independent_eval.py through BaseScene.frag and the lighting pass, so the whole
chain is checked without the oracle.  The shapes are where a tiled rasteriser goes wrong: sizes that are not multiples of the 32-pixel
tile, one tile row, the smallest frames, a large frame with a 2048-texel map; each once with every cull on and once with every cull off.
"""
import numpy as np
import pytest

import independent_eval as ie
import independent_geometry as ig
import independent_sky as isky
from independent_scenes import EDGE_SCENES, FACES, SCENES, SKY_SCENES, TEXTURED_SCENES, Case, Scene, _lights, _sun_at, case, sky_dome_noise, tex_packed
from independent_sky_checks import SKY_CAPS, VIEW_SCENES, check_frame, forward_surface, gbuffer_of, load, statement
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

CUBE_DIM = 4
NO_CULL = abi.FLAG_NO_HIZ | abi.FLAG_NO_FRUSTUM_CULL | abi.FLAG_NO_CONE_CULL


def _large(W=1280, H=720, SD=2048, n_boxes=2500):
    """a few thousand instances, a grazing sun and a 2048-texel map (37 000 triangles at the default size)"""
    s = Scene()
    s.add(scenes.grid_plane(30.0, 8, 0.0))
    s.add(scenes.box((0.5, 0.4, 0.6), (0.0, 0.0, 0.6)), None, scenes.generate_instances(n_boxes, 1.0, 12.0, 0.2, 0.6, seed=41))
    s.add(scenes.uv_sphere(12, 6, 0.6), None, scenes.generate_instances(60, 1.0, 10.0, 0.4, 1.0, seed=42))
    return Case(s, abi.make_camera((9.0, -7.0, 4.0), (0.0, 0.0, 0.3), fov=55.0), _sun_at(_lights(1, 16), 0.15, 0.4), 0.1, 0.3, W, H, SD)


def _ground_near(W=1280, H=720, SD=2048):
    """a 60-unit ground plane in 4 x 4 cells crossing the light's near plane (the camera's zNear 6.0005, the sun 6 away): the
    clipped casters held to their bias budget at full size (every such triangle is listed once per tile of its meshlet in the
    shadow pass's slow list, and so is every caster with an edge of 64 texels, as any prop this close to the light: the 32 triangles
    alone stay within its default capacity at 2048^2)"""
    s = Scene()
    s.add(scenes.grid_plane(60.0, 4, 0.0))
    return Case(s, abi.make_camera((6.5, -5.0, 4.5), (0.0, 0.0, 0.0), fov=55.0, znear=6.0005, zfar=60.0), _sun_at(_lights(1, 8), 1.3, 0.7, 6.0),
                0.0, 0.0, W, H, SD)


def _resized(name, W, H, SD):
    return lambda: case(name, W, H, SD)


SHAPES = {n: _resized(n, 192, 128, 256) for n in SCENES}
SHAPES.update(EDGE_SCENES)
SHAPES.update({"mixed_1000x37": _resized("mixed", 1000, 37, 256), "mixed_33x17": _resized("mixed", 33, 17, 64),
               "large_1280x720": _large, "ground_near_1280x720": _ground_near})
# the ambiguous fractions of these shapes (camera, shadow) as measured when the test was written, with headroom; the 192 x 128 scenes
# and the edge scenes share the caps of tests/test_oracle_geometry.py (the statement is the same)
EXTRA_CAPS = {"mixed_1000x37": (0.001, 0.001), "mixed_33x17": (0.03, 0.005), "large_1280x720": (0.009, 0.002), "history": (0.002, 0.001),
              "ground_near_1280x720": (0.001, 0.001)}

_statements = {}


def _statement(name):
    """(case, frame_uniforms, camera raster, shadow raster), computed once per shape for both flag sets"""
    if name not in _statements:
        c = SHAPES[name]()
        d, p, sp = c.lights
        fu = ig.frame_uniforms(c.cam, d, p, c.W, c.H, c.roll_stage, c.roll_light, sp, CUBE_DIM)
        draws = c.scene.draws()
        _statements[name] = (c, fu, ig.raster(draws, fu["cam"], c.W, c.H), ig.raster(draws, fu["shadow"], c.SD, c.SD, shadow=True))
    return _statements[name]


def _caps(name):
    if name in EXTRA_CAPS:
        return EXTRA_CAPS[name]
    from test_oracle_geometry import AMBIGUITY_CAPS
    return AMBIGUITY_CAPS[name]


def _ubo_record(ubo):
    rec = np.zeros((), dtype=abi.XkUniformBufferMVP)
    for k in ("Model", "View", "Proj"):
        rec[k] = ubo[k].T.reshape(16)             # column-major, as ie.mat() reads it
    return rec


def _within_one(a, b):
    return np.all(np.abs(a - b) <= 1, axis=-1)


def _check_chain(g, c, fu, st_cam, view):
    """BaseScene.frag from the float64 winner of every unambiguous covered pixel, then the lighting pass over the renderer's own
    GBuffer and shadow map: the thresholds of tests/test_oracle_independent.py, unchanged"""
    W, H = c.W, c.H
    prim = np.where(st_cam["covered"] & ~st_cam["ambiguous"], st_cam["prim"], np.uint32(0xFFFFFFFF)).astype(np.uint32)
    mine = ie.base_scene(c.scene.draws(), _ubo_record(fu["cam"]), prim, W, H)
    ys, xs = mine["yx"]
    if len(ys):
        got = {"scene_color": ie.unpack_rgba8(g.gbuffer(1))[ys, xs], "a": ie.unpack_a2r10g10b10(g.gbuffer(2))[ys, xs],
               "b": ie.unpack_rgba8(g.gbuffer(3))[ys, xs], "c": ie.unpack_rgba8(g.gbuffer(4))[ys, xs]}
        want = {"scene_color": ie.unorm(mine["scene_color"], 8), "b": ie.unorm(mine["b"], 8), "c": ie.unorm(mine["c"], 8),
                "a": np.concatenate([ie.unorm(mine["a"][:, :3], 10), ie.unorm(mine["a"][:, 3:], 2)], axis=1)}
        for k in ("scene_color", "b", "c"):
            assert np.array_equal(got[k], want[k]), "GBuffer %s: constant material slots must come out exactly" % k
        d_vals, d_codes = ie.unpack_rgba16f(g.gbuffer(5))
        mine_d = mine["d"].astype(np.float16).view(np.uint16)
        budget = np.hstack([mine["d_per_pixel"] / 256.0, np.zeros((len(ys), 1))])      # (as in test_oracle_independent.py)
        ok_d = np.all((np.abs(ie.f16_ordinal(d_codes[ys, xs]) - ie.f16_ordinal(mine_d)) <= 1) | (np.abs(d_vals[ys, xs] - mine["d"]) <= budget), axis=-1)
        ok_a = _within_one(got["a"], want["a"])
        assert ok_a.mean() >= 0.999, "normals (A2R10G10B10): only %.4f of %d pixels within one code" % (ok_a.mean(), len(ok_a))
        assert ok_d.mean() >= 0.999, "world position (fp16): only %.4f of %d pixels within one ulp" % (ok_d.mean(), len(ok_d))
    d_vals, _ = ie.unpack_rgba16f(g.gbuffer(5))
    gb = {"scene_color": ie.unpack_rgba8(g.gbuffer(1)) / 255.0, "b": ie.unpack_rgba8(g.gbuffer(3)) / 255.0, "c": ie.unpack_rgba8(g.gbuffer(4)) / 255.0,
          "a": ie.unpack_a2r10g10b10(g.gbuffer(2)) / np.array([1023.0, 1023.0, 1023.0, 3.0]), "d": d_vals}
    smap = g.shadowmap()
    want_rgb = ie.unorm(ie.lighting(gb, smap, view, FACES, W, H), 8)
    have = g.color().astype(np.int64)
    ok = _within_one(have[..., :3], want_rgb)
    lo_hi = [ie.unorm(ie.lighting(gb, smap, view, FACES, W, H, pcf_eps=e), 8) for e in (-4e-7, 4e-7)]        # the PCF ties
    lo, hi = np.minimum(np.minimum(lo_hi[0], lo_hi[1]), want_rgb) - 1, np.maximum(np.maximum(lo_hi[0], lo_hi[1]), want_rgb) + 1
    on_edge = (lo_hi[0] != lo_hi[1]).any(axis=-1)
    ok = ok | (on_edge & np.all((have[..., :3] >= lo) & (have[..., :3] <= hi), axis=-1))
    assert on_edge.mean() < 0.1
    assert (have[..., 3] == 255).all()
    assert ok.mean() >= 0.999, "lit colour: only %.4f of the pixels within one LSB (worst %d)" % (ok.mean(), np.abs(have[..., :3] - want_rgb).max())
    return len(ys)


def _check_frame(g, name, c, fu, st_cam, st_sh, flags):
    d, p, _ = c.lights
    frame = g.get_frame()
    bad = ig.check_uniforms(frame, fu, d, p)
    assert not bad, "%s: zr_get_frame differs from UpdateUniformBuffer's: %s" % (name, bad)
    rc = ig.check_camera(st_cam, g.gbuffer(0))
    rs = ig.check_shadow(st_sh, g.shadowmap())
    print("%s flags %d %dx%d map %d: camera ambiguous %.4f worst depth %.3f tol | shadow ambiguous %.4f worst depth %.3f tol" % (
        name, flags, c.W, c.H, c.SD, rc["ambiguous"], rc["worst"], rs["ambiguous"], rs["worst"]))
    assert rc["ok"], "%s camera pass: %r" % (name, rc)
    assert rs["ok"], "%s shadow map: %r" % (name, rs)
    cap_cam, cap_sh = _caps(name)
    assert rc["ambiguous"] <= cap_cam and rs["ambiguous"] <= cap_sh, (name, rc["ambiguous"], rs["ambiguous"])
    if name == "sun_at_zenith":
        assert (g.shadowmap() == 1.0).all()
    return _check_chain(g, c, fu, st_cam, frame[2])


@pytest.mark.parametrize("flags", [0, NO_CULL], ids=["culled", "no_cull"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_renderer_against_the_independent_statements(gpu_engine, name, flags):
    c, fu, st_cam, st_sh = _statement(name)
    g = gpu_engine.Renderer(c.W, c.H, c.SD, flags=flags)
    try:
        c.scene.load(g)
        d, p, sp = c.lights
        g.update_uniforms(c.cam, d, p, sp, c.roll_stage, c.roll_light, 0.0)
        g.render()
        g.finish()
        n = _check_frame(g, name, c, fu, st_cam, st_sh, flags)
        if c.W * c.H >= 1000:
            assert n > 0.3 * (st_cam["covered"].sum())
    finally:
        g.close()


def _occluded(W=320, H=180, SD=512):
    """a wall in front of 40 spheres: the spheres behind it are what Hi-Z culls"""
    s = Scene()
    s.add(scenes.grid_plane(20.0, 4, 0.0))
    s.add(scenes.box((0.4, 3.0, 1.4), (1.5, 0.0, 1.4)))
    s.add(scenes.uv_sphere(12, 6, 0.6), None, scenes.generate_instances(40, 1.0, 3.0, 0.6, 1.0, seed=43))
    return Case(s, abi.make_camera((7.0, 0.5, 1.6), (0.0, 0.0, 0.8)), _lights(1, 8), 0.0, 0.0, W, H, SD)


def test_second_frame_with_hiz_history_against_the_statements(gpu_engine):
    """two frames with the camera moved in between: the second is culled against the first frame's Hi-Z, and must still be the
    statement's frame (culling conservative against the independent statement, not only against itself).  Props are spheres of
    some size: with hundreds of boxes a few pixels wide (the large shape at 320 x 180), the normal check of the whole chain sits at
    0.9989 for the oracle and the renderer alike (the 1/256-pixel snap moves the quad derivatives of such triangles by a code, and
    that check carries no snap budget)"""
    c0 = _occluded()
    cams = [c0.cam, abi.make_camera((7.0, -0.3, 1.8), (0.0, 0.2, 0.8))]
    d, p, sp = c0.lights
    g = gpu_engine.Renderer(c0.W, c0.H, c0.SD, flags=0)
    try:
        c0.scene.load(g)
        for cam in cams:
            g.update_uniforms(cam, d, p, sp, c0.roll_stage, c0.roll_light, 0.0)
            g.render()
        g.finish()
        c = c0._replace(cam=cams[1])
        fu = ig.frame_uniforms(c.cam, d, p, c.W, c.H, c.roll_stage, c.roll_light, sp, CUBE_DIM)
        draws = c.scene.draws()
        st_cam, st_sh = ig.raster(draws, fu["cam"], c.W, c.H), ig.raster(draws, fu["shadow"], c.SD, c.SD, shadow=True)
        _check_frame(g, "history", c, fu, st_cam, st_sh, 0)
        st = g.stats()
        print("history: Hi-Z culled %d meshlet-instances, %d in the geometry pass" % (st["hiz_culled"], st["hiz_culled_geom"]))
        assert st["hiz_culled"] + st["hiz_culled_geom"] > 0, "the second frame must have culled against the first frame's Hi-Z"
    finally:
        g.close()



# ---------------------------------------------------------------------------------------------------------------- sampled materials
# The textured scenes of tests/test_oracle_textured.py on the renderer, plus one at 1280 x 720: the packed-material form (seven slots of
# one size), the per-slot path (mixed sizes, non-powers of two, default and constant slots), the sampled resolve at odd frame sizes,
# and the sampled cubemap in both shading modes.  The geometry statement's winners drive base_scene(), which is held to the renderer's
# GBuffer within the derived tolerance; the lighting pass (deferred: over the renderer's GBuffer; forward: over the statement's own
# surface) to its frame at the thresholds of tests/test_oracle_textured.py.

TEXTURED_SHAPES = dict(TEXTURED_SCENES)
TEXTURED_SHAPES["tex_packed_1280x720"] = lambda: tex_packed(1280, 720, 2048)
TEXTURED_CAPS = {"tex_packed_1280x720": (0.067, 0.014)}        # measured 0.0441, 0.0091; headroom as in tests/test_oracle_textured.py
_textured = {}


def _textured_statement(name):
    """(case, frame_uniforms, camera raster, shadow raster, base_scene over the unambiguous winners), once per shape"""
    if name not in _textured:
        c = TEXTURED_SHAPES[name]()
        d, p, sp = c.lights
        fu = ig.frame_uniforms(c.cam, d, p, c.W, c.H, c.roll_stage, c.roll_light, sp, c.scene.cube[0].shape[0])
        draws = c.scene.draws()
        st_cam = ig.raster(draws, fu["cam"], c.W, c.H)
        prim = np.where(st_cam["covered"] & ~st_cam["ambiguous"], st_cam["prim"], np.uint32(0xFFFFFFFF)).astype(np.uint32)
        mine = ie.base_scene(draws, _ubo_record(fu["cam"]), prim, c.W, c.H)
        _textured[name] = (c, fu, st_cam, ig.raster(draws, fu["shadow"], c.SD, c.SD, shadow=True), mine)
    return _textured[name]


@pytest.mark.parametrize("forward", [False, True], ids=["deferred", "forward"])
@pytest.mark.parametrize("flags", [0, NO_CULL], ids=["culled", "no_cull"])
@pytest.mark.parametrize("name", list(TEXTURED_SHAPES))
def test_renderer_textured_against_the_independent_statements(gpu_engine, name, flags, forward):
    from test_oracle_textured import AMBIGUITY_CAPS as TEX_CAPS, check_lit, check_scene_pass, gbuffer_codes, _R
    c, fu, st_cam, st_sh, mine = _textured_statement(name)
    cap_s, cap_c = TEXTURED_CAPS.get(name) or TEX_CAPS[name]
    W, H = c.W, c.H
    g = gpu_engine.Renderer(W, H, c.SD, flags=flags)
    try:
        c.scene.load(g)
        d, p, sp = c.lights
        g.update_uniforms(c.cam, d, p, sp, c.roll_stage, c.roll_light, 0.0)
        g.set_shading(forward)
        g.render()
        g.finish()
        frame = g.get_frame()
        bad = ig.check_uniforms(frame, fu, d, p)
        assert not bad, "%s: zr_get_frame differs from UpdateUniformBuffer's: %s" % (name, bad)
        rc, rs_ = ig.check_camera(st_cam, g.gbuffer(0)), ig.check_shadow(st_sh, g.shadowmap())
        assert rc["ok"] and rs_["ok"], (name, rc, rs_)
        ys, xs = mine["yx"]
        assert len(ys) > 0.3 * st_cam["covered"].sum()
        view, cube, smap = frame[2], c.scene.cube_statement(), g.shadowmap()
        have = g.color().astype(np.int64)
        assert (have[..., 3] == 255).all()
        if not forward:
            r = check_scene_pass(mine, gbuffer_codes(g, ys, xs))
            d_vals, _ = ie.unpack_rgba16f(g.gbuffer(5))
            gb = {"scene_color": ie.unpack_rgba8(g.gbuffer(1)) / 255.0, "b": ie.unpack_rgba8(g.gbuffer(3)) / 255.0, "c": ie.unpack_rgba8(g.gbuffer(4)) / 255.0,
                  "a": ie.unpack_a2r10g10b10(g.gbuffer(2)) / np.array([1023.0, 1023.0, 1023.0, 3.0]), "d": d_vals}
            shade = lambda eps, off: ie.unorm(ie.lighting(gb, smap, view, cube, W, H, pcf_eps=eps), 8)      # noqa: E731
            frac, cube_amb, on_edge = check_lit(have, shade, _R(gb, smap, view, cube, c))
            print("%s flags %d %dx%d deferred: %d pixels from the statement's winners, sampled ambiguous %.4f worst %.3f tol, normals %.5f | "
                  "lit %.5f, cube boundary %.4f, PCF on edge %.4f" % (name, flags, W, H, len(ys), r["ambiguous"], r["worst"], r["normals"], frac, cube_amb, on_edge))
            assert r["ok"], "%s: %d sampled GBuffer values outside the derived tolerance (worst %.3f x)" % (name, r["bad"], r["worst"])
            assert r["normals"] >= 0.999 and r["ambiguous"] <= cap_s, (name, r)
        else:
            gb = {k: np.zeros((H, W, 4)) for k in ("scene_color", "a", "b", "c", "d")}
            for k in ("scene_color", "b", "c", "d"):
                gb[k][ys, xs] = mine[k]
            gb["a"][ys, xs, :3] = (mine["normal"] + 1.0) / 2.0
            unexcused = np.zeros((H, W), bool)
            unexcused[ys[~mine["ambiguous"]], xs[~mine["ambiguous"]]] = True
            shade = lambda eps, off: ie.unorm(ie.lighting(gb, smap, view, cube, W, H, pcf_eps=eps, forward=True, r_offset=off), 8)      # noqa: E731
            frac, cube_amb, on_edge = check_lit(have, shade, _R(gb, smap, view, cube, c, True), unexcused, r_spread=True)
            print("%s flags %d %dx%d forward: lit %.5f of %d pixels from the statement's winners, cube boundary %.4f, PCF on edge %.4f" % (
                name, flags, W, H, frac, unexcused.sum(), cube_amb, on_edge))
        assert on_edge < 0.1 and cube_amb <= cap_c, (name, on_edge, cube_amb)
        assert frac >= 0.999, "%s lit colour: only %.4f of the pixels within one LSB" % (name, frac)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------- skydome, background, debug views
# The scenes of tests/test_oracle_sky.py on the renderer, plus the dome at 1280 x 720: k_sky_tiles and the background in view 0, the view
# switch of k_lighting / k_forward and k_gbuffer_vis in views 1-10, held to tests/independent_sky.py and independent_eval's switch from
# the geometry statement's winners and depth - never through the oracle.  With every cull on and every cull off, deferred and forward;
# then the rank contexts of a 3-rank tile partition (k_sky_tiles walks the rank's owned tiles), and a queued sequence that toggles the
# dome and the background across frames in flight (the overlay plane is kept per GBuffer parity).

SKY_SHAPES = dict(SKY_SCENES)
SKY_SHAPES["sky_dome_1280x720"] = lambda: sky_dome_noise(1280, 720)
SKY_GPU_CAPS = {"sky_dome_1280x720": 0.048}        # measured 0.0318; headroom as in independent_sky_checks.SKY_CAPS


def _sky_render(gpu_engine, c, flags, forward, views):
    """-> {view: (H, W, 4) codes}, the renderer's GBuffer dict (deferred) or None, its shadow map and XkView, the uniforms check"""
    k = c.case
    g = gpu_engine.Renderer(k.W, k.H, k.SD, flags=flags)
    try:
        load(g, c, forward)
        out = {}
        for v in views:
            g.render(v)
            g.finish()
            out[v] = g.color().astype(np.int64).copy()
        return out, (None if forward else gbuffer_of(g)), g.shadowmap().copy(), g.get_frame(), g.gbuffer(0).copy()
    finally:
        g.close()


@pytest.mark.parametrize("forward", [False, True], ids=["deferred", "forward"])
@pytest.mark.parametrize("flags", [0, NO_CULL], ids=["culled", "no_cull"])
@pytest.mark.parametrize("name", list(SKY_SHAPES))
def test_renderer_sky_and_views_against_the_independent_statements(gpu_engine, name, flags, forward):
    c = SKY_SHAPES[name]()
    k = c.case
    fu, st, sky, bg = statement(name, c)
    views = list(range(11)) if name in VIEW_SCENES else [0]
    frames, gb, smap, frame, depth = _sky_render(gpu_engine, c, flags, forward, views)
    d, p, _sp = k.lights
    if not any(c.bars):
        bad = ig.check_uniforms(frame, fu, d, p)
        assert not bad, "%s: zr_get_frame differs from UpdateUniformBuffer's: %s" % (name, bad)
    rc = ig.check_camera(st, depth)
    assert rc["ok"], (name, rc)
    view = frame[2]
    covered = excused = None
    if forward:
        prim = np.where(st["covered"] & ~st["ambiguous"], st["prim"], np.uint32(0xFFFFFFFF)).astype(np.uint32)
        gb, excused = forward_surface(c, prim, _ubo_record(fu["cam"]))
        covered, excused = st["covered"], excused | st["ambiguous"]
    for v in views:
        r = check_frame(frames[v], c, gb, smap, view, v, forward, sky, bg, covered, excused, aniso=False)
        print(name, "flags", flags, "forward" if forward else "deferred", "view", v, {key: r[key] for key in r if key != "ok"})
        assert r["ok"], (name, v, r)
        if v == 0:
            assert r["sky_excused"] <= SKY_GPU_CAPS.get(name, SKY_CAPS.get(name, 0.0)), (name, r["sky_excused"])


@pytest.mark.parametrize("forward", [False, True], ids=["deferred", "forward"])
def test_renderer_sky_on_tile_partitioned_ranks(gpu_engine, forward):
    """three rank contexts of a tile partition: each rank's packed tiles, assembled, hold the dome and the background of the statement"""
    from zeldaengine_amd import dist as zdist
    name = "sky_dome_257x131"
    c = SKY_SHAPES[name]()
    k = c.case
    _fu, _st, sky, bg = statement(name, c)
    tiles = []
    for r in range(3):
        g = gpu_engine.Renderer(k.W, k.H, k.SD, tile_rank=r, tile_world=3)
        try:
            load(g, c, forward)
            g.render()
            g.render()
            g.finish()
            tiles.append(np.asarray(g.read_tiles()).copy())
        finally:
            g.close()
    have = zdist.untile(np.stack(tiles), k.W, k.H).astype(np.int64)
    colour, tol, overlay, amb = isky.compose(np.zeros((k.H, k.W, 3)), sky, bg, 0)
    r = isky.check_overlay(have, colour, tol, overlay, amb)
    print(name, "3 ranks", "forward" if forward else "deferred", r)
    assert r["ok"] and r["n"] > 0.4 * k.W * k.H, r


def test_queued_frames_toggle_the_dome_and_the_background(gpu_engine):
    """frames enqueued back to back, each copied out on the device in stream order, while the dome and the background are switched on
    and off: every frame's sky / background pixels against the statement of ITS flags, and every other pixel the lit frame"""
    import torch
    name = "sky_dome_noise"
    c = SKY_SHAPES[name]()
    k = c.case
    W, H = k.W, k.H
    _fu, st, sky, bg = statement(name, c)
    bg_alone = isky.background(c.background, st, W, H)
    flags_seq = [(1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (1, 1), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (0, 1)]
    g = gpu_engine.Renderer(W, H, k.SD)
    dev = torch.device("cuda", 0)
    col = [torch.zeros(W * H, dtype=torch.int32, device=dev) for _ in flags_seq]
    sha = [torch.zeros(k.SD * k.SD, dtype=torch.int32, device=dev) for _ in flags_seq]
    try:
        load(g, c)
        g.set_sky_flags(False, False)
        g.render()
        g.finish()
        lit = g.color().astype(np.int64).copy()
        torch.cuda.synchronize()
        for i, (s_on, b_on) in enumerate(flags_seq):
            g.set_sky_flags(bool(s_on), bool(b_on))
            g.render()
            g.copy_frame_async(col[i].data_ptr(), sha[i].data_ptr())
        g.finish()
    finally:
        g.close()
    for i, (s_on, b_on) in enumerate(flags_seq):
        have = col[i].cpu().numpy().view(np.uint8).reshape(H, W, 4).astype(np.int64)
        colour, tol, overlay, amb = isky.compose(np.zeros((H, W, 3)), sky if s_on else None, (bg if s_on else bg_alone) if b_on else None, 0)
        r = isky.check_overlay(have, colour, tol, overlay, amb)
        rest = ~overlay & ~amb
        stale = int((have[rest] != lit[rest]).any(axis=-1).sum())
        print("queued frame %d sky %d background %d:" % (i, s_on, b_on), r, "non-overlay pixels off the lit frame:", stale)
        assert r["ok"] and stale == 0, (i, s_on, b_on, r, stale)
        assert r["n"] > (0.3 * W * H if s_on or b_on else -1)
