"""What tests/test_oracle_sky.py (the oracle) and tests/test_gpu_independent.py (the HIP renderer) share to hold a frame with a skydome,
a background and the debug views to the independent statements: loading a sky scene, the statements of one scene (computed once and
cached), the GBuffer and forward-surface inputs of the lighting statement, and `check_frame`, which applies every assertion of those
tests to one frame.  TEST INFRASTRUCTURE; it imports nothing from oracle/ or csrc/.
"""
import numpy as np

import independent_eval as ie
import independent_geometry as ig
import independent_sky as isky
from independent_scenes import FACES, SKY_SCENES

CUBE_DIM = 4          # the scenes' cubemap: FACES, one colour per 4 x 4 face
# Caps on the excused fraction of the sky / background pixels (view 0), from the fractions measured when the test was written (printed
# below, quoted in DESIGN.md section 6) with headroom: the larger of 1.5 x and + 0.5 %, rounded up to 0.1 %.
SKY_CAPS = {"background_only": 0.007, "sky_dome_noise": 0.039, "sky_coarse_clipped": 0.015, "sky_rolled_npot": 0.008, "sky_pole": 0.015,
            "sky_dome_257x131": 0.031, "sky_coarse_33x17": 0.035, "sky_rolled_64x64": 0.008, "sky_bars_200x120": 0.038}
VIEW_SCENES = ["sky_dome_noise", "sky_rolled_64x64", "sky_bars_200x120"]
VIEWS = list(range(0, 11))


def load(r, c, forward=False):
    """the scene, the dome and the background into the oracle or the renderer (same method names), the frame's uniforms and bars"""
    k = c.case
    k.scene.load(r)
    if c.sky is not None:
        r.set_skydome(c.sky[0], c.sky[1], c.sky_image)
    if c.background is not None:
        r.set_background(c.background)
    d, p, sp = k.lights
    r.update_uniforms(k.cam, d, p, sp, k.roll_stage, k.roll_light, 0.0)
    if any(c.bars):
        cam, sh, view = r.get_frame()
        view["ViewportInfo"][2], view["ViewportInfo"][3] = c.bars
        r.set_frame(cam, sh, view)
    r.set_shading(forward)


_statements = {}


def statement(name, c=None, control=None):
    """(frame_uniforms, camera raster, skydome(), background()) - from the geometry statement alone; cached per scene and control"""
    key = (name, control)
    if key not in _statements:
        c = c or SKY_SCENES[name]()
        k = c.case
        d, p, sp = k.lights
        fu = ig.frame_uniforms(k.cam, d, p, k.W, k.H, k.roll_stage, k.roll_light, sp, CUBE_DIM)
        st = ig.raster(k.scene.draws(), fu["cam"], k.W, k.H)
        sky = isky.skydome(c.sky, c.sky_image, fu["cam"], st, k.W, k.H, control) if c.sky is not None else None
        bg = isky.background(c.background, sky or st, k.W, k.H, control) if c.background is not None else None
        _statements[key] = (fu, st, sky, bg)
    return _statements[key]


def gbuffer_of(r):
    d_vals, _ = ie.unpack_rgba16f(r.gbuffer(5))
    return {"scene_color": ie.unpack_rgba8(r.gbuffer(1)) / 255.0, "b": ie.unpack_rgba8(r.gbuffer(3)) / 255.0, "c": ie.unpack_rgba8(r.gbuffer(4)) / 255.0,
            "a": ie.unpack_a2r10g10b10(r.gbuffer(2)) / np.array([1023.0, 1023.0, 1023.0, 3.0]), "d": d_vals}


def forward_surface(c, prim, mvp):
    """Base.frag's inputs from base_scene() at the winners `prim`: lighting()'s dict, and the pixels base_scene excuses"""
    k = c.case
    W, H = k.W, k.H
    mine = ie.base_scene(k.scene.draws(), mvp, prim, W, H)
    ys, xs = mine["yx"]
    gb = {n: np.zeros((H, W, 4)) for n in ("scene_color", "a", "b", "c", "d")}
    for n in ("scene_color", "b", "c", "d"):
        gb[n][ys, xs] = mine[n]
    gb["a"][ys, xs, :3] = (mine["normal"] + 1.0) / 2.0
    gb["ao_rgb"], gb["vertex_color"] = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    gb["ao_rgb"][ys, xs], gb["vertex_color"][ys, xs] = mine["ao_rgb"], mine["vertex_color"]
    excused = np.zeros((H, W), bool)
    excused[ys[mine["ambiguous"]], xs[mine["ambiguous"]]] = True
    return gb, excused


LIT_VIEWS = (0, 7, 8, 10)      # views whose value passes through the lighting (PCF ties, cube faces): within one LSB on 99.9 %


def check_frame(have, c, gb, smap, view, debug_view, forward, sky_st, bg_st, covered=None, excused=None, aniso=True, control=None):
    """one frame (H, W, 4 codes) against the statements.  covered: forward only, the pixels the main pass shaded (the others hold the
    clear).  -> dict of measurements, "ok" whether every assertion of the module holds"""
    k = c.case
    W, H = k.W, k.H
    cube = FACES
    shade = lambda eps, off, v=debug_view: ie.unorm(ie.lighting(gb, smap, view, cube, W, H, pcf_eps=eps, forward=forward, r_offset=off,  # noqa: E731
                                                                 debug_view=v), 8)
    lit = ie.lighting(gb, smap, view, cube, W, H, forward=forward, debug_view=debug_view if debug_view != 9 else 0)
    colour, tol, overlay, amb = isky.compose(lit, sky_st, bg_st, debug_view)
    res = {"ok": True}
    if debug_view == 0:
        r = isky.check_overlay(have, colour, tol, overlay, amb)
        res.update(overlay=r["n"], sky_bad=r["bad"], sky_worst=r["worst"], sky_excused=r["excused"])
        res["ok"] &= r["ok"]
    rest = ~overlay & ~amb
    if forward:
        clear = ~covered & rest & ~excused
        res["clear_ok"] = bool((have[clear][:, :3] == 0).all())
        res["ok"] &= res["clear_ok"]
        rest &= covered & ~excused
    aux = {}
    ie.lighting(gb, smap, view, cube, W, H, forward=forward, out=aux)
    if debug_view == 9 and not forward:
        mv = ie.gbuffer_vis(gb, smap, view, cube, W, H, lit, control=control, aniso=aniso)
        cells = (mv["cell"] >= 0) & ~mv["excused"]
        err = np.abs(have[..., :3] - np.clip(mv["colour"], 0.0, 1.0) * 255.0)          # the UNORM store saturates
        bad = cells & (err > mv["tol"] * 255.0 + 1.0).any(axis=-1)
        res.update(cells=int(cells.sum()), cells_bad=int(bad.sum()), cells_excused=float(((mv["cell"] >= 0) & mv["excused"]).mean()))
        res["ok"] &= res["cells_bad"] == 0
        fin = rest & (mv["cell"] == -1)
        frac, _, on_edge = ie.check_lit(have, lambda eps, off: shade(eps, off, 0), aux["R"], fin)
        res.update(lit=frac, on_edge=on_edge)
        res["ok"] &= frac >= 0.999
    elif debug_view in LIT_VIEWS or (forward and debug_view == 9):
        frac, cube_amb, on_edge = ie.check_lit(have, shade, aux["R"], rest, r_spread=forward) if rest.any() else (1.0, 0.0, 0.0)
        res.update(lit=frac, cube=cube_amb, on_edge=on_edge)
        res["ok"] &= frac >= 0.999 and on_edge < 0.1
    else:
        want = ie.unorm(lit, 8)
        within = np.all(np.abs(have[..., :3] - want) <= 1, axis=-1)
        res["lit"] = float(within[rest].mean())
        res["ok"] &= res["lit"] >= (0.999 if forward else 1.0)
    res["alpha_ok"] = bool((have[..., 3] == 255).all())
    res["ok"] &= res["alpha_ok"]
    return res
