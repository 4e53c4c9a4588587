"""The CPU oracle's skydome, background and debug views against the INDEPENDENT float64 statements (tests/independent_sky.py,
tests/independent_eval.py's debug-view switch and gbuffer_vis), deferred and forward.

Until now these passes were checked only for bit equality between the oracle and the kernels (tests/test_gpu_scenes.py), so a misreading
both share would pass.  Here the dome is rasterised by the geometry statement against ITS OWN deferred depth (not the oracle's), sampled
through independent_sampler's chains, and composed over the lit quad in view 0 only; views 1-10 are the switch of BaseLighting.frag
(deferred, over the oracle's GBuffer and shadow map as tests/test_oracle_textured.py does) and of Base.frag (forward, over base_scene's
own surface at the oracle's winners).  Outside the derived ambiguity masks: every sky / background channel within its span plus one code,
views 1-6 within one code on every pixel (forward: 99.9 %, ComputeNormal's derivatives), the lit views within one LSB on 99.9 % with
the PCF and cube-face allowances of tests/test_oracle_textured.py, view 9's cells within their span.  The excused fractions are capped
per scene.  Each negative control states one rule the way the engine's text rules out and must make its comparison FAIL.

View 9: the literal reading re-samples the GBuffer with the samplers' anisotropy (N = 2 taps for unequal editor bars); the contract
takes one bilinear tap (oracle/CONTRACT.md row 7).  The literal build is held to the literal statement, the contract build to the
statement with row 7 applied, and the statement without anisotropy must fail against the literal build.
"""
import numpy as np
import pytest

import independent_geometry as ig
import independent_sampler as isamp
import independent_sky as isky
from independent_scenes import SKY_SCENES
from independent_sky_checks import SKY_CAPS, VIEW_SCENES, VIEWS, check_frame, forward_surface, gbuffer_of, load, statement


def _oracle(oracle_lib, c, forward=False, literal=False):
    k = c.case
    o = oracle_lib.Oracle(k.W, k.H, k.SD, literal=literal)
    load(o, c, forward)
    return o


def run(oracle_lib, name, views, forward, control=None, literal=False, aniso=None):
    """render `name` in each of `views` with the oracle and hold it to the statements -> {view: measurements}"""
    c = SKY_SCENES[name]()
    fu, st, sky, bg = statement(name, c, control if control in isky.CONTROLS else None)
    o = _oracle(oracle_lib, c, forward, literal)
    mvp, _sh, view = o.get_frame()
    bad = ig.check_uniforms(o.get_frame(), fu, *c.case.lights[:2]) if not any(c.bars) else []
    assert not bad, bad
    out = {}
    for v in views:
        o.render(v)
        have = o.color().astype(np.int64)
        if forward:
            prim = o.visibility()
            gb, excused = forward_surface(c, prim, mvp)
            covered = prim != 0xFFFFFFFF
        else:
            gb, excused, covered = gbuffer_of(o), None, None
        out[v] = check_frame(have, c, gb, o.shadowmap(), view, v, forward, sky, bg, covered, excused,
                             aniso=literal if aniso is None else aniso, control=control)
    o.close()
    return out


@pytest.mark.parametrize("forward", [False, True], ids=["deferred", "forward"])
@pytest.mark.parametrize("name", list(SKY_SCENES))
def test_oracle_sky_and_background_against_the_statement(oracle_lib, name, forward):
    r = run(oracle_lib, name, [0], forward)[0]
    _fu, _st, sky, bg = statement(name)
    c = SKY_SCENES[name]()
    n = c.case.W * c.case.H
    dome, clipped = (0, 0) if sky is None else (sky["covered"].sum(), (sky["covered"] & sky["clipped"]).sum())
    print("%s %s: %d overlay pixels (dome %d, of them clipped %d; background %d), excused %.4f, worst %.3f tol, lit %.5f" % (
        name, "forward" if forward else "deferred", r["overlay"], dome, clipped, 0 if bg is None else bg["drawn"].sum(), r["sky_excused"],
        r["sky_worst"], r["lit"]))
    assert r["ok"], r
    assert r["sky_excused"] <= SKY_CAPS[name], (name, r["sky_excused"])
    assert r["overlay"] > 0.2 * n
    if name == "sky_pole":
        share = float((sky["ratio"][sky["covered"]] >= isamp.MAX_ANISO).mean())
        print("sky_pole: Pmax / Pmin >= 16 (N clamped) on %.4f of the dome's pixels, max %.1f" % (share, sky["ratio"].max()))
        assert share > 0.05, "the pole scene must reach the anisotropy clamp"
    if name.startswith("sky_coarse"):
        assert (sky["covered"] & sky["clipped"]).sum() > 0.3 * sky["covered"].sum(), "the near plane must cut the visible triangles"


@pytest.mark.parametrize("forward", [False, True], ids=["deferred", "forward"])
@pytest.mark.parametrize("name", VIEW_SCENES)
def test_oracle_debug_views_against_the_statement(oracle_lib, name, forward):
    """views 1-10: the sky and background suppressed, the switch of BaseLighting.frag / Base.frag; view 9 with the contract's one tap"""
    res = run(oracle_lib, name, VIEWS[1:], forward, aniso=False)
    for v, r in res.items():
        print(name, "forward" if forward else "deferred", "view", v, {k: r[k] for k in r if k != "ok"})
        assert r["ok"], (name, v, r)


def test_literal_mosaic_against_the_statement_with_anisotropy(oracle_lib):
    """the literal build's view 9 (N = ceil(Pmax / Pmin) = 2 taps at 200 x 120 with bars 37, 21) against the literal statement"""
    r = run(oracle_lib, "sky_bars_200x120", [9], False, literal=True, aniso=True)[9]
    print("literal view 9:", r)
    assert r["ok"] and r["cells"] > 5000, r


# ---------------------------------------------------------------------------------------------------------------- negative controls

@pytest.mark.parametrize("control,name", [("dome_without_model", "sky_rolled_npot"), ("cull_front", "sky_dome_noise"), ("sky_unorm", "sky_dome_noise"),
                                          ("bg_v_flipped", "sky_dome_noise"), ("bg_clamp", "background_only"), ("bg_lod0", "sky_dome_noise"),
                                          ("no_gamma", "sky_pole")])
def test_control_sky(oracle_lib, control, name):
    """the dome without the stage roll (Model); cull FRONT; the sky image as UNORM (it is sRGB, ZE:5855); the background's v flipped (uv
    (0, 0) is the top-left); CLAMP_TO_EDGE (the samplers REPEAT); the background at lod 0 (its derivatives minify); no gamma: each
    must put sky or background pixels outside the tolerance"""
    r = run(oracle_lib, name, [0], False, control=control)[0]
    print("control %s on %s:" % (control, name), r)
    assert not r["ok"] and r["sky_bad"] > 20


@pytest.mark.parametrize("control,literal", [("mosaic_no_aniso", True), ("cell6_step_y", False)])
def test_control_mosaic(oracle_lib, control, literal):
    """view 9 re-sampled without anisotropy against the literal build (which takes the samplers' two taps); the sixth cell with Step.y * 3
    where the shader has Step.x * 3: each must put mosaic pixels outside the tolerance"""
    r = run(oracle_lib, "sky_bars_200x120", [9], False, control=control, literal=literal, aniso=True)[9]
    print("control %s:" % control, r)
    assert not r["ok"] and r["cells_bad"] > 20
