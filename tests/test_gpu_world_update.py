"""A world applied as a difference (zr_world_update_json): after the update everything observable equals that of a NEW context that
loaded the same payload - frames byte for byte, counts, objects, instances, identities, the saved world - and only the time and what
the frame loop keeps differ.

The frames cannot tell whether the visibility history was carried to the right work-item numbers (k_history_carry): the depth test decides
every pixel.  The counters can: a context whose numbering an update shifted must cull exactly what an undisturbed twin culls (nothing
hidden from the camera enters or leaves), so those checks are equalities.
"""
import copy
import json
import time

import numpy as np
import pytest

from parity_util import compare_all
from test_gpu_tiles_world import _oracle_from_renderer, _register_sample_profabs
from zeldaengine_amd import abi, livelink, scenes

pytestmark = pytest.mark.gpu

W, H, SD = 160, 120, 128
CUBE = scenes.synthetic_cubemap(16)
FAR_BOX = scenes.box((0.5, 0.5, 0.5), (300.0, 300.0, 0.0))        # outside the sample camera's frustum: never owns a pixel
CAMERA, LIGHTS, OBJECTS = abi.WORLD_DIFF_CAMERA, abi.WORLD_DIFF_LIGHTS, abi.WORLD_DIFF_OBJECTS
# meshlets per model: plane 1, box 1, uv_sphere() 11
A_ITEMS = 1 + 1 + 64 * 1 + 700 * 11


def world_a():
    w = copy.deepcopy(scenes.sample_world())
    w["Objects"][3]["InstanceCount"] = 700                     # grass_01; grass_02 has no Profab and draws nothing
    return w


def far_box_desc(count=1):
    d = copy.deepcopy(scenes.sample_world()["Objects"][0])
    d["ProfabName"] = "far_box"; d["InstanceCount"] = count
    return d


def ctx(eng, w=W, h=H, sd=SD, ids=False, **kw):
    g = eng.Renderer(w, h, sd, **kw)
    g.set_cubemap(CUBE)
    g.mesh_ids = _register_sample_profabs(g)
    g.mesh_ids["far_box"] = g.mesh_create(*FAR_BOX)
    g.profab_register("far_box", g.mesh_ids["far_box"])
    if ids:
        g.set_id_capture(True)
    return g


def grab(r, ids=False):
    r.finish()
    st = r.stats()
    assert st["overflow"] == 0, st
    out = {"color": r.color(), "g": [r.gbuffer(t) for t in range(6)], "shadow": r.shadowmap().view(np.uint32), "st": st}
    if ids and r.object_count():
        out["ids"] = (r.read_ids(abi.IDS_PRIMITIVE), r.read_ids(abi.IDS_OBJECT), r.instance_coverage())
    return out


def same(a, b, what):
    assert np.array_equal(a["color"], b["color"]), "%s: colour, %d pixels differ" % (what, int((a["color"] != b["color"]).any(axis=2).sum()))
    for t in range(6):
        assert np.array_equal(a["g"][t].view(np.uint8), b["g"][t].view(np.uint8)), "%s: GBuffer target %d" % (what, t)
    assert np.array_equal(a["shadow"], b["shadow"]), "%s: shadow map, %d texels differ" % (what, int((a["shadow"] != b["shadow"]).sum()))
    assert a["st"]["covered_pixels"] == b["st"]["covered_pixels"], what
    assert a["st"]["covered_shadow_texels"] == b["st"]["covered_shadow_texels"], what
    if "ids" in a and "ids" in b:
        for k, name in enumerate(("primitive ids", "{object, instance}", "instance coverage")):
            assert np.array_equal(a["ids"][k], b["ids"][k]), "%s: %s" % (what, name)


def same_scene(s, f, what):
    """Everything but pixels: object order and count, instances, visibility, the saved world, the camera."""
    assert s.object_count() == f.object_count(), what
    for i in range(s.object_count()):
        (ms, a), (mf, b) = s.object_get_instances(i), f.object_get_instances(i)
        assert ms == mf, "%s: mesh of object %d" % (what, i)
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), "%s: instances of object %d" % (what, i)
        (ov, va), (of, vb) = s.object_get_visibility(i), f.object_get_visibility(i)
        assert ov and of and (va is None or (va.all() and np.array_equal(va, vb))), "%s: visibility of object %d" % (what, i)
    assert s.world_save_json() == f.world_save_json(), what
    assert bytes(s.world_camera()) == bytes(f.world_camera()), what


def fresh(eng, world, ids=False, frames=1, keep=False, **kw):
    """frames frame(s) of a new context that loaded `world`"""
    f = ctx(eng, ids=ids, **kw)
    f.world_load_json(json.dumps(world))
    for _ in range(frames):
        f.render()
    out = grab(f, ids)
    if keep:
        return out, f
    f.close()
    return out


def counters(d):
    return {k: d[k] for k in ("scene_changed", "objects_kept", "objects_reinstanced", "objects_added", "objects_removed", "materials_rebuilt")}


def delta(changed=0, kept=0, reinst=0, added=0, removed=0, mats=0):
    return {"scene_changed": changed, "objects_kept": kept, "objects_reinstanced": reinst, "objects_added": added, "objects_removed": removed,
            "materials_rebuilt": mats}


# ---------------------------------------------------------------------------------------------------- 1. equals a fresh load

def _steps():
    """(name, edit of the running world, differs, expected counters, history_items) - each applied on top of the one before"""
    def camera(w): w["MainCamera"]["Position"] = [6.0, 4.0, 5.5]
    def light(w): w["PointLights"][2]["Color"] = [0.1, 0.9, 0.3]
    def rock90(w): w["Objects"][2]["InstanceCount"] = 90
    def grass(w): w["Objects"][3]["MinRadius"] = 1.5; w["Objects"][3]["MaxRadius"] = 6.5
    def drop(w): del w["Objects"][1]                        # rock_01, from the middle: rock_02 and grass_01 get new seeds
    def append(w): w["Objects"].append(far_box_desc())
    def reverse(w): w["Objects"].reverse()                  # grass_01 stays third of five: its seed and values stay
    def empty(w): w["Objects"] = []
    def again(w): w.clear(); w.update(world_a())
    return [
        ("identical", lambda w: None, 0, delta(0, kept=4), 0),
        ("camera moved", camera, CAMERA, delta(0, kept=4), 0),
        ("point light recoloured", light, LIGHTS, delta(0, kept=4), 0),
        ("rock_02 64 -> 90", rock90, OBJECTS, delta(1, kept=3, reinst=1), A_ITEMS),
        ("grass_01 radius range", grass, OBJECTS, delta(1, kept=3, reinst=1), 0),
        ("a desc removed from the middle", drop, OBJECTS, delta(1, kept=1, reinst=2, removed=1), 1 + 90 + 7700),
        ("a desc appended", append, OBJECTS, delta(1, kept=3, added=1), 1 + 90 + 7700),
        ("Objects reversed", reverse, OBJECTS, delta(1, kept=3, reinst=1), 1 + 1 + 90 + 7700),
        ("Objects empty", empty, OBJECTS, delta(1, removed=4), 0),
        ("A again", again, CAMERA | LIGHTS | OBJECTS, delta(1, added=4), 0),
    ]


def test_update_equals_a_fresh_load(gpu_engine):
    s = ctx(gpu_engine, ids=True)
    w = world_a()
    s.world_load_json(json.dumps(w))
    for _ in range(3):
        s.render()
    for name, edit, differs, want, items in _steps():
        edit(w)
        d = s.world_update_json(json.dumps(w))
        assert d["differs"] == differs, (name, d)
        assert counters(d) == want, (name, d)
        assert d["history_items"] == items, (name, d)
        with pytest.raises(gpu_engine.ZeldaRenderError) as e:          # the identities went with the old world, as after a load
            s.read_ids(abi.IDS_PRIMITIVE)
        assert e.value.code == abi.ERR_STATE, name
        s.render()
        got = grab(s, ids=True)
        ref, f = fresh(gpu_engine, w, ids=True, keep=True)
        same(got, ref, name)
        same_scene(s, f, name)
        f.close()
        s.render()                                                     # ... and the frame after it (the kept history at work)
        same(grab(s, ids=True), ref, name + ", second frame")
    s.close()


def test_update_in_forward_shading_and_against_the_oracle(oracle_lib, gpu_engine):
    """rock_02 64 -> 90 (a draw resized, later bases shifted): the deferred frame against the CPU oracle, the forward frame against a
    fresh context's."""
    s = ctx(gpu_engine)
    w = world_a()
    s.world_load_json(json.dumps(w))
    for _ in range(2):
        s.render()
    w["Objects"][2]["InstanceCount"] = 90
    d = s.world_update_json(json.dumps(w))
    assert counters(d) == delta(1, kept=3, reinst=1) and d["history_items"] == A_ITEMS
    s.render(); s.finish()
    ids = s.mesh_ids
    meshes = {ids["terrain"]: scenes.grid_plane(20.0, 4, 0.0), ids["rock_01"]: scenes.box((0.5, 0.5, 0.5), (0, 0, 0.5)), ids["grass_01"]: scenes.uv_sphere()}
    o = _oracle_from_renderer(oracle_lib, s, meshes, W, H, SD, CUBE)
    o.render()
    bad = {k: v for k, v in compare_all(o, s).items() if v}
    assert not bad, bad
    assert s.stats()["covered_pixels"] == o.covered_pixels()
    s.set_shading(True)
    s.render()
    f = ctx(gpu_engine)
    f.set_shading(True)
    f.world_load_json(json.dumps(w))
    f.render()
    same(grab(s), grab(f), "forward")
    f.close(); s.close()


# ---------------------------------------------------------------------------------------------------- 2. camera and lights only

def test_camera_only_update_keeps_history_and_shadow_map(gpu_engine):
    s, t = ctx(gpu_engine), ctx(gpu_engine)
    w = world_a()
    for r in (s, t):
        r.world_load_json(json.dumps(w))
        for _ in range(3):
            r.render()
    w["MainCamera"]["Position"] = [5.5, 4.5, 5.0]
    d = s.world_update_json(json.dumps(w))
    assert d["differs"] == CAMERA and d["scene_changed"] == 0 and counters(d) == delta(0, kept=4) and d["history_items"] == 0
    s.render()
    got = grab(s)
    assert got["st"]["round1_survivors"] > 0                      # last frame's visibility still counts ...
    times = s.pass_times(1)
    assert times["cull_shadow"] == 0.0 and times["shadow"] == 0.0, times      # ... and the shadow map was kept
    t.world_load_json(json.dumps(w))
    t.render()
    loaded = grab(t)
    assert loaded["st"]["round1_survivors"] == 0                  # a load forgets
    assert t.pass_times(1)["shadow"] > 0.0
    ref = fresh(gpu_engine, w)
    same(got, ref, "camera moved"); same(loaded, ref, "loaded")
    w["MainCamera"]["FOV"] = 50.0                                  # the light's projection takes the camera's FOV: the map is drawn again
    d = s.world_update_json(json.dumps(w))
    assert d["differs"] == CAMERA and d["scene_changed"] == 0
    s.render()
    got = grab(s)
    assert s.pass_times(1)["shadow"] > 0.0 and got["st"]["round1_survivors"] > 0
    same(got, fresh(gpu_engine, w), "FOV")
    s.close(); t.close()


# ---------------------------------------------------------------------------------------------------- 3. the carry is exact

def _twins(eng, flags, moving_light):
    s, t = ctx(eng, flags=flags), ctx(eng, flags=flags)
    a = world_a()
    b = world_a()
    b["Objects"].append(far_box_desc())          # non-instanced: drawn ahead of the instanced draws, whose work bases all move up by one
    d, p, sp = scenes.lights_from_world(a)
    cam = abi.make_camera((5.0, 5.0, 5.0), (0.0, 0.0, 0.5))
    frame_no = [0, 0]

    def frame(r, k):
        if moving_light:                         # the same uniforms on both, a little further every frame: the map is drawn
            i = frame_no[k]
            d[0]["Position"][:3] = (20.0 + 0.3 * i, 0.4 * i, 20.0); d[0]["Direction"][:3] = d[0]["Position"][:3]
            r.update_uniforms(cam, d, p, sp, 0.0, 0.0, 1.0)
        frame_no[k] += 1
        r.render()
        return grab(r)

    keys = ("round1_survivors", "hiz_culled", "survivors") + (("shadow_occluded", "shadow_late") if moving_light else ())

    def agree(gs, gt, what):
        same(gs, gt, what)
        for k in keys:
            a_, b_ = gs["st"][k], gt["st"][k]
            assert (a_[1] if k == "survivors" else a_) == (b_[1] if k == "survivors" else b_), (what, k, gs["st"], gt["st"])

    for r in (s, t):
        r.world_load_json(json.dumps(a))
    for _ in range(3):
        gs, gt = frame(s, 0), frame(t, 1)
    agree(gs, gt, "frame 3")
    assert gt["st"]["round1_survivors"] > 0, gt["st"]      # there is a history to lose
    dl = s.world_update_json(json.dumps(b))      # n_work grows past the pools' capacity: they are re-made
    assert counters(dl) == delta(1, kept=4, added=1) and dl["history_items"] == A_ITEMS, dl
    agree(frame(s, 0), frame(t, 1), "frame 4: bases shifted up, pools re-made")
    dl = s.world_update_json(json.dumps(a))      # ... and down again, in place
    assert counters(dl) == delta(1, kept=4, removed=1) and dl["history_items"] == A_ITEMS, dl
    agree(frame(s, 0), frame(t, 1), "frame 5: bases shifted down")
    s.close(); t.close()


def test_carried_history_culls_what_an_undisturbed_twin_culls(gpu_engine):
    _twins(gpu_engine, 0, False)


def test_carried_shadow_flags_match_an_undisturbed_twin(gpu_engine):
    _twins(gpu_engine, abi.FLAG_SHADOW_OCCLUSION, True)


# ---------------------------------------------------------------------------------------------------- 4. partial carry

def test_partial_carry_when_a_draw_shrinks_and_grows(gpu_engine):
    s, t = ctx(gpu_engine), ctx(gpu_engine)
    w = world_a()
    for r in (s, t):
        r.world_load_json(json.dumps(w))
        for _ in range(3):
            r.render()
    for count, items in ((40, A_ITEMS - 24), (64, A_ITEMS - 24)):
        w["Objects"][2]["InstanceCount"] = count
        d = s.world_update_json(json.dumps(w))
        assert counters(d) == delta(1, kept=3, reinst=1) and d["history_items"] == items, d
        s.render()
        got = grab(s)
        t.world_load_json(json.dumps(w))
        t.render()
        first = grab(t)
        t.render()
        second = grab(t)
        ref = fresh(gpu_engine, w)
        same(got, ref, "rock_02 -> %d" % count); same(first, ref, "loaded"); same(second, ref, "loaded, second frame")
        assert first["st"]["round1_survivors"] == 0
        assert got["st"]["round1_survivors"] > 0, got["st"]
        if count == 40:      # after the shrink every carried item is one the loaded twin knows too, a frame later
            assert got["st"]["round1_survivors"] <= second["st"]["round1_survivors"], (got["st"], second["st"])
        s.render()                               # (both at their second frame of this world before the next step)
        same(grab(s), ref, "second frame")
    s.close(); t.close()


# ---------------------------------------------------------------------------------------------------- 5. rules

def _checker(seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def test_rules_hidden_texture_moved_and_added_objects(gpu_engine):
    import torch
    img = _checker(1)
    mat, keep = abi.make_material([img] + [None] * 6)

    def make():
        g = ctx(gpu_engine)
        g.profab_register("painted", g.mesh_create(*scenes.box((0.6, 0.6, 0.6), (1.5, 1.0, 0.6))), mat)
        return g

    w = world_a()
    painted = copy.deepcopy(w["Objects"][0]); painted["ProfabName"] = "painted"
    w["Objects"].insert(2, painted)              # objects: terrain, rock_01, painted, rock_02 (64), grass_01 (700)
    s = make()
    s.world_load_json(json.dumps(w))
    s.render()
    f = make()
    f.world_load_json(json.dumps(w))
    f.render()
    ref = grab(f)
    same(grab(s), ref, "loaded")
    # a kept object hidden as a whole, and some instances of another: shown again
    s.object_set_visible(1, False)
    vis = np.ones(64, np.uint8); vis[::3] = 0
    s.object_set_instance_visibility(3, vis)
    s.render()
    assert not np.array_equal(grab(s)["color"], ref["color"])
    d = s.world_update_json(json.dumps(w))
    assert d["differs"] == 0 and counters(d) == delta(1, kept=5), d
    s.render()
    same(grab(s), ref, "hidden, then updated"); same_scene(s, f, "hidden, then updated")
    # a kept object's texture replaced: the Profab's image again
    s.object_set_texture(2, 0, _checker(2))
    s.render(); s.finish()
    assert not np.array_equal(s.object_get_texture(2, 0)[0], img)
    d = s.world_update_json(json.dumps(w))
    assert counters(d) == delta(1, kept=4, mats=1), d
    s.render()
    same(grab(s), ref, "texture replaced, then updated")
    assert np.array_equal(s.object_get_texture(2, 0)[0], img)
    # a kept object moved with the device form of the instance update: the generated values again
    _, inst = s.object_get_instances(3)
    moved = inst.copy(); moved["InstancePosition"][:, 2] += 0.7
    dev = torch.from_numpy(moved.view(np.uint8).reshape(-1, 32).copy()).cuda()
    s.object_update_instances_async(3, dev)
    s.render()
    assert not np.array_equal(grab(s)["color"], ref["color"])
    d = s.world_update_json(json.dumps(w))
    assert counters(d) == delta(1, kept=4, reinst=1), d
    s.render()
    same(grab(s), ref, "moved, then updated"); same_scene(s, f, "moved, then updated")
    # an object the host added itself is dropped, as a load drops it
    s.object_add(s.mesh_ids["rock_01"], None, scenes.generate_instances(50, 1.0, 4.0, 0.2, 0.4, seed=9))
    s.render()
    assert s.object_count() == 6
    d = s.world_update_json(json.dumps(w))
    assert counters(d) == delta(1, kept=5, removed=1) and d["history_items"] == A_ITEMS + 1, d
    s.render()
    same(grab(s), ref, "added, then updated"); same_scene(s, f, "added, then updated")
    s.close(); f.close()


def test_a_deformed_mesh_stays_deformed_as_across_a_load(gpu_engine):
    s, t = ctx(gpu_engine), ctx(gpu_engine)
    w = world_a()
    v = scenes.uv_sphere()[0].copy()
    v["Position"][:, 2] *= 1.6                   # taller spheres
    for r in (s, t):
        r.world_load_json(json.dumps(w))
        r.render()
        r.mesh_set_vertices(r.mesh_ids["grass_01"], v)
        r.render()
    plain = fresh(gpu_engine, w)
    assert not np.array_equal(grab(s)["color"], plain["color"])
    w["Objects"][2]["InstanceCount"] = 90
    d = s.world_update_json(json.dumps(w))
    assert counters(d) == delta(1, kept=3, reinst=1), d
    t.world_load_json(json.dumps(w))
    s.render(); t.render()
    gs, gt = grab(s), grab(t)
    same(gs, gt, "deformed: update against load")
    assert not np.array_equal(gs["color"], fresh(gpu_engine, w)["color"])
    assert np.array_equal(s.mesh_get_vertices(s.mesh_ids["grass_01"])["Position"], v["Position"])
    s.close(); t.close()


# ---------------------------------------------------------------------------------------------------- 6. refusals

def test_refused_updates_leave_the_context_as_it_was(gpu_engine, tmp_path):
    s = ctx(gpu_engine)
    s.set_asset_root(str(tmp_path))              # an (empty) content tree: the world below names no file
    w = world_a()
    w["Skydome"].update(OverrideSkydome=False, OverrideCubemap=False)
    w["Background"]["OverrideBackground"] = False
    s.world_load_json(json.dumps(w))
    s.render()
    before = grab(s)
    saved = s.world_save_json()

    def bad(edit):
        b = copy.deepcopy(w)
        b["MainCamera"]["Position"] = [7.0, 3.0, 4.0]; b["Objects"][2]["InstanceCount"] = 90      # (what must NOT happen)
        edit(b)
        return json.dumps(b)

    def lights17(b): b["DirectionalLights"] = [b["DirectionalLights"][0]] * 17
    def too_many(b): b["Objects"][3]["InstanceCount"] = 4194305
    def outside(b): b["Background"].update(OverrideBackground=True, BackgroundFileName="../outside.png")
    def missing(b): b["Background"].update(OverrideBackground=True, BackgroundFileName="Content/Textures/not_there.png")
    cases = [("malformed", "{not json", abi.ERR_PARSE), ("17 directional lights", bad(lights17), abi.ERR_PARSE),
             ("InstanceCount above the limit", bad(too_many), abi.ERR_PARSE), ("a name that leaves the tree", bad(outside), abi.ERR_ARG),
             ("a missing file", bad(missing), abi.ERR_IO)]
    for name, text, code in cases:
        with pytest.raises(gpu_engine.ZeldaRenderError) as e:
            s.world_update_json(text)
        assert e.value.code == code, (name, e.value)
        s.render()
        same(grab(s), before, name)
        assert s.world_save_json() == saved and s.object_count() == 4, name
    s.render_geometry()                          # between the stages of a frame
    with pytest.raises(gpu_engine.ZeldaRenderError) as e:
        s.world_update_json(bad(lambda b: None))
    assert e.value.code == abi.ERR_STATE
    s.render_lighting()
    same(grab(s), before, "between the stages")
    s.render()
    same(grab(s), before, "after the refused frame")
    assert s.world_save_json() == saved
    d = s.world_update_json(bad(lambda b: None))              # ... and the same payload is taken once the frame is finished
    assert d["differs"] == CAMERA | OBJECTS and counters(d) == delta(1, kept=3, reinst=1)
    s.close()


# ---------------------------------------------------------------------------------------------------- 7. livelink

def _poll(g):
    for _ in range(100):
        if g.livelink_poll():
            return True
        time.sleep(0.02)
    return False


def test_livelink_incremental(gpu_engine):
    g = ctx(gpu_engine, 128, 96, 64)
    g.livelink_set_incremental(True)
    port = g.livelink_serve(0)
    w = world_a()
    assert livelink.send_world(w, port=port, host="127.0.0.1") == b""
    assert _poll(g), "the livelink payload never reached the render thread"
    assert g.object_count() == 4
    for _ in range(3):
        g.render()
    w["MainCamera"]["Position"] = [5.5, 4.5, 5.0]
    livelink.send_world(w, port=port, host="127.0.0.1")
    assert _poll(g)                              # the second poll reports a reload
    g.render()
    got = grab(g)
    assert got["st"]["round1_survivors"] > 0     # ... that kept the history
    f = ctx(gpu_engine, 128, 96, 64)
    f.world_load_json(json.dumps(w))
    f.render()
    same(got, grab(f), "livelink"); same_scene(g, f, "livelink")
    g.livelink_stop()
    g.close(); f.close()


# ---------------------------------------------------------------------------------------------------- 8. work lists and rank contexts

def test_update_with_work_lists(gpu_engine):
    """70 000 instances of an 8 x 5 sphere at 320 x 180: k_cull_instances builds work lists.  The plane goes: the instanced draw's work
    base moves down by one, its values stay (its place in Objects does)."""
    def make():
        g = gpu_engine.Renderer(320, 180, 256)
        g.set_cubemap(CUBE)
        g.profab_register("terrain", g.mesh_create(*scenes.grid_plane(40.0, 4, 0.0)))
        g.profab_register("grass_01", g.mesh_create(*scenes.uv_sphere(8, 5)))
        return g
    w = world_a()
    grass = w["Objects"][3]
    grass.update(InstanceCount=70000, MinRadius=1.0, MaxRadius=14.0, MinPScale=0.05, MaxPScale=0.2)
    w["Objects"] = [grass, w["Objects"][0]]
    w["MainCamera"].update(Position=[12.0, -9.0, 7.0])
    s, f = make(), make()
    s.world_load_json(json.dumps(w))
    for _ in range(3):
        s.render()
    kept = grab(s)["st"]
    del w["Objects"][1]
    d = s.world_update_json(json.dumps(w))
    assert counters(d) == delta(1, kept=1, removed=1) and d["history_items"] == 70000, d
    s.render()
    got = grab(s)
    f.world_load_json(json.dumps(w))
    f.render()
    same(got, grab(f), "plane removed"); same_scene(s, f, "plane removed")
    assert 0 < got["st"]["round1_survivors"] <= kept["round1_survivors"]
    s.close(); f.close()


def test_update_on_rank_contexts(gpu_engine):
    """tile_world = 2: after an update each rank's packed tiles are a fresh rank context's."""
    a, b = world_a(), world_a()
    b["Objects"][2]["InstanceCount"] = 90
    b["Objects"].append(far_box_desc())
    for rank in range(2):
        s, f = ctx(gpu_engine, tile_rank=rank, tile_world=2), ctx(gpu_engine, tile_rank=rank, tile_world=2)
        s.world_load_json(json.dumps(a))
        for _ in range(2):
            s.render()
        d = s.world_update_json(json.dumps(b))
        assert counters(d) == delta(1, kept=3, reinst=1, added=1) and d["history_items"] == A_ITEMS, d
        f.world_load_json(json.dumps(b))
        for k in range(2):
            s.render(); f.render()
            s.finish(); f.finish()
            assert np.array_equal(s.read_tiles(), f.read_tiles()), (rank, k)
            assert s.stats()["covered_pixels"] == f.stats()["covered_pixels"] and s.stats()["overflow"] == 0
        s.close(); f.close()
