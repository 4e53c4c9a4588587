"""A live context takes a new extent and keeps its scene (zr_resize, csrc/zr_resize.cpp; DESIGN.md section 5, "Resizing").

The contract: after zr_resize(ctx, W', H') everything observable is that of a new context with the same zr_config but for the extent,
given the same scene, the same calls and the same last uniforms.  So every frame here is compared bit for bit - six GBuffer planes, the
map, the colour - with the CPU oracle at that extent AND with a context created at that extent; statistics, identity queries, uniforms
and deliveries with that context's.  What the resize must NOT do is as observable: the scene is not submitted again (state that only a
device-form update ever wrote is still there), and the shadow map is kept (its pass times read exactly 0).

Scene and helpers are those of test_gpu_round2_keep.py: the pile (160 x 90, a 128^2 map), the point lights on their spiral.  The extents
are where the code can go wrong: 70 x 50 (W % 4 != 0, partial tiles, a shrink), 257 x 131 (growth past the first allocation, 9 tiles
wide, W % 64 == 1 for the Hi-Z regions and the highlight's word plane), 33 x 31 (one full tile and a sliver), and back.
"""
import numpy as np
import pytest

from parity_util import TARGET_NAMES
from test_gpu_gbuffer_keep import CAMERA_PASSES, ViewChecker, _whole
from test_gpu_round2_keep import BOX, SPHERES, Checker, Stage, _dev, _render, _same
from zeldaengine_amd import abi, dist as zdist

pytestmark = pytest.mark.gpu

START = (160, 90)
WALK = [(160, 90), (70, 50), (257, 131), (33, 31), (160, 90)]
SHADOW_PASSES = ("cull_shadow", "shadow")


class RStage(Stage):
    """The pile at an extent of the test's choosing; a new extent is a new version (the oracle is built again at it)."""

    def __init__(self, extent=START):
        super().__init__("pile")
        self.W, self.H = extent

    def extent(self, wh):
        if (self.W, self.H) != tuple(wh):
            self.W, self.H = wh
            self.version += 1


def _grab(g):
    return [g.color()] + [g.gbuffer(t) for t in range(6)] + [g.shadowmap()]


def _equal(a, b, what):
    """frame, six planes and map of two contexts, bit for bit"""
    for name, x, y in zip(["color"] + TARGET_NAMES + ["shadowmap"], a, b):
        assert x.shape == y.shape, "%s: %s has shape %r, the new context's %r" % (what, name, x.shape, y.shape)
        n = int((x.view(np.uint8) != y.view(np.uint8)).sum())
        assert n == 0, "%s: %s differs from the new context's in %d bytes" % (what, name, n)


def _fresh(eng, st, frames, flags=0, setup=None):
    """A context created at the stage's extent, given the same scene and frames `frames` -> (it, the last frame's pass times)"""
    f = st.renderer(eng, flags)
    if setup:
        setup(f)
    t = None
    for i in frames:
        t = _render(f, st, i)
    return f, t


# ------------------------------------------------------------------------------------------------ 1. the walk

@pytest.mark.parametrize("forward", [False, True])
def test_walk_through_the_extents(oracle_lib, gpu_engine, forward):
    """Two frames at each extent, the point lights moving.  Every frame is the oracle's at that extent and a new context's; so are
    covered_pixels and covered_shadow_texels; nothing overflows.  Once more with forward shading and id capture on: the winners are a new
    context's too."""
    st = RStage()

    def setup(r):
        if forward:
            r.set_shading(True); r.set_id_capture(True)

    g = st.renderer(gpu_engine)
    setup(g)
    chk = ViewChecker(oracle_lib)
    chk.forward = forward
    i = 0
    for step, wh in enumerate(WALK):
        g.resize(*wh)
        st.extent(wh)
        assert g.extent() == wh and (g.W, g.H) == wh
        first = i
        for _ in range(2):
            _render(g, st, i)
            what = "%dx%d (step %d), frame %d" % (wh[0], wh[1], step, i)
            _same(chk.frame(st, i), g, what)
            f, _ = _fresh(gpu_engine, st, range(first, i + 1), setup=setup)
            _equal(_grab(g), _grab(f), what)
            sg, sf = g.stats(), f.stats()
            print(what, {k: sg[k] for k in ("covered_pixels", "covered_shadow_texels", "overflow", "round1_survivors")})
            assert sg["covered_pixels"] == sf["covered_pixels"] and sg["covered_shadow_texels"] == sf["covered_shadow_texels"], (what, sg, sf)
            assert sg["covered_pixels"] > 0 and sg["overflow"] == 0, (what, sg)
            if i == first and step > 0:
                assert sg["round1_survivors"] == 0, "the first frame after a resize draws in one round: %r" % (sg,)
            if forward:
                assert np.array_equal(g.read_ids(abi.IDS_OBJECT), f.read_ids(abi.IDS_OBJECT)), what + ": read_ids"
                assert np.array_equal(g.read_ids(abi.IDS_PRIMITIVE), f.read_ids(abi.IDS_PRIMITIVE)), what + ": read_ids (primitives)"
                assert np.array_equal(g.instance_coverage(), f.instance_coverage()), what + ": instance_coverage"
            f.close()
            i += 1
    g.close()


# ------------------------------------------------------------------------------------------------ 2. through a rest

def test_resize_through_a_rest(oracle_lib, gpu_engine):
    """Four still frames: camera pass, map and light plane are all kept.  A resize, four more: the first draws its camera pass and keeps
    its map (the shadow pass times are exactly 0), the plane is filled once more and read again, at the new extent's size.  The same
    extent again is nothing at all."""
    st = RStage()
    g = st.renderer(gpu_engine)
    chk = Checker(oracle_lib)
    for i in range(4):
        t = _render(g, st, i)
        _same(chk.frame(st, i), g, "frame %d" % i)
    k0 = g.light_keep()
    assert _whole(t) and all(t[k] == 0.0 for k in SHADOW_PASSES) and k0["read"] > 0 and k0["plane_bytes"] == 32 * 160 * 90, (t, k0)
    wh = (257, 131)
    g.resize(*wh); st.extent(wh)
    assert g.light_keep()["plane_bytes"] == 0
    did = []
    for i in range(4, 8):
        t = _render(g, st, i)
        print("frame", i, {k: t[k] for k in CAMERA_PASSES + SHADOW_PASSES}, g.light_keep())
        _same(chk.frame(st, i), g, "frame %d, %dx%d" % (i, wh[0], wh[1]))
        if i == 4:
            assert all(t[k] > 0.0 for k in ("cull_camera", "gbuffer", "resolve")), "the first frame after the resize drew no camera pass: %r" % (t,)
        assert all(t[k] == 0.0 for k in SHADOW_PASSES), "frame %d drew its shadow map: %r" % (i, t)
        did.append(g.light_keep()["last"])
    k1 = g.light_keep()
    assert did == ["ignored", "ignored", "filled", "read"], did
    assert k1["filled"] == k0["filled"] + 1 and k1["read"] == k0["read"] + 1 and k1["plane_bytes"] == 32 * wh[0] * wh[1], (k0, k1)
    g.resize(*wh)                                                   # the extent it has: nothing happens
    t = _render(g, st, 8)
    _same(chk.frame(st, 8), g, "frame 8, after a resize to the same extent")
    k2 = g.light_keep()
    assert _whole(t) and all(t[k] == 0.0 for k in SHADOW_PASSES), t
    assert k2["last"] == "read" and k2["read"] == k1["read"] + 1 and k2["filled"] == k1["filled"], (k1, k2)
    g.close()


# ------------------------------------------------------------------------------------------------ 3. in flight

def test_resize_with_frames_in_flight(oracle_lib, gpu_engine):
    """zr_resize right behind zr_render, no finish in between - at every step of the walk.  The frames that follow are the oracle's."""
    st = RStage()
    g = st.renderer(gpu_engine)
    chk = Checker(oracle_lib)
    i = 0
    for wh in WALK[1:]:
        st.uniforms(g, i); g.render()
        st.uniforms(g, i + 1); g.render()                           # two frames in flight
        g.resize(*wh); st.extent(wh)
        i += 2
        for _ in range(2):
            st.uniforms(g, i); g.render()
            g.finish()
            _same(chk.frame(st, i), g, "%dx%d, frame %d" % (wh[0], wh[1], i))
            assert g.stats()["overflow"] == 0
            i += 1
    g.close()


# ------------------------------------------------------------------------------------------------ 4. device-only state survives

def test_what_only_the_device_holds_is_still_there(gpu_engine):
    """A texture, an instance range and a vertex range last written by the device forms have no host copy.  After a resize the frame is
    that of a new context given the same values by the host forms, and the texture reads back as updated."""
    import torch
    st = RStage()
    st.box_image = np.random.default_rng(4).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    g = st.renderer(gpu_engine)
    for i in range(2):
        _render(g, st, i)
    image = 255 - st.box_image
    inst = st.inst[:60].copy()
    inst["InstancePosition"][:, 2] += np.float32(2.5); inst["InstancePScale"] *= np.float32(1.5)
    verts = st.sphere[0].copy(); verts["Position"][:, 2] *= np.float32(1.3)
    dev = torch.device("cuda", 0)
    g.object_update_texture_async(BOX, 0, torch.from_numpy(image.copy()).to(dev))
    g.object_update_instances_async(SPHERES, _dev(inst, 32))
    g.mesh_update_vertices_async(SPHERES, torch.from_numpy(verts.view(np.uint8).reshape(-1, abi.XkVertex.itemsize).copy()).to(dev))
    _render(g, st, 2)
    wh = (70, 50)
    g.resize(*wh); st.extent(wh)

    def host_forms(f):
        f.object_set_texture(BOX, 0, image)
        f.object_set_instances(SPHERES, inst)
        f.mesh_set_vertices(SPHERES, verts)

    for i in (3, 4):
        _render(g, st, i)
        f, _ = _fresh(gpu_engine, st, range(3, i + 1), setup=host_forms)
        _equal(_grab(g), _grab(f), "frame %d after the resize" % (i - 2))
        f.close()
    assert np.array_equal(g.object_get_texture(BOX, 0)[0], image)
    assert np.array_equal(g.object_get_instances(SPHERES)[1][:60].view(np.uint8), inst.view(np.uint8))
    assert np.array_equal(g.mesh_get_vertices(SPHERES).view(np.uint8), verts.view(np.uint8))
    g.close()


# ------------------------------------------------------------------------------------------------ 5. uniforms

def test_uniforms_follow_the_extent_or_stay_as_given(gpu_engine):
    """After a resize get_frame is byte for byte a new context's after the same update_uniforms; uniforms last set raw by set_frame
    stay as the caller gave them; a context that never had uniforms still has none."""
    st = RStage()
    g = st.renderer(gpu_engine)
    st.uniforms(g, 3)
    for wh in WALK[1:4]:
        g.resize(*wh); st.extent(wh)
        f = st.renderer(gpu_engine)
        st.uniforms(f, 3)
        for name, a, b in zip(("cam", "shadow", "view"), g.get_frame(), f.get_frame()):
            assert a.tobytes() == b.tobytes(), "%dx%d: %s differs from a new context's" % (wh[0], wh[1], name)
        f.close()
    cam, sh, view = g.get_frame()
    cam["Proj"][0] *= np.float32(1.25); view["ViewportInfo"][2] = 7.0
    g.set_frame(cam, sh, view)
    g.resize(*START)
    for name, a, b in zip(("cam", "shadow", "view"), g.get_frame(), (cam, sh, view)):
        assert a.tobytes() == b.tobytes(), "set_frame's %s changed with the extent" % name
    g.close()
    n = gpu_engine.Renderer(64, 64, 128)
    n.resize(96, 40)
    with pytest.raises(gpu_engine.ZeldaRenderError) as e:
        n.render()
    assert e.value.code == abi.ERR_STATE
    n.close()


# ------------------------------------------------------------------------------------------------ 6. deliveries

def test_deliveries_of_changes_go_on_at_the_new_extent(gpu_engine):
    """Packed deliveries at delta scale 2: deliver, resize, deliver.  The second is a full one with the new tile count and the next
    serial, and decodes into a zeroed client as the new frame filtered by 2."""
    st = RStage()
    g = st.renderer(gpu_engine)
    g.set_frame_delta_scale(2)
    g.set_frame_delta(abi.FRAME_DELTA_PACKED)
    _render(g, st, 0)
    t, o, s, h0 = g.read_frame_delta_packed()
    assert (h0["full"], h0["serial"]) == (1, 1) and h0["total_tiles"] == 3 * 2, h0            # 80 x 45
    _render(g, st, 1)
    _, _, _, h1 = g.read_frame_delta_packed()
    assert (h1["full"], h1["serial"]) == (0, 2), h1
    wh = (257, 131)
    g.resize(*wh); st.extent(wh)
    assert g.frame_delta_extent() == (129, 66, 5 * 3, 2)
    with pytest.raises(gpu_engine.ZeldaRenderError) as e:                                    # no frame yet at this extent
        g.read_frame_delta_packed()
    assert e.value.code == abi.ERR_STATE
    _render(g, st, 2)
    t, o, s, h2 = g.read_frame_delta_packed()
    assert (h2["full"], h2["serial"], h2["total_tiles"], h2["n_tiles"]) == (1, 3, 15, 15), h2
    client = np.zeros((66, 129, 4), dtype=np.uint8)
    gpu_engine.frame_delta_decode(t, o, s, client)
    assert np.array_equal(client, g.color_scaled(2))
    _render(g, st, 3)
    t, o, s, h3 = g.read_frame_delta_packed()
    assert (h3["full"], h3["serial"]) == (0, 4), h3
    gpu_engine.frame_delta_decode(t, o, s, client)
    assert np.array_equal(client, g.color_scaled(2))
    g.close()


def test_a_highlighted_delivery_after_a_resize(gpu_engine):
    """The set made before the resize is still the set, and a highlighted delivery of the new frame is the host statement of the rule
    over that frame with the mask of its own winners."""
    st = RStage()
    g = st.renderer(gpu_engine)
    g.set_id_capture(True)
    on = np.zeros(len(st.inst), dtype=np.uint8); on[::3] = 1
    g.highlight_set(SPHERES, on)
    g.highlight_set(BOX, 1)
    g.set_frame_delta_highlight(True)
    g.set_frame_delta(True)
    _render(g, st, 0)
    g.read_frame_delta()
    before = g.highlight_get().copy()
    wh = (257, 131)
    g.resize(*wh); st.extent(wh)
    assert np.array_equal(g.highlight_get(), before) and before.sum() == on.sum() + 1
    _render(g, st, 1)
    tiles, pixels, h = g.read_frame_delta()
    assert (h["full"], h["serial"], h["total_tiles"], h["n_tiles"]) == (1, 2, 9 * 5, 45), h
    client = np.zeros((5 * 32, 9 * 32, 4), dtype=np.uint8)
    for tile, px in zip(tiles, pixels):
        y, x = 32 * (int(tile) // 9), 32 * (int(tile) % 9)
        client[y:y + 32, x:x + 32] = px
    ids = g.read_ids(abi.IDS_OBJECT)
    base, _ = g.instance_slots()
    slot = np.where(ids[..., 0] == abi.NO_ID, 0, base[np.minimum(ids[..., 0], len(base) - 1)] + ids[..., 1])
    mask = (ids[..., 0] != abi.NO_ID) & (before[slot] != 0)
    assert mask.any() and not mask.all()
    want = gpu_engine.frame_highlight(g.color(), mask)
    assert not np.array_equal(want, g.color())
    assert np.array_equal(client[:wh[1], :wh[0]], want)
    assert np.array_equal(g.color_highlighted(1), want)
    g.close()


# ------------------------------------------------------------------------------------------------ 7. rank contexts

def test_rank_contexts_follow_the_extent(gpu_engine):
    """Two ranks on the one GPU, both resized: each rank's packed tiles are the single context's frame on the tiles the partition gives
    it at the new extent."""
    st = RStage()
    world = 2
    single = st.renderer(gpu_engine)
    ranks = []
    for r in range(world):
        g = gpu_engine.Renderer(st.W, st.H, st.SD, tile_rank=r, tile_world=world)
        st.populate(g)
        ranks.append(g)
    # a caller-owned tile buffer is sized by the old slots_per_rank: the resize (a shrink first, so nothing could land outside it) puts
    # the internal one back, and the caller's is never written again
    import torch
    mine = torch.zeros(ranks[0].tiles_device_buffer()[1], dtype=torch.uint8, device="cuda")
    ranks[0].set_tiles_buffer(mine.data_ptr())
    st.uniforms(ranks[0], 0); ranks[0].render(); ranks[0].finish()
    assert bool(mine.any()), "the caller's tile buffer was not written before the resize"
    mine.zero_(); torch.cuda.synchronize()
    i = 0
    for wh in WALK[1:4]:
        for g in [single] + ranks:
            g.resize(*wh)
        st.extent(wh)
        for _ in range(2):
            for g in [single] + ranks:
                st.uniforms(g, i); g.render(); g.finish()
            assert not bool(mine.any()), "the caller's tile buffer of the old extent was written after the resize"
            want = single.color()
            for r, g in enumerate(ranks):
                owned, spr = gpu_engine.tile_partition(wh[0], wh[1], world, r)
                got = g.read_tiles()
                assert got.shape[0] == spr and g.tiles_device_buffer()[1] == spr * abi.TILE_BYTES
                assert np.array_equal(got, zdist.pack_tiles(want, r, world)), "%dx%d frame %d, rank %d" % (wh[0], wh[1], i, r)
                assert g.stats()["overflow"] == 0
            i += 1
    for g in [single] + ranks:
        g.close()


# ------------------------------------------------------------------------------------------------ 8. refusals

def test_refusals_change_nothing(oracle_lib, gpu_engine):
    st = RStage()
    g = st.renderer(gpu_engine)
    chk = Checker(oracle_lib)
    _render(g, st, 0)
    for wh, code in [((0, 90), abi.ERR_ARG), ((160, 0), abi.ERR_ARG), ((0, 0), abi.ERR_ARG), ((8161, 90), abi.ERR_ARG), ((160, 8161), abi.ERR_ARG),
                     ((8160, 4000), abi.ERR_ARG)]:
        with pytest.raises(gpu_engine.ZeldaRenderError) as e:
            g.resize(*wh)
        assert e.value.code == code, (wh, e.value)
        assert g.extent() == START and (g.W, g.H) == START
    st.uniforms(g, 1)
    g.render_geometry()
    with pytest.raises(gpu_engine.ZeldaRenderError) as e:
        g.resize(70, 50)
    assert e.value.code == abi.ERR_STATE and g.extent() == START
    g.render_lighting(); g.finish()
    _same(chk.frame(st, 1), g, "the frame the refused resize fell into")
    _render(g, st, 2)
    _same(chk.frame(st, 2), g, "the frame after the refusals")
    g.close()


# ------------------------------------------------------------------------------------------------ 9. the native driver

def test_native_headless_driver_resizes_mid_run(gpu_engine, tmp_path):
    """tools/zelda_headless --resize-at 2:WxH: the world is loaded once, frames 2 and 3 are rendered at the new extent; the PPM is the one a
    run started at that extent writes - plain, and through the packed deliveries, whose first delivery after the resize is a full one."""
    import os
    import re
    import subprocess
    import test_gpu_native_host as nh
    from zeldaengine_amd import build as zbuild
    root = str(tmp_path)
    nh._content_tree(root)
    exe = zbuild.build_headless()
    W2, H2 = 257, 131
    total2 = 9 * 5

    def run(name, *extra):
        ppm = os.path.join(root, name + ".ppm")
        cmd = [exe, "--root", root, "--world", "Content/World.json", "--shadow", str(nh.SD), "--frames", "4", "--out", ppm] + list(extra)
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        text = out.stdout.decode(errors="replace")
        assert out.returncode == 0, text
        return open(ppm, "rb").read(), text

    at = "2:%dx%d" % (W2, H2)
    want, _ = run("fresh", "--size", "%dx%d" % (W2, H2))
    plain, text = run("plain", "--size", "%dx%d" % (nh.W, nh.H), "--resize-at", at)
    assert "resized %dx%d" % (W2, H2) in text, text
    assert want.startswith(("P6\n%d %d\n255\n" % (W2, H2)).encode()) and plain == want
    packed, text = run("packed", "--size", "%dx%d" % (nh.W, nh.H), "--resize-at", at, "--delta-packed")
    rows = re.findall(r"^delta-packed (\d+)/(\d+) tiles", text, re.M)
    assert len(rows) == 4 and rows[2] == (str(total2), str(total2)) and rows[3] == ("0", str(total2)), text
    assert packed == want
