"""Object identity of the last frame on the renderer (zr_set_id_capture, zr_read_ids, zr_pick, zr_instance_coverage[_async]).

The winner plane is held to the CPU oracle's visibility buffer and to the float64 geometry statement (tests/independent_geometry.py);
the object plane, the coverage and every pick to tests/ids_reference.py, which tests/test_ids_cpu.py holds to the oracle's shading.
Capture must not move any other output: colour, GBuffer and shadow map are compared bit for bit with capture off and with the oracle.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import ids_reference as idr
import independent_geometry as ig
from independent_scenes import EDGE_SCENES, SCENES, TEXTURED_SCENES, Scene, _lights, case
from independent_sky_checks import load as load_sky
from independent_scenes import SKY_SCENES
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

NO_CULL = abi.FLAG_NO_HIZ | abi.FLAG_NO_FRUSTUM_CULL | abi.FLAG_NO_CONE_CULL


def _spheres(W, H):
    """400 instanced spheres over a plane that crosses the near plane"""
    s = Scene()
    s.add(scenes.grid_plane(40.0, 3, 0.0), [(90, 140, 60, 255), (0, 0, 0, 255), (200, 200, 200, 255), (127, 127, 255, 255),
                                             (255, 255, 255, 255), (0, 0, 0, 255), (255, 255, 255, 255)])
    s.add(scenes.uv_sphere(10, 5, 0.5), None, scenes.generate_instances(400, 0.5, 7.0, 0.3, 0.9, seed=17))
    s.add(scenes.box((0.6, 0.5, 0.7), (0.5, -0.5, 0.7)))
    return s


def _cam(i):
    a = 0.4 + 0.05 * i
    return abi.make_camera((6.0 * math.cos(a), 6.0 * math.sin(a), 1.1 + 0.1 * i), (0.0, 0.0, 0.4), fov=60.0)


def _case_scene(kind, W, H):
    """(loader(r), items, camera(i)); loader feeds the oracle or the renderer"""
    if kind == "spheres":
        s = _spheres(W, H)
        d, p, sp = _lights(1, 4)
        return (lambda r, i: (s.load(r) if i == 0 else None, r.update_uniforms(_cam(i), d, p, sp, 0.0, 0.0, 0.0))), idr.items_of_scene(s)
    if kind in TEXTURED_SCENES:
        c = TEXTURED_SCENES[kind](W, H, 128)
    elif kind in SKY_SCENES:
        sc = SKY_SCENES[kind](W, H)
        c = sc.case

        def loader(r, i):
            if i == 0:
                load_sky(r, sc, False)
            d, p, sp = c.lights
            cam = c.cam if i == 0 else _moved(c.cam)
            r.update_uniforms(cam, d, p, sp, c.roll_stage, c.roll_light, 0.0)
        return loader, idr.items_of_scene(c.scene)
    else:
        c = case(kind, W, H, 128)

    def loader(r, i):
        if i == 0:
            c.scene.load(r)
        d, p, sp = c.lights
        r.update_uniforms(c.cam if i == 0 else _moved(c.cam), d, p, sp, c.roll_stage, c.roll_light, 0.0)
    return loader, idr.items_of_scene(c.scene)


def _moved(cam):
    pos = [cam.Position[k] for k in range(3)]
    return abi.make_camera((pos[0] * 0.97 + 0.05, pos[1] * 0.97, pos[2] + 0.05), tuple(cam.Lookat[k] for k in range(3)), cam.Speed, cam.FOV,
                           cam.zNear, cam.zFar)


def _planes(r):
    return [r.color()] + [r.gbuffer(t).copy() for t in range(6)] + [r.shadowmap().view(np.uint32).copy()]


CASES = [("mixed", 192, 128, 0, False), ("mixed", 257, 131, NO_CULL, True), ("mixed", 33, 17, 0, True),
         ("rolled_and_clipped", 192, 128, 0, False), ("rolled_and_clipped", 257, 131, NO_CULL, False),
         ("spheres", 192, 128, 0, False), ("spheres", 257, 131, 0, True), ("spheres", 33, 17, NO_CULL, False),
         ("tex_packed", 192, 128, 0, False), ("tex_clipped", 257, 131, NO_CULL, True),
         ("sky_dome_noise", 192, 128, 0, False), ("background_only", 257, 131, 0, True)]


@pytest.mark.parametrize("kind,W,H,flags,forward", CASES, ids=["%s_%dx%d_%s_%s" % (k, w, h, "nocull" if f else "cull", "fwd" if fw else "def")
                                                              for k, w, h, f, fw in CASES])
def test_winner_plane_and_queries_against_the_oracle(gpu_engine, oracle_lib, kind, W, H, flags, forward):
    """frame 1 and the second frame of a moving camera (Hi-Z history, two rounds): primitive plane = the oracle's visibility buffer,
    object plane / coverage = the reference mapping, and capture moves nothing else"""
    loader, items = _case_scene(kind, W, H)
    g = gpu_engine.Renderer(W, H, 128, flags=flags)
    off = gpu_engine.Renderer(W, H, 128, flags=flags)
    o = oracle_lib.Oracle(W, H, 128)
    try:
        g.set_id_capture(True)
        for i in range(2):
            for r in (g, off, o):
                loader(r, i)
                r.set_shading(forward)
                r.render()
            g.finish(); off.finish()
            vis = o.visibility().copy()
            got = g.read_ids(abi.IDS_PRIMITIVE)
            bad = int((got != vis).sum())
            assert bad == 0, "%s frame %d: %d of %d pixels name another winner than the oracle" % (kind, i, bad, W * H)
            assert np.array_equal(g.read_ids(abi.IDS_OBJECT), idr.object_plane(vis, items))
            cov = g.instance_coverage()
            assert np.array_equal(cov, idr.coverage(vis, items))
            assert int(cov.sum()) == g.stats()["covered_pixels"] == o.covered_pixels()
            a, b = _planes(g), _planes(off)
            for k, (x, y) in enumerate(zip(a, b)):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "plane %d moved with capture on" % k
            assert np.array_equal(a[0], o.color())
            for t in range(6):
                assert np.array_equal(a[1 + t].view(np.uint8), o.gbuffer(t).view(np.uint8)), "GBuffer %d differs from the oracle" % t
            assert np.array_equal(a[7], o.shadowmap().view(np.uint32))
    finally:
        g.close(); off.close(); o.close()


def test_winner_plane_at_1080p_against_the_oracle(gpu_engine, oracle_lib):
    cfg = scenes.config3(3000, 1920, 1080)
    g = gpu_engine.Renderer(1920, 1080, 1024)
    o = oracle_lib.Oracle(1920, 1080, 1024)
    o.set_threads(16)
    try:
        gpu_engine.load_scene(g, cfg)
        from oracle import pyoracle
        pyoracle.load_scene(o, cfg)
        g.set_id_capture(True)
        g.render(); g.render()
        o.render()
        vis = o.visibility().copy()
        assert np.array_equal(g.read_ids(abi.IDS_PRIMITIVE), vis)
        items = idr.items_of_config(cfg)
        cov = g.instance_coverage()
        assert np.array_equal(cov, idr.coverage(vis, items)) and int(cov.sum()) == g.stats()["covered_pixels"]
    finally:
        g.close(); o.close()


STATEMENT_SCENES = [(n, 192, 128) for n in SCENES] + [(n, None, None) for n in EDGE_SCENES]


@pytest.mark.parametrize("name,W,H", STATEMENT_SCENES, ids=[n for n, _, _ in STATEMENT_SCENES])
def test_winner_plane_against_the_float64_statement(gpu_engine, name, W, H):
    c = case(name, W, H, 256) if W else case(name)
    d, p, sp = c.lights
    fu = ig.frame_uniforms(c.cam, d, p, c.W, c.H, c.roll_stage, c.roll_light, sp, 4)
    st = ig.raster(c.scene.draws(), fu["cam"], c.W, c.H)
    for flags in (0, NO_CULL):
        g = gpu_engine.Renderer(c.W, c.H, c.SD, flags=flags)
        try:
            c.scene.load(g)
            g.set_id_capture(True)
            g.update_uniforms(c.cam, d, p, sp, c.roll_stage, c.roll_light, 0.0)
            g.render()
            rc = ig.check_camera(st, g.gbuffer(0), g.read_ids(abi.IDS_PRIMITIVE))
            assert rc["prim"] == 0 and rc["ok"], (name, flags, rc)
        finally:
            g.close()


def _picks(W, H, rng, vis):
    rects = [(0, 0, W, H), (W - 5, H - 3, 40, 40), (W // 2, 0, W, 7), (0, H // 2, 9, H), (W, 0, 3, 3), (0, H, 1, 1), (W + 7, H + 9, 4, 4)]
    for _ in range(22):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        rects.append((x, y, int(rng.integers(1, W)), int(rng.integers(1, H))))
    # 1 x 1 on silhouettes: pixels whose right or lower neighbour has another winner
    edge = np.zeros_like(vis, dtype=bool)
    edge[:, :-1] |= vis[:, :-1] != vis[:, 1:]
    edge[:-1, :] |= vis[:-1, :] != vis[1:, :]
    ys, xs = np.nonzero(edge)
    for k in rng.choice(len(ys), size=min(16, len(ys)), replace=False):
        rects.append((int(xs[k]), int(ys[k]), 1, 1))
    for _ in range(6):
        rects.append((int(rng.integers(0, W)), int(rng.integers(0, H)), 1, 1))
    return rects


@pytest.mark.parametrize("W,H", [(257, 131), (640, 360)])
def test_pick_against_the_numpy_reference(gpu_engine, W, H):
    loader, items = _case_scene("spheres", W, H)
    g = gpu_engine.Renderer(W, H, 256)
    try:
        g.set_id_capture(True)
        for i in range(2):
            loader(g, i)
            g.render()
        vis, depth = g.read_ids(abi.IDS_PRIMITIVE), g.gbuffer(0)
        rng = np.random.default_rng(2026)
        rects = _picks(W, H, rng, vis)
        assert len(rects) >= 50
        for (x, y, w, h) in rects:
            want, total = idr.pick(vis, depth, items, x, y, w, h)
            hits, n = g.pick(x, y, w, h)
            assert n == total, (x, y, w, h)
            got = [(int(t["object"]), int(t["instance"]), int(t["pixels"]), int(t["triangle"]), int(t["x"]), int(t["y"]), float(t["depth"]))
                   for t in hits]
            assert got == want, (x, y, w, h)
            assert (hits["reserved"] == 0).all()
            if total > 2:                            # truncation at cap: the first entries, the full total
                part, n2 = g.pick(x, y, w, h, cap=2)
                assert n2 == total and len(part) == 2 and np.array_equal(part, hits[:2])
        full, n = g.pick(0, 0, W, H)
        cov = g.instance_coverage()
        assert n == int((cov > 0).sum()) and int(full["pixels"].sum()) == int(cov.sum())
        assert g.pick(W, H, 5, 5)[1] == 0
        with pytest.raises(gpu_engine.ZeldaRenderError) as e:
            g.pick(0, 0, 0, 1)
        assert e.value.code == abi.ERR_ARG
    finally:
        g.close()


def _code(gpu_engine, f):
    try:
        f()
    except gpu_engine.ZeldaRenderError as e:
        return e.code
    return 0


def test_state_errors(gpu_engine):
    import torch
    W, H = 96, 64
    loader, _ = _case_scene("mixed", W, H)
    g = gpu_engine.Renderer(W, H, 128)
    buf = torch.zeros(4096, dtype=torch.int32, device=torch.device("cuda", 0))
    try:
        loader(g, 0)
        queries = [lambda: g.read_ids(abi.IDS_PRIMITIVE), lambda: g.read_ids(abi.IDS_OBJECT), lambda: g.pick(1, 1),
                   lambda: g.instance_coverage(), lambda: g.instance_coverage_async(buf.data_ptr())]
        for q in queries:                                # before any frame
            assert _code(gpu_engine, q) == abi.ERR_STATE
        g.render()
        for q in queries:                                # a frame rendered without capture
            assert _code(gpu_engine, q) == abi.ERR_STATE
        g.set_id_capture(True)
        g.render()
        for q in queries[:4]:
            assert _code(gpu_engine, q) == 0
        g.object_add(g.mesh_create(*scenes.box()))       # the scene changed, no frame since
        for q in queries:
            assert _code(gpu_engine, q) == abi.ERR_STATE
        g.render()
        assert _code(gpu_engine, queries[3]) == 0
        g.render_shadow()                                # between the stages of a frame
        assert _code(gpu_engine, lambda: g.set_id_capture(False)) == abi.ERR_STATE
        for q in queries:
            assert _code(gpu_engine, q) == abi.ERR_STATE
        g.render_gbuffer(); g.render_lighting()
        assert _code(gpu_engine, queries[0]) == 0 and _code(gpu_engine, queries[4]) == 0
        g.finish()
        g.scene_clear()
        assert _code(gpu_engine, queries[0]) == abi.ERR_STATE
    finally:
        g.close()


def test_coverage_async_with_frames_in_flight(gpu_engine):
    """three frames of a moving camera queued back to back, each followed by zr_instance_coverage_async into its own buffer: frame
    N + 2 reuses frame N's winner plane, so it must wait for the census behind frame N"""
    import torch
    W, H = 320, 180
    loader, items = _case_scene("spheres", W, H)
    g = gpu_engine.Renderer(W, H, 256)
    try:
        g.set_id_capture(True)
        loader(g, 0); g.render(); g.finish()
        n = g.instance_slots()[1]
        dev = torch.device("cuda", 0)
        bufs = [torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        for i in range(3):
            loader(g, 1 + i)
            g.render()
            g.instance_coverage_async(bufs[i].data_ptr())
        g.finish()
        torch.cuda.synchronize()
        for i in range(3):
            ref = gpu_engine.Renderer(W, H, 256)
            try:
                ref.set_id_capture(True)
                loader(ref, 0)
                loader(ref, 1 + i)
                ref.render(); ref.render()        # (two frames: the same rounds as the queued context's)
                want = ref.instance_coverage()
            finally:
                ref.close()
            got = bufs[i].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want), "frame %d: async coverage differs from a fresh context's" % i
    finally:
        g.close()


def test_rank_contexts_report_their_owned_tiles(gpu_engine):
    W, H, WORLD = 257, 131, 4
    loader, items = _case_scene("spheres", W, H)
    single = gpu_engine.Renderer(W, H, 256)
    ranks = [gpu_engine.Renderer(W, H, 256, tile_rank=k, tile_world=WORLD) for k in range(WORLD)]
    try:
        for r in [single] + ranks:
            r.set_id_capture(True)
            loader(r, 0)
            r.render()
        want = single.read_ids(abi.IDS_PRIMITIVE)
        union = np.full_like(want, idr.NO_ID)
        T = abi.TILE
        total_cov = np.zeros(single.instance_slots()[1], np.int64)
        for k, r in enumerate(ranks):
            got = r.read_ids(abi.IDS_PRIMITIVE)
            owned = np.zeros_like(want, dtype=bool)
            for t in gpu_engine.tile_partition(W, H, WORLD, k)[0]:
                tx, ty = t % ((W + T - 1) // T), t // ((W + T - 1) // T)
                owned[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] = True
            assert (got[~owned] == idr.NO_ID).all()
            union[owned] = got[owned]
            total_cov += r.instance_coverage()
        assert np.array_equal(union, want)
        assert np.array_equal(total_cov, single.instance_coverage().astype(np.int64))
    finally:
        for r in [single] + ranks:
            r.close()


def test_config4_coverage_is_consistent_with_the_id_planes(gpu_engine):
    """1 M instances at 3840 x 2160 (no oracle at this size): coverage = bincount of the object plane, sum = covered pixels"""
    cfg = scenes.config4()
    W, H = cfg["width"], cfg["height"]
    g = gpu_engine.Renderer(W, H, 1024)
    try:
        gpu_engine.load_scene(g, cfg)
        g.set_id_capture(True)
        g.render(); g.render()
        items = idr.items_of_config(cfg)
        vis = g.read_ids(abi.IDS_PRIMITIVE)
        cov = g.instance_coverage()
        assert np.array_equal(cov, idr.coverage(vis, items))
        assert int(cov.sum()) == g.stats()["covered_pixels"]
        assert np.array_equal(g.read_ids(abi.IDS_OBJECT), idr.object_plane(vis, items))
        hits, n = g.pick(0, 0, W, H, cap=1000)
        assert n == int((cov > 0).sum()) and len(hits) == min(n, 1000)
    finally:
        g.close()


def test_headless_pick_prints_what_renderer_pick_returns(gpu_engine, tmp_path):
    import json
    from test_gpu_native_host import H, SD, W, _content_tree
    from zeldaengine_amd import build as zbuild
    root = str(tmp_path)
    _content_tree(root)
    exe = zbuild.build_headless()
    rect = (W // 4, H // 4, W // 2, H // 2)
    out = subprocess.run([exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (W, H), "--shadow", str(SD),
                          "--frames", "2", "--pick", "%d,%d,%d,%d" % rect], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    assert out.returncode == 0, text
    printed = [json.loads(l) for l in text.splitlines() if l.startswith("{")]
    g = gpu_engine.Renderer(W, H, SD)
    try:
        g.set_asset_root(root)
        g.world_load_file("Content/World.json")
        g.set_id_capture(True)
        for f in range(2):
            g.world_update_uniforms(0.0, 0.0, 0.016 * f)
            g.render()
        hits, n = g.pick(*rect)
    finally:
        g.close()
    assert n > 0 and len(printed) == n
    for p, h in zip(printed, hits):
        assert (p["object"], p["instance"], p["pixels"], p["triangle"], p["x"], p["y"]) == tuple(int(h[k]) for k in
                                                                                              ("object", "instance", "pixels", "triangle", "x", "y"))
        assert np.float32(p["depth"]) == h["depth"]
