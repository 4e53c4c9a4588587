"""Casting rays into the scene of the last frame on the renderer (zr_raycast, zr_raycast_async, zr_camera_ray): bit for bit against the
host statement of the rule (zr_ray_triangles) where the scene is exact in float32, against the independent float64 statement
(tests/raycast_reference.py) where it is not, and through every state the scene can be in.  All frames are 96 x 64."""
import json
import math
import subprocess

import numpy as np
import pytest

import independent_geometry as ig
import raycast_cases as rcc
import raycast_reference as rr
from independent_scenes import Scene, _lights
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

W, H, SD = rcc.W, rcc.H, rcc.SD
MISS = 0xFFFFFFFF
CAM = abi.make_camera((7.0, -5.0, 4.5), (0.0, 0.5, 0.5), fov=50.0)


def _uniforms(r, cam=CAM, roll=0.0):
    d, p, sp = _lights(1, 2)
    r.update_uniforms(cam, d, p, sp, roll, 0.0, 0.0)


def _renderer(gpu_engine, scene, cam=CAM, roll=0.0, render=True, **kw):
    r = gpu_engine.Renderer(W, H, SD, **kw)
    scene.load(r)
    _uniforms(r, cam, roll)
    if render:
        r.render()
    return r


class World:
    """the scene as the test forms it itself: float32 world triangles in primitive-id order and who each belongs to"""

    def __init__(self, scene, roll=0.0):
        self.draws = rcc.draws_of(scene)
        self.model = ig.rotate_z(roll)
        self.tris = rcc.world_f32(self.draws, self.model)
        self.tris64, self.err, self.who = rr.world_triangles(self.draws, self.model)
        self.sizes = [len(d["idx"]) // 3 for d in self.draws for _ in range(1 if d["instances"] is None else len(d["instances"]))]

    def expect(self, engine, rays, flags=0, hidden=None):
        """zr_ray_triangles over the shown triangles, its records renamed (object, instance, triangle)"""
        keep = np.ones(len(self.tris), dtype=bool) if hidden is None else ~hidden
        h = engine.ray_triangles(rays, self.tris[keep], flags)
        m = h["object"] != MISS
        who = self.who[keep][h["triangle"][m]]
        h["object"][m], h["instance"][m], h["triangle"][m] = who[:, 0], who[:, 1], who[:, 2]
        return h

    def hidden(self, obj, inst=None):
        return (self.who[:, 0] == obj) & (True if inst is None else np.isin(self.who[:, 1], inst))

    def reference(self, rays, cull_back=False):
        return rr.cast(rays["origin"], rays["dir"], rays["t_min"], rays["t_max"], self.tris64, self.err, cull_back, groups=rr.groups_of(self.tris64, self.sizes))


def _same(got, want, what=""):
    if got.tobytes() != want.tobytes():
        k = int(np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(got, want)])[0][0])
        raise AssertionError("%s: record %d of %d differs: %r, the host statement %r" % (what, k, len(got), got[k], want[k]))


# ---- 1: bit-exact against the host statement

def test_raycast_equals_the_host_statement_in_every_byte(gpu_engine):
    scene = rcc.dyadic_scene()
    w = World(scene)
    # every world corner is one float32 rounding of an exact value - p * s is exact (a power of two), + t rounds once - whatever the
    # order of operations: the float32 chain gives the bits of the float64 chain rounded
    d = w.draws[2]
    assert d["instances"] is not None and w.who[-1, 0] == d["object"]
    p32 = np.asarray(d["verts"]["Position"], dtype=np.float32)[np.asarray(d["idx"], dtype=np.int64).reshape(-1, 3)]
    mine = np.concatenate([p32 * np.float32(i["InstancePScale"]) + i["InstancePosition"].astype(np.float32) for i in d["instances"]])
    assert mine.dtype == np.float32 and np.array_equal(mine, w.tris[-len(mine):]), "the scene is not exact in float32"
    rays = rcc.mixed_rays(np.random.default_rng(1), w.tris, 4096)
    r = _renderer(gpu_engine, scene)
    try:
        for flags in (0, abi.RAY_CULL_BACK, abi.RAY_ANY_HIT, abi.RAY_NO_BOUNDS):
            got, want = r.raycast(rays, flags), w.expect(gpu_engine, rays, flags)
            _same(got, want, "flags %d" % flags)
        n_hit, n_inv = int((want["flags"] & 1 != 0).sum()), int((want["flags"] & 4 != 0).sum())
        assert n_hit > 1500 and n_inv == 512 and (want["flags"] == 0).sum() > 500, (n_hit, n_inv)
    finally:
        r.close()


# ---- 2: bounds reject nothing they should not

def _to_world(points, inst, model):
    v = np.zeros(len(points), dtype=abi.XkVertex)
    v["Position"], v["Normal"] = points, (0.0, 0.0, 1.0)
    return rr.vertex_stage(v, inst, model, np.eye(4), np.eye(4))[1]


def _tangent_rays(rng, V, C, n, tangent=True):
    """n rays aimed exactly (t = 1, up to the float32 rounding of the direction) at points of V, each with the centre C of a sphere
    through it.  tangent: the origin lies on the plane through the vertex perpendicular to its radius - the ray touches the sphere
    there, the vertex is on the silhouette as the ray sees it.  A third run on, a third end at the vertex, a third begin there."""
    k = rng.integers(0, len(V), n)
    P, rad = V[k], V[k] - C[k]
    rad /= np.sqrt(np.sum(rad * rad, axis=1, keepdims=True))
    T = np.cross(rad, rng.normal(size=(n, 3)))
    T /= np.sqrt(np.sum(T * T, axis=1, keepdims=True))
    if not tangent:
        T = T * rng.uniform(0.0, 1.0, (n, 1)) + rad * rng.uniform(0.05, 1.0, (n, 1))
        T /= np.sqrt(np.sum(T * T, axis=1, keepdims=True))
    o = (P + T * rng.uniform(2.0, 12.0, n)[:, None]).astype(np.float32)
    rays = abi.make_rays(o, (P - o.astype(np.float64)).astype(np.float32), 0.0, np.inf)
    rays["t_max"][1::3] = 1.0
    rays["t_min"][2::3] = 1.0
    return rays


def _grazing_rays(rng, scene, model, meshlets, mverts, n):
    """The rays that graze the bounds, aimed exactly: at vertices of the spheres from origins on their tangent planes (every vertex of
    uv_sphere lies on the whole-mesh sphere, whose radius is its farthest vertex: the instance level's bound is touched), at the hull
    vertices of the meshlets - those at the meshlet sphere's radius - tangent to the MESHLET's sphere, and at hull vertices from any
    side.  meshlets, mverts: the renderer's own (mesh_get_meshlets)."""
    it = scene.items[0]
    pos = np.asarray(it["verts"]["Position"], dtype=np.float64)
    hull_p, hull_c = [], []
    for m in meshlets:
        mv = mverts[m["VertexOffset"]:m["VertexOffset"] + m["VertexCount"]]
        c = m["BoundsCenter"].astype(np.float64)
        dist = np.sqrt(np.sum((pos[mv] - c) ** 2, axis=1))
        on = mv[dist >= 0.999 * dist.max()]
        hull_p.append(pos[on]); hull_c.append(np.tile(c, (len(on), 1)))
    hull_p, hull_c = np.concatenate(hull_p), np.concatenate(hull_c)
    centre = 0.5 * (pos.min(axis=0) + pos.max(axis=0))
    V, C, HV, HC = [], [], [], []
    for inst in it["instances"]:
        V.append(_to_world(pos, inst, model)); C.append(np.tile(_to_world(centre[None], inst, model), (len(pos), 1)))
        HV.append(_to_world(hull_p, inst, model)); HC.append(_to_world(hull_c, inst, model))
    V, C, HV, HC = (np.concatenate(a) for a in (V, C, HV, HC))
    a = n // 3
    return np.concatenate([_tangent_rays(rng, V, C, a), _tangent_rays(rng, HV, HC, a), _tangent_rays(rng, HV, HC, n - 2 * a, tangent=False)])


def test_bounds_reject_nothing_and_both_arms_hold_to_the_reference(gpu_engine):
    """4 096 rays: a third at triangle interiors, a third grazing the bounds - aimed exactly at silhouette and meshlet-hull vertices,
    tangent to the whole-mesh and the meshlet spheres - a third random.  All of them: the same bytes with and without
    ZR_RAY_NO_BOUNDS (also with BACK hits culled), and ZR_RAY_ANY_HIT's bit the nearest-hit form's.  Those comparisons need no
    reference, so the grazing aims are exact.  The float64 reference cannot decide a ray aimed at a vertex: it is held to on the other
    two thirds, the decidable rays, with its cap of 1 % of them excused."""
    scene, roll = rcc.general_scene(), 0.3
    w = World(scene, roll)
    rng = np.random.default_rng(4)
    r = _renderer(gpu_engine, scene, roll=roll)
    try:
        meshlets, mverts, _ = r.mesh_get_meshlets(0)
        assert len(meshlets) >= 2
        decidable = np.concatenate([rcc.rays_at_triangles(rng, w.tris64, 1366), abi.make_rays(rng.uniform(-9, 9, (1365, 3)), rng.normal(size=(1365, 3)), 0.0, np.inf)])
        rays = np.concatenate([decidable, _grazing_rays(rng, scene, w.model, meshlets, mverts, 1365)])
        assert len(rays) == 4096
        bounded, unbounded = r.raycast(rays), r.raycast(rays, abi.RAY_NO_BOUNDS)
        _same(bounded, unbounded, "with and without ZR_RAY_NO_BOUNDS")
        for flags in (abi.RAY_ANY_HIT, abi.RAY_ANY_HIT | abi.RAY_NO_BOUNDS):
            anyh = r.raycast(rays, flags)
            assert np.array_equal(anyh["flags"], bounded["flags"] & 1) and (anyh["object"] == MISS).all()
        _same(r.raycast(rays, abi.RAY_CULL_BACK), r.raycast(rays, abi.RAY_CULL_BACK | abi.RAY_NO_BOUNDS), "culled, with and without bounds")
    finally:
        r.close()
    graze = bounded[len(decidable):]
    print("grazing rays: %d of %d hit" % (int((graze["flags"] & 1).sum()), len(graze)))
    assert 100 < (graze["flags"] & 1).sum() < len(graze)                 # (they are on the edge: some hit, some pass)
    ref = w.reference(decidable)
    n_amb, worst, bad = rr.compare(ref, bounded[:len(decidable)], w.who)
    print("zr_raycast vs float64: %d of %d rays ambiguous, %d hits, largest error / bound ratio %.4f" % (n_amb, len(decidable), int((ref["prim"] >= 0).sum()), worst))
    assert not bad, bad[:5]
    assert n_amb <= len(decidable) // 100
    assert int((ref["prim"] >= 0).sum()) >= 1366                       # (the interior third was aimed at triangles)


# ---- 3: camera rays meet the winner plane

def _solid(prim):
    """pixels whose 3 x 3 neighbourhood holds one value (the frame's border excluded)"""
    ok = np.zeros(prim.shape, dtype=bool)
    c = prim[1:-1, 1:-1]
    ok[1:-1, 1:-1] = np.all([prim[1 + dy:prim.shape[0] - 1 + dy, 1 + dx:prim.shape[1] - 1 + dx] == c for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    return ok


def test_camera_rays_meet_the_winner_plane(gpu_engine):
    scene, cam = rcc.camera_scene(), rcc.camera_of_scene()
    r = _renderer(gpu_engine, scene, cam, render=False)
    try:
        r.set_id_capture(True)
        r.render()
        prim, obj = r.read_ids(abi.IDS_PRIMITIVE), r.read_ids(abi.IDS_OBJECT)
        solid = _solid(prim) & _solid(obj[..., 0]) & _solid(obj[..., 1])
        inside, empty = solid & (prim != MISS), solid & (prim == MISS)
        assert inside.sum() >= (prim != MISS).sum() // 4 and empty.sum() > 0, (int(inside.sum()), int((prim != MISS).sum()), int(empty.sum()))
        ys, xs = np.nonzero(inside | empty)
        rays = np.concatenate([r.camera_ray(x + 0.5, y + 0.5) for x, y in zip(xs, ys)])
        assert (rays["t_min"] == 0.0).all() and (rays["t_max"] == 1.0).all()
        hits = r.raycast(rays)
        w = World(scene)
        for h, x, y in zip(hits, xs, ys):
            if prim[y, x] == MISS:
                assert h["flags"] == 0 and h["object"] == MISS, "pixel (%d, %d) is empty, the ray hits %r" % (x, y, h)
                continue
            want = tuple(int(v) for v in w.who[prim[y, x]])
            assert (int(h["object"]), int(h["instance"]), int(h["triangle"])) == want == (int(obj[y, x, 0]), int(obj[y, x, 1]), want[2]), (x, y, h, want)
            assert h["flags"] == 1 and 0.0 < h["t"] < 1.0, (x, y, h)
        # the ray itself: origin on the near plane, origin + dir on the far plane, through the pixel centre (float64 from the uniforms)
        fu = ig.frame_uniforms(cam, *_lights(1, 2)[:2], W, H)["cam"]
        pv = fu["Proj"] @ fu["View"]
        for k in (0, len(rays) // 2, len(rays) - 1):
            for t, depth in ((0.0, 0.0), (1.0, 1.0)):
                p = pv @ np.append(rays[k]["origin"].astype(np.float64) + t * rays[k]["dir"].astype(np.float64), 1.0)
                ndc = p[:3] / p[3]
                assert abs((ndc[0] + 1) * W / 2 - (xs[k] + 0.5)) < 1e-2 and abs((ndc[1] + 1) * H / 2 - (ys[k] + 0.5)) < 1e-2 and abs(ndc[2] - depth) < 1e-4
    finally:
        r.close()


# ---- 4: scene state

def _probe_rays(w, n=600, seed=9):
    return rcc.mixed_rays(np.random.default_rng(seed), w.tris, n - n % 8)


def test_hidden_objects_and_instances_are_passed_through(gpu_engine):
    scene = rcc.dyadic_scene()
    w = World(scene)
    rays = _probe_rays(w)
    r = _renderer(gpu_engine, scene, render=False)
    try:
        r.object_set_visible(2, False)                                  # the box
        vis = np.ones(6, dtype=np.uint8)
        vis[[0, 3]] = 0
        r.object_set_instance_visibility(1, vis)
        r.render()
        hidden = w.hidden(2) | w.hidden(1, [0, 3])
        want = w.expect(gpu_engine, rays, 0, hidden)
        _same(r.raycast(rays), want, "hidden")
        assert not np.array_equal(want, w.expect(gpu_engine, rays)), "the rays do not tell the hidden scene from the whole one"
        r.object_set_visible(0, False); r.object_set_visible(1, False)
        _same(r.raycast(rays), want, "hiding takes effect with the next frame")
        r.render()
        got = r.raycast(rays)
        assert (got["object"] == MISS).all() and set(np.unique(got["flags"])) <= {0, 4}, "a scene whose every draw is hidden gives all misses"
    finally:
        r.close()


def _moved_scene():
    """the dyadic scene after the three updates: instances 1 and 4 moved and rescaled, the box's vertices doubled, instance 2 hidden"""
    s = rcc.dyadic_scene()
    inst = s.items[1]["instances"].copy()
    inst["InstancePosition"][1] = (0.5, 0.25, 1.25)
    inst["InstancePScale"][1] = 2.0
    inst["InstancePosition"][4] = (-1.25, 2.5, 0.5)
    s.items[1]["instances"] = inst
    v = s.items[2]["verts"].copy()
    v["Position"] = v["Position"] * np.float32(2.0) - np.float32(0.5)
    s.items[2]["verts"] = v
    return s


@pytest.mark.parametrize("device_form", [False, True], ids=["host_forms", "device_forms"])
def test_updates_take_effect_with_the_next_frame(gpu_engine, device_form):
    import torch
    old_scene, new_scene = rcc.dyadic_scene(), _moved_scene()
    w_old, w_new = World(old_scene), World(new_scene)
    rays = _probe_rays(w_old, 800, seed=13)
    r = _renderer(gpu_engine, old_scene)
    fresh = None
    try:
        before = w_old.expect(gpu_engine, rays)
        _same(r.raycast(rays), before, "before")
        inst, verts = new_scene.items[1]["instances"], new_scene.items[2]["verts"]
        vis = np.ones(6, dtype=np.uint8)
        vis[2] = 0
        keep = []
        if device_form:
            for a in (inst, verts, vis):
                keep.append(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda())
            torch.cuda.synchronize()
            r.object_update_instances_async(1, keep[0])
            r.mesh_update_vertices_async(2, keep[1])
            r.object_update_instance_visibility_async(1, keep[2])
        else:
            r.object_set_instances(1, inst)
            r.mesh_set_vertices(2, verts)
            r.object_set_instance_visibility(1, vis)
        _same(r.raycast(rays), before, "the old frame's answers until the next zr_render")
        r.render()
        after = w_new.expect(gpu_engine, rays, 0, w_new.hidden(1, [2]))
        assert not np.array_equal(after, before)
        _same(r.raycast(rays), after, "after the next frame")
        r.render(); r.render()                                          # the third frame on of unchanged inputs: a resting frame
        _same(r.raycast(rays), after, "on a resting frame")
        fresh = _renderer(gpu_engine, new_scene, render=False)
        fresh.object_set_instance_visibility(1, vis)
        fresh.render()
        _same(fresh.raycast(rays), after, "a fresh context")
    finally:
        r.close()
        if fresh is not None:
            fresh.close()


# ---- 5: sizes where the kernel can go wrong

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ray_counts(gpu_engine, n):
    scene = rcc.dyadic_scene()
    w = World(scene)
    rays = rcc.mixed_rays(np.random.default_rng(n), w.tris, 4104)[:n]
    r = _renderer(gpu_engine, scene)
    try:
        _same(r.raycast(rays), w.expect(gpu_engine, rays), "n = %d" % n)
    finally:
        r.close()


def _row_scene(n=300):
    s = Scene()
    s.add(rcc.sphere(), None, rcc.instances([(0.5 * k, 0.0, 1.0) for k in range(n)], None, np.where(np.arange(n) % 2 == 0, 1.0, 0.5)))
    return s


def test_a_ray_down_a_row_of_300_instances(gpu_engine):
    """every instance's sphere is met by the ray: the list of candidates overflows its batch and is drained on the way"""
    scene = _row_scene()
    w = World(scene)
    o = [(-3.0, 0.0, 1.0), (160.0, 0.0, 1.0), (-3.0, 0.0625, 1.125), (-3.0, 0.0, 1.0), (40.0, 0.25, 9.0)]
    d = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, -0.03125, -1.0)]
    rays = abi.make_rays(o, d, [0.0, 0.0, 0.0, 30.3125, 0.0], np.inf)
    r = _renderer(gpu_engine, scene, abi.make_camera((75.0, -120.0, 40.0), (75.0, 0.0, 1.0), fov=60.0, zfar=400.0))
    try:
        for flags in (0, abi.RAY_NO_BOUNDS, abi.RAY_CULL_BACK, abi.RAY_ANY_HIT):
            want = w.expect(gpu_engine, rays, flags)
            _same(r.raycast(rays, flags), want, "the row, flags %d" % flags)
        assert want["flags"][:4].all()
        first = w.expect(gpu_engine, rays)
        assert first["instance"][0] == 0 and first["instance"][1] == 299 and first["instance"][3] > 100
        vis = np.ones(300, dtype=np.uint8)
        vis[0] = 0
        r.object_set_instance_visibility(0, vis)
        r.render()
        want = w.expect(gpu_engine, rays, 0, w.hidden(0, [0]))
        _same(r.raycast(rays), want, "the row with the nearest hidden")
        assert want["instance"][0] == 1
    finally:
        r.close()


def test_two_coincident_instances_tie_to_the_lower_primitive_id(gpu_engine):
    s = Scene()
    s.add(rcc.sphere(), None, rcc.instances([(0.0, 0.0, 1.0), (0.0, 0.0, 1.0), (2.0, 0.0, 1.0)]))
    w = World(s)
    rays = rcc.rays_at_triangles(np.random.default_rng(6), w.tris[:224], 64)
    r = _renderer(gpu_engine, s)
    try:
        want = w.expect(gpu_engine, rays)
        assert (want["instance"] != 1).all() and (want["instance"] == 0).sum() > 50 and (want["flags"] == 1).sum() > 50
        for k in range(10):
            _same(r.raycast(rays), want, "call %d" % k)
    finally:
        r.close()


def test_sick_records_among_healthy_ones(gpu_engine):
    """an instance with NaN rotation, one with scale 0 and a mesh with a non-finite vertex: the healthy ones answer as if the others were
    absent, and the call returns"""
    pos = [(0.0, 0.0, 1.0), (1.5, 0.0, 1.0), (3.0, 0.0, 1.0), (4.5, 0.0, 1.0)]
    rot = np.zeros((4, 3), dtype=np.float32)
    rot[1, 0] = np.nan
    scale = np.array([1.0, 1.0, 0.0, 1.0], dtype=np.float32)
    healthy, sick = Scene(), Scene()
    healthy.add(rcc.sphere(), None, rcc.instances([pos[0], pos[3]]))
    sick.add(rcc.sphere(), None, rcc.instances(pos, rot, scale))
    bv, bi = scenes.box((0.5, 0.5, 0.5), (0.0, 3.0, 0.5))
    for s in (healthy, sick):
        s.add((bv, bi))
    broken = bv.copy()
    broken["Position"] = broken["Position"] + np.float32(4.0)
    broken["Position"][3, 1] = np.inf
    sick.add((broken, bi))
    wh = World(healthy)
    rays = np.concatenate([rcc.rays_at_triangles(np.random.default_rng(8), wh.tris, 192),
                           abi.make_rays([(-2.0, 0.0, 1.0), (1.5, -4.0, 1.0), (3.0, -4.0, 1.0), (4.0, 0.0, 4.5)], [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)])])
    want = wh.expect(gpu_engine, rays)
    want["instance"][(want["object"] == 0) & (want["instance"] == 1)] = 3
    r = _renderer(gpu_engine, sick)
    try:
        for flags in (0, abi.RAY_NO_BOUNDS):
            got = r.raycast(rays, flags)
            on_broken = got["object"] == 2                               # (the broken box's finite triangles may be hit: not what is asked here)
            _same(got[~on_broken], want[~on_broken], "flags %d" % flags)
            assert on_broken.sum() <= 8
    finally:
        r.close()


# ---- 6: frames in flight

def test_raycast_async_with_frames_in_flight(gpu_engine):
    import torch
    scene = rcc.dyadic_scene()
    w = World(scene)
    rays = _probe_rays(w, 512, seed=17)
    moved = rcc.dyadic_scene()
    inst = moved.items[1]["instances"].copy()
    inst["InstancePosition"] += np.float32(0.5)
    moved.items[1]["instances"] = inst
    w_moved = World(moved)
    r = _renderer(gpu_engine, scene)
    try:
        r.finish()
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
        d_hits = [torch.full((len(rays) * 48,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        r.render()                                                       # (a frame in flight ahead of the cast)
        r.raycast_async(d_rays.data_ptr(), d_hits[0].data_ptr(), len(rays))
        r.object_set_instances(1, inst)
        r.render(); r.render()                                           # no synchronisation between
        r.raycast_async(d_rays.data_ptr(), d_hits[1].data_ptr(), len(rays))
        r.finish()
        torch.cuda.synchronize()
        first, second = (h.cpu().numpy().view(abi.RAY_RECORD) for h in d_hits)
        _same(first, w.expect(gpu_engine, rays), "the first frame's scene")
        _same(second, w_moved.expect(gpu_engine, rays), "the moved scene")
        assert not np.array_equal(first, second)
    finally:
        r.close()


# ---- 7: refusals

def test_refusals_leave_the_context_as_it_was(gpu_engine):
    import torch
    scene = rcc.dyadic_scene()
    w = World(scene)
    rays = _probe_rays(w, 64, seed=19)
    hits = np.zeros(len(rays), dtype=abi.RAY_RECORD)
    r, twin = _renderer(gpu_engine, scene, render=False), _renderer(gpu_engine, scene, render=False)
    L = r.L
    dev = torch.zeros(len(rays) * 48 + 64, dtype=torch.uint8, device="cuda")
    p = dev.data_ptr()
    assert p % 16 == 0

    def host(n=len(rays), flags=0, rp=rays.ctypes.data, hp=hits.ctypes.data, nbytes=None):
        return L.zr_raycast(r.h, rp, n, flags, hp, n * 48 if nbytes is None else nbytes)

    def device(n=len(rays), flags=0, rp=p, hp=p):
        return L.zr_raycast_async(r.h, rp, n, flags, hp)
    try:
        # ZR_ERR_ARG comes first, whatever the state
        assert host(rp=None) == host(hp=None) == host(nbytes=47) == host(flags=8) == host(n=(1 << 24) + 1, nbytes=0) == abi.ERR_ARG
        assert device(rp=None) == device(hp=None) == device(rp=p + 4) == device(hp=p + 8) == device(flags=16) == device(n=(1 << 24) + 1) == abi.ERR_ARG
        # ZR_ERR_STATE: no frame yet - also for no rays at all
        assert host() == device() == host(n=0) == device(n=0) == abi.ERR_STATE
        r.render_shadow()
        assert host() == device() == abi.ERR_STATE                      # between the stages, before any frame
        r.render_gbuffer(); r.render_lighting()
        assert host() == 0 and host(n=0) == 0 and device(n=0) == 0 and host(n=0, rp=None, hp=None) == 0
        _same(hits, w.expect(gpu_engine, rays), "after the staged frame")
        r.render_shadow()
        assert host() == device() == abi.ERR_STATE and b"no finished frame" in L.zr_last_error(r.h)     # (ids_ready's wording: a frame between its stages is not finished)
        r.render_gbuffer(); r.render_lighting()
        r.object_add(r.mesh_create(*scenes.box()))
        assert host() == device() == abi.ERR_STATE and b"scene changed" in L.zr_last_error(r.h)
        r.render()
        assert host() == 0
        r.resize(W + 32, H)
        assert host() == device() == abi.ERR_STATE and b"no finished frame" in L.zr_last_error(r.h)
        r.resize(W, H)
        # the twin saw none of this but the frames and the added box: the same bytes afterwards
        for _ in range(3):
            twin.render()
        twin.object_add(twin.mesh_create(*scenes.box()))
        twin.render()
        r.render(); twin.render()
        assert np.array_equal(r.color(), twin.color())
    finally:
        r.close(); twin.close()


def test_a_rank_context_answers_like_the_single_context(gpu_engine):
    scene = rcc.dyadic_scene()
    w = World(scene)
    rays = _probe_rays(w, 512, seed=23)
    single, rank = _renderer(gpu_engine, scene), _renderer(gpu_engine, scene, tile_rank=1, tile_world=2)
    try:
        want = w.expect(gpu_engine, rays)
        _same(single.raycast(rays), want, "single")
        _same(rank.raycast(rays), want, "rank 1 of 2")
    finally:
        single.close(); rank.close()


# ---- 8: the tool

def test_headless_raycast_prints_what_the_renderer_returns(gpu_engine, tmp_path):
    from test_gpu_native_host import H as NH, SD as NSD, W as NW, _content_tree
    from zeldaengine_amd import build as zbuild
    root = str(tmp_path)
    _content_tree(root)
    exe = zbuild.build_headless()
    g = gpu_engine.Renderer(NW, NH, NSD)
    try:
        g.set_asset_root(root)
        g.world_load_file("Content/World.json")
        g.set_id_capture(True)
        for f in range(2):
            g.world_update_uniforms(0.0, 0.0, 0.016 * f)
            g.render()
        prim = g.read_ids(abi.IDS_PRIMITIVE)
        ys, xs = np.nonzero(_solid(prim) & (prim != MISS))
        assert len(xs)
        x, y = int(xs[len(xs) // 2]), int(ys[len(xs) // 2])
        ray = g.camera_ray(x + 0.5, y + 0.5)
        h = g.raycast(ray)[0]
    finally:
        g.close()
    out = subprocess.run([exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (NW, NH), "--shadow", str(NSD), "--frames", "2",
                          "--raycast", "%d,%d" % (x, y)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    assert out.returncode == 0, text
    printed = [json.loads(l) for l in text.splitlines() if l.startswith("{")]
    assert len(printed) == 1 and h["flags"] & 1
    p = printed[0]
    assert (p["hit"], p["object"], p["instance"], p["triangle"], p["x"], p["y"], p["back"]) == (1, int(h["object"]), int(h["instance"]), int(h["triangle"]), x, y,
                                                                                                 int(h["flags"] >> 1) & 1)
    assert np.float32(p["t"]) == h["t"] and np.float32(p["u"]) == h["u"] and np.float32(p["v"]) == h["v"]
    assert [np.float32(v) for v in p["normal"]] == list(h["normal"])
    pos = ray[0]["origin"].astype(np.float64) + float(h["t"]) * ray[0]["dir"].astype(np.float64)
    assert np.allclose(p["position"], pos, rtol=0, atol=1e-6 * (1.0 + np.abs(pos).max()))
    assert math.isfinite(p["t"])
