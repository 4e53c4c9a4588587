"""Hiding and showing instances and whole objects between frames (zr_object_set_visible, zr_object_set_instance_visibility,
zr_object_update_instance_visibility_async, zr_object_get_visibility), bit for bit.

What a context with hidden objects and instances draws must equal what a context built with only the shown ones, in the same order,
draws: the work lists are rebuilt and the kept shadow map is redrawn, the visibility history, the bucket plan and the shadow flags are
kept (the frame does not depend on them), and with two frames in flight a call reaches only the frames enqueued after it.  Every
comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

from parity_util import compare_all
from zeldaengine_amd import abi, dist as zdist, scenes

pytestmark = pytest.mark.gpu

EYE, TARGET = np.array([12.0, -9.0, 7.0], np.float32), np.array([0.0, 0.0, 0.5], np.float32)
PLANE, SPHERES = 0, 1                         # object indices (add order)


class Scene:
    """A plane and n instanced spheres."""

    def __init__(self, w, h, sd, n, sphere, rmax, smin, smax, seed):
        self.W, self.H, self.SD, self.N = w, h, sd, n
        self.sphere = scenes.uv_sphere(*sphere)
        self.plane = scenes.grid_plane(40.0, 4, 0.0)
        self.inst = scenes.generate_instances(n, 1.0, rmax, smin, smax, seed=seed)
        self.cube = scenes.synthetic_cubemap(16)
        w_ = scenes.sample_world()
        d, _, s = scenes.lights_from_world(w_)
        w_["PointLights"] = scenes.sample_point_lights(4)
        _, p, _ = scenes.lights_from_world(w_)
        self.u = (abi.make_camera(tuple(EYE.tolist()), tuple(TARGET.tolist()), fov=50.0), d, p, s)

    def populate(self, r, inst=None, plane=True, spheres=True):
        """inst: the spheres' instances (default: all of them); an empty array leaves the object out, like spheres=False."""
        inst = self.inst if inst is None else inst
        r.set_cubemap(self.cube)
        if plane:
            r.object_add(r.mesh_create(*self.plane))
        if spheres and len(inst):
            r.object_add(r.mesh_create(*self.sphere), None, inst)

    def renderer(self, eng, flags=0, **kw):
        return eng.Renderer(self.W, self.H, self.SD, flags=flags, **kw)

    def frame(self, r):
        cam, d, p, s = self.u
        r.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
        r.render()

    def fresh(self, eng, flags=0, setup=None, **kw):
        """One frame of a new context built from populate(**kw)."""
        b = self.renderer(eng, flags)
        self.populate(b, **kw)
        if setup:
            setup(b)
        self.frame(b)
        out = _grab(b)
        b.close()
        return out


# L: >= 65 536 instances, so that k_cull_instances builds work lists; S: several meshlets per instance (the local / nm decode of the
# meshlet-level cull, no work list), cheap for the oracle
L = Scene(320, 180, 512, 70000, (8, 5), 14.0, 0.05, 0.2, 11)
S = Scene(128, 72, 256, 300, (24, 13), 6.0, 0.2, 0.5, 5)
_MASKS = {}


def _grab(r):
    r.finish()
    st = r.stats()
    assert st["overflow"] == 0, st
    return r.color().copy(), [r.gbuffer(t).copy() for t in range(6)], r.shadowmap().view(np.uint32).copy(), st


def _same(a, b, what, stats=True):
    assert np.array_equal(a[0], b[0]), "%s: colour, %d pixels differ" % (what, int((a[0] != b[0]).any(axis=2).sum()))
    for t in range(6):
        assert np.array_equal(a[1][t].view(np.uint8), b[1][t].view(np.uint8)), "%s: GBuffer target %d" % (what, t)
    assert np.array_equal(a[2], b[2]), "%s: shadow map, %d texels differ" % (what, int((a[2] != b[2]).sum()))
    if stats:      # (work_items stays out: it counts hidden meshlet-instances too)
        assert a[3]["covered_pixels"] == b[3]["covered_pixels"], what
        assert a[3]["covered_shadow_texels"] == b[3]["covered_shadow_texels"], what


def _mask(eng, sc):
    """The shown instances (True) of the standard hidden set: hidden are the instances with nonzero coverage at an odd index and a
    seeded 30 % of the rest.  Found once per scene, from one frame with id capture."""
    if id(sc) not in _MASKS:
        g = sc.renderer(eng)
        sc.populate(g)
        g.set_id_capture(True)
        sc.frame(g)
        g.finish()
        base, _ = g.instance_slots()
        cov = g.instance_coverage()[base[SPHERES]:base[SPHERES] + sc.N]
        g.close()
        odd = (np.arange(sc.N) % 2) == 1
        hide = (cov > 0) & odd
        rest = np.flatnonzero(~hide)
        rng = np.random.default_rng(77)
        hide[rng.choice(rest, int(0.3 * len(rest)), replace=False)] = True
        assert ((cov > 0) & hide).any(), "no hidden instance had coverage"
        assert ((cov > 0) & ~hide).any()
        _MASKS[id(sc)] = (~hide, cov)
    return _MASKS[id(sc)][0].copy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


# ------------------------------------------------------------------------------------------------ 1. hidden == fresh, scene L

@pytest.mark.parametrize("flags", [0, abi.FLAG_SHADOW_OCCLUSION, abi.FLAG_NO_HIZ, abi.FLAG_NO_FRUSTUM_CULL | abi.FLAG_NO_CONE_CULL])
def test_hidden_instances_match_a_fresh_context(gpu_engine, flags):
    """Lists, plan, history and the kept map stand (two frames); the hidden set goes through the host form: the next frame and the one
    after it equal a new context's of the shown instances.  Everything shown again: the full scene's.  A reused work list would keep the
    hidden instances, a kept shadow map their shadows."""
    mask = _mask(gpu_engine, L)
    a = L.renderer(gpu_engine, flags)
    L.populate(a)
    for _ in range(2):
        L.frame(a)
    before = _grab(a)
    assert before[3]["work_items"][1] >= 65536
    a.object_set_instance_visibility(SPHERES, mask)
    L.frame(a)
    hidden = _grab(a)
    L.frame(a)
    again = _grab(a)
    ov, bytes_ = a.object_get_visibility(SPHERES)
    assert ov and np.array_equal(bytes_, mask.astype(np.uint8))
    assert np.array_equal(a.object_get_instances(SPHERES)[1].view(np.uint8), L.inst.view(np.uint8))      # hidden ones too
    a.object_set_instance_visibility(SPHERES, np.ones(L.N, np.uint8))
    L.frame(a)
    shown = _grab(a)
    L.frame(a)
    shown2 = _grab(a)
    a.close()
    fresh = L.fresh(gpu_engine, flags, inst=L.inst[mask])
    full = L.fresh(gpu_engine, flags)
    assert not np.array_equal(before[0], hidden[0])                  # the hide shows (a condition: the comparison is not vacuous)
    assert not np.array_equal(before[2], hidden[2])
    _same(hidden, fresh, "frame after the hide")
    _same(again, fresh, "the frame after that")
    _same(shown, full, "frame after showing everything")
    _same(shown2, full, "the frame after that")
    _same(before, full, "the warm frame")


# ------------------------------------------------------------------------------------------------ 2. both forms against the oracle, scene S

_ORACLES = {}


def _oracle_of_shown(oracle_lib, eng, forward):
    if forward not in _ORACLES:
        mask = _mask(eng, S)
        o = oracle_lib.Oracle(S.W, S.H, S.SD)
        S.populate(o, inst=S.inst[mask])
        o.set_shading(forward)
        cam, d, p, s = S.u
        o.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
        o.render()
        assert o.covered_pixels() > 100
        _ORACLES[forward] = o
    return _ORACLES[forward]


@pytest.mark.parametrize("forward", [False, True])
@pytest.mark.parametrize("form", ["host", "device"])
def test_both_forms_match_the_oracle(gpu_engine, oracle_lib, form, forward):
    """The hidden set through the host form, or through the device form - a torch tensor on a torch stream, the index list shuffled -:
    every target equals the CPU oracle's frame of the shown instances, in deferred shading and in the forward variant."""
    import torch
    mask = _mask(gpu_engine, S)
    g = S.renderer(gpu_engine)
    S.populate(g)
    g.set_shading(forward)
    S.frame(g); S.frame(g)
    if form == "host":
        g.object_set_instance_visibility(SPHERES, mask)
    else:
        dev = torch.device("cuda", 0)
        order = np.random.default_rng(3).permutation(S.N).astype(np.int32)
        ts = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            d_idx = torch.from_numpy(order).pin_memory().to(dev, non_blocking=True)
            d_vis = torch.from_numpy(mask[order].astype(np.uint8) * 255).pin_memory().to(dev, non_blocking=True)      # (any nonzero byte shows)
            g.object_update_instance_visibility_async(SPHERES, d_vis, d_idx, stream=ts)
            d_vis.fill_(1)                                             # overwritten behind the call, on its stream
            d_idx.fill_(0)
    S.frame(g)
    g.finish()
    assert np.array_equal(g.object_get_visibility(SPHERES)[1], mask.astype(np.uint8))
    diffs = compare_all(_oracle_of_shown(oracle_lib, gpu_engine, forward), g)
    assert all(v == 0 for v in diffs.values()), diffs
    g.close()


# ------------------------------------------------------------------------------------------------ 3. whole objects

def test_whole_objects_hide_and_show(gpu_engine):
    mask = _mask(gpu_engine, S)
    g = S.renderer(gpu_engine)
    S.populate(g)
    S.frame(g); S.frame(g)
    full = _grab(g)
    assert g.object_get_visibility(PLANE) == (True, None)
    g.object_set_visible(PLANE, False)
    S.frame(g)
    _same(_grab(g), S.fresh(gpu_engine, plane=False), "plane hidden")
    assert g.object_get_visibility(PLANE)[0] is False
    g.object_set_visible(PLANE, True)
    g.object_set_instance_visibility(SPHERES, mask)
    g.object_set_visible(SPHERES, False)
    S.frame(g)
    plane_only = S.fresh(gpu_engine, spheres=False)
    _same(_grab(g), plane_only, "spheres hidden")
    S.frame(g)
    _same(_grab(g), plane_only, "spheres hidden, second frame")
    ov, bytes_ = g.object_get_visibility(SPHERES)
    assert ov is False and np.array_equal(bytes_, mask.astype(np.uint8))          # the instance bytes are as left
    g.object_set_visible(SPHERES, True)
    S.frame(g)
    _same(_grab(g), S.fresh(gpu_engine, inst=S.inst[mask]), "spheres shown again, with their own bytes")
    g.object_set_visible(SPHERES, False)
    g.object_set_visible(PLANE, False)
    S.frame(g)
    nothing = _grab(g)                                                              # (zr_finish is ZR_OK in there)
    _same(nothing, S.fresh(gpu_engine, plane=False, spheres=False), "everything hidden")
    assert nothing[3]["covered_pixels"] == 0 and nothing[3]["covered_shadow_texels"] == 0
    g.object_set_visible(SPHERES, True)
    g.object_set_visible(PLANE, True)
    g.object_set_instance_visibility(SPHERES, np.ones(S.N, np.uint8))
    S.frame(g)
    _same(_grab(g), full, "everything back")
    g.close()


@pytest.mark.parametrize("flags", [0, abi.FLAG_SHADOW_OCCLUSION])
def test_every_instance_hidden_leaves_an_empty_work_list(gpu_engine, flags):
    """Scene L with every instance hidden through the per-instance form: work lists of length 0; with the plane hidden too, nothing
    survives at all and the frame is an empty context's."""
    g = L.renderer(gpu_engine, flags)
    L.populate(g)
    L.frame(g); L.frame(g)
    assert g.stats()["work_items"][1] >= 65536
    g.object_set_instance_visibility(SPHERES, np.zeros(L.N, np.uint8))
    L.frame(g)
    plane_only = L.fresh(gpu_engine, flags, spheres=False)
    _same(_grab(g), plane_only, "every instance hidden")
    L.frame(g)
    _same(_grab(g), plane_only, "every instance hidden, second frame")
    g.object_set_visible(PLANE, False)
    L.frame(g)
    _same(_grab(g), L.fresh(gpu_engine, flags, plane=False, spheres=False), "nothing survives")
    g.close()


# ------------------------------------------------------------------------------------------------ 4. frames in flight

FRAMES = 10


def _steps():
    """Frame i's visibility step and the state after it: ('host', first, bytes) | ('device', idx, bytes) | ('object', index, visible)."""
    steps, state = [], {"mask": np.ones(L.N, bool), "obj": [True, True]}
    for i in range(FRAMES):
        rng = np.random.default_rng(300 + i)
        if i in (3, 5):                                   # the two whole-object flips: the spheres go, and come back
            step = ("object", SPHERES, i == 5)
            state["obj"][SPHERES] = i == 5
        elif i % 2 == 0:
            first = int(rng.integers(0, L.N - 9000)); n = int(rng.integers(3000, 9000))
            if i % 4 == 2:                                # a re-show: the range of two steps ago, all of it
                _, first, old = steps[i - 2][0]
                vals = np.ones(len(old), np.uint8)
            else:
                vals = (rng.random(n) < 0.4).astype(np.uint8)
            step = ("host", first, vals)
            state["mask"][first:first + len(vals)] = vals != 0
        else:
            idx = np.unique(rng.choice(L.N, 6000, replace=False)).astype(np.int32)
            vals = (rng.random(len(idx)) < 0.5).astype(np.uint8)
            step = ("device", idx, vals)
            state["mask"][idx] = vals != 0
        steps.append((step, state["mask"].copy(), list(state["obj"])))
    return steps


@pytest.mark.parametrize("flags", [0, abi.FLAG_SHADOW_OCCLUSION])
def test_visibility_between_queued_frames(gpu_engine, flags):
    """10 frames back to back, a visibility step before each - host ranges, sparse device lists on a torch stream, two whole-object
    flips, some steps showing again -, copied out on the device, no finish() until all are enqueued.  Every frame equals the frame of a
    serial context that sets the whole state and finishes after every frame."""
    import torch
    steps = _steps()
    ref = L.renderer(gpu_engine, flags | abi.FLAG_SERIAL_PASSES)
    L.populate(ref)
    want = []
    for _, mask, obj in steps:
        ref.object_set_instance_visibility(SPHERES, mask)
        for k in (PLANE, SPHERES):
            ref.object_set_visible(k, obj[k])
        L.frame(ref)
        ref.finish()
        want.append((ref.color().copy(), ref.shadowmap().view(np.uint32).copy()))
    assert ref.stats()["work_items"][0] >= 65536
    ref.close()
    assert len({w[0].tobytes() for w in want}) >= FRAMES - 2            # the steps show
    g = L.renderer(gpu_engine, flags)
    L.populate(g)
    dev = torch.device("cuda", 0)
    got = [(torch.zeros(L.W * L.H, dtype=torch.int32, device=dev), torch.zeros(L.SD * L.SD, dtype=torch.int32, device=dev)) for _ in range(FRAMES)]
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for i, (step, _, _) in enumerate(steps):
        if step[0] == "object":
            g.object_set_visible(step[1], step[2])
        elif step[0] == "host":
            g.object_set_instance_visibility(SPHERES, step[2], step[1])
        else:
            idx = np.concatenate([step[1], np.array([L.N, L.N + 7, -1], np.int32)])          # the last three: >= the instance count
            vals = np.concatenate([step[2], np.zeros(3, np.uint8)])
            with torch.cuda.stream(ts):
                d_idx = torch.from_numpy(idx).pin_memory().to(dev, non_blocking=True)
                d_val = torch.from_numpy(vals).pin_memory().to(dev, non_blocking=True)
                g.object_update_instance_visibility_async(SPHERES, d_val, d_idx, stream=ts)
                d_val.fill_(0)                                                             # overwritten behind the call, on its stream
                d_idx.fill_(3)
        L.frame(g)
        g.copy_frame_async(got[i][0].data_ptr(), got[i][1].data_ptr())
    g.finish()
    ts.synchronize()
    assert g.stats()["overflow"] == 0
    for i, (c, s) in enumerate(got):
        got_s = s.cpu().numpy().view(np.uint32).reshape(L.SD, L.SD)
        got_c = c.cpu().numpy().view(np.uint8).reshape(L.H, L.W, 4)
        assert np.array_equal(got_s, want[i][1]), "shadow map of queued frame %d: %d texels differ" % (i, int((got_s != want[i][1]).sum()))
        assert np.array_equal(got_c, want[i][0]), "colour of queued frame %d" % i
    ov, bytes_ = g.object_get_visibility(SPHERES)
    assert ov == steps[-1][2][SPHERES] and np.array_equal(bytes_, steps[-1][1].astype(np.uint8))
    g.close()


# ------------------------------------------------------------------------------------------------ 5. moves and visibility together

def _moved(inst, sel, seed):
    rng = np.random.default_rng(seed)
    new = inst.copy()
    new["InstancePosition"][sel, :2] += rng.normal(0.0, 0.7, (len(sel), 2)).astype(np.float32)
    new["InstanceRotation"][sel, 1] += np.float32(0.8)
    new["InstancePScale"][sel] *= np.float32(1.4)
    return new


def test_moves_and_visibility_in_one_interval(gpu_engine):
    """Between two frames: set A moved then hidden, set B hidden (device form) then moved, set C - hidden already - moved, then shown.
    The frame equals a new context's of the final transforms and the final mask."""
    A, B, Cs = np.arange(1000, 3000), np.arange(20000, 22000), np.arange(40000, 42000)
    g = L.renderer(gpu_engine)
    L.populate(g)
    L.frame(g)
    hide_c = np.zeros(len(Cs), np.uint8)
    g.object_set_instance_visibility(SPHERES, hide_c, int(Cs[0]))
    L.frame(g); L.frame(g)
    before = _grab(g)
    new = _moved(_moved(_moved(L.inst, A, 1), B, 2), Cs, 3)
    d_zero = _dev(np.zeros(len(B), np.uint8))
    import torch
    torch.cuda.synchronize()
    g.object_set_instances(SPHERES, new[A], int(A[0]))
    g.object_set_instance_visibility(SPHERES, np.zeros(len(A), np.uint8), int(A[0]))
    g.object_update_instance_visibility_async(SPHERES, d_zero, first=int(B[0]))
    g.object_set_instances(SPHERES, new[B], int(B[0]))
    g.object_set_instances(SPHERES, new[Cs], int(Cs[0]))
    g.object_set_instance_visibility(SPHERES, np.ones(len(Cs), np.uint8), int(Cs[0]))
    L.frame(g)
    got = _grab(g)
    L.frame(g)
    again = _grab(g)
    mask = np.ones(L.N, bool)
    mask[A] = False; mask[B] = False
    assert np.array_equal(g.object_get_visibility(SPHERES)[1], mask.astype(np.uint8))
    assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), new.view(np.uint8))      # hidden ones moved too
    g.close()
    fresh = L.fresh(gpu_engine, inst=new[mask])
    assert not np.array_equal(before[0], got[0])
    _same(got, fresh, "moves and visibility in one interval")
    _same(again, fresh, "the frame after that")


# ------------------------------------------------------------------------------------------------ 6. identity

def test_identity_queries_skip_hidden_instances(gpu_engine):
    mask = _mask(gpu_engine, L)
    g = L.renderer(gpu_engine)
    L.populate(g)
    g.set_id_capture(True)
    L.frame(g); L.frame(g)
    g.finish()
    base, n_slots = g.instance_slots()
    cov_before = g.instance_coverage()
    ids_before = g.read_ids(abi.IDS_OBJECT)
    depth = g.gbuffer(0)
    sph = cov_before[base[SPHERES]:base[SPHERES] + L.N]
    k = int(np.flatnonzero((sph > 0) & ~mask)[0])                                  # visible now, hidden next
    own = (ids_before[..., 0] == SPHERES) & (ids_before[..., 1] == k)
    assert own.any()
    ys, xs = np.nonzero(own)
    j = int(np.argmin(depth[ys, xs]))                                              # its nearest pixel
    x, y = int(xs[j]), int(ys[j])
    hits, total = g.pick(x, y)
    assert total == 1 and (int(hits[0]["object"]), int(hits[0]["instance"])) == (SPHERES, k)
    g.object_set_instance_visibility(SPHERES, mask)
    # (no frame since the call: the queries answer for the frame before it, the scene did not change)
    assert np.array_equal(g.instance_coverage(), cov_before)
    assert np.array_equal(g.read_ids(abi.IDS_OBJECT), ids_before)
    assert g.pick(x, y)[1] == 1
    L.frame(g)
    g.finish()
    ids = g.read_ids(abi.IDS_OBJECT)
    won = ids[..., 0] == SPHERES
    assert won.any() and mask[ids[..., 1][won]].all(), "a hidden instance owns a pixel"
    cov = g.instance_coverage()
    assert len(cov) == n_slots and int(cov.sum()) == g.stats()["covered_pixels"]
    sph = cov[base[SPHERES]:base[SPHERES] + L.N]
    assert not sph[~mask].any()
    hits, total = g.pick(x, y)
    assert all((int(h["object"]), int(h["instance"])) != (SPHERES, k) for h in hits)
    g.close()
    b = L.renderer(gpu_engine)
    L.populate(b, inst=L.inst[mask])
    b.set_id_capture(True)
    L.frame(b)
    b.finish()
    base_b, _ = b.instance_slots()
    cov_b = b.instance_coverage()
    b.close()
    assert np.array_equal(sph[mask], cov_b[base_b[SPHERES]:base_b[SPHERES] + int(mask.sum())])
    assert cov[base[PLANE]] == cov_b[base_b[PLANE]]


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refused_calls_change_nothing_and_empty_calls_keep_the_map(gpu_engine):
    import torch
    from zeldaengine_amd.engine import ZeldaRenderError
    ARG, STATE = -1, -6
    g = S.renderer(gpu_engine)
    S.populate(g)
    some = np.zeros(4, np.uint8)
    d_some = _dev(some)
    d_idx = _dev(np.arange(8, dtype=np.int32))
    torch.cuda.synchronize()
    # a scene no frame has used yet: the host forms work (undone here), the device form has no device copy to write
    g.object_set_instance_visibility(SPHERES, some, 8)
    g.object_set_instance_visibility(SPHERES, np.ones(4, np.uint8), 8)
    with pytest.raises(ZeldaRenderError) as e:
        g.object_update_instance_visibility_async(SPHERES, d_some)
    assert e.value.code == STATE
    S.frame(g); S.frame(g)
    before = _grab(g)
    assert g.pass_times(1)["shadow"] == 0.0                                       # the map stands
    Lb, h = g.L, g.h
    vp = C.c_void_p
    refused = (
        (lambda: g.object_set_visible(7, False), ARG),                                     # no such object
        (lambda: g.object_set_instance_visibility(7, some), ARG),
        (lambda: g.object_update_instance_visibility_async(7, d_some), ARG),
        (lambda: g.object_get_visibility(7), ARG),
        (lambda: g.object_set_instance_visibility(PLANE, some[:1]), ARG),                  # the plane: not instanced
        (lambda: g.object_update_instance_visibility_async(PLANE, d_some[:1]), ARG),
        (lambda: g.object_set_instance_visibility(SPHERES, some, S.N - 3), ARG),           # [N - 3, N + 1)
        (lambda: g.object_update_instance_visibility_async(SPHERES, d_some, first=S.N - 2), ARG),
        (lambda: g._chk(Lb.zr_object_set_instance_visibility(h, SPHERES, 0, None, 4)), ARG),                       # n > 0, no buffer
        (lambda: g._chk(Lb.zr_object_update_instance_visibility_async(h, SPHERES, 0, None, None, 4, None)), ARG),
        (lambda: g._chk(Lb.zr_object_update_instance_visibility_async(h, SPHERES, 0, vp(d_idx.data_ptr() + 1), vp(d_some.data_ptr()), 4, None)), ARG),   # misaligned idx_dev
    )
    for i, (call, code) in enumerate(refused):
        with pytest.raises(ZeldaRenderError) as e:
            call()
        assert e.value.code == code, i
    cam, d, p, s = S.u
    g.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
    g.render_shadow()
    for call in (lambda: g.object_set_visible(SPHERES, False), lambda: g.object_set_instance_visibility(SPHERES, some),
                 lambda: g.object_update_instance_visibility_async(SPHERES, d_some)):
        with pytest.raises(ZeldaRenderError) as e:
            call()
        assert e.value.code == STATE
    g.render_gbuffer(); g.render_lighting()
    S.frame(g)
    # (images only: the statistics block of a frame that follows a staged frame counts differently, with or without these calls)
    _same(_grab(g), before, "after refused calls", stats=False)
    assert g.object_get_visibility(SPHERES)[0] is True and g.object_get_visibility(SPHERES)[1].all()
    # n == 0, and a zr_object_set_visible that flips nothing: ZR_OK, and the kept shadow map stays kept
    g.object_set_instance_visibility(SPHERES, np.zeros(0, np.uint8))
    g.object_update_instance_visibility_async(SPHERES, d_some[:0])
    g.object_update_instance_visibility_async(SPHERES, d_some[:0], d_idx[:0])
    g.object_set_visible(SPHERES, True)
    g.object_set_visible(PLANE, True)
    S.frame(g)
    _same(_grab(g), before, "after empty calls", stats=False)
    assert g.pass_times(1)["shadow"] == 0.0
    # a real hide does not leave it kept
    g.object_set_instance_visibility(SPHERES, some)
    S.frame(g)
    g.finish()
    assert g.pass_times(1)["shadow"] > 0.0
    S.frame(g)
    g.finish()
    assert g.pass_times(1)["shadow"] == 0.0
    g.object_set_visible(PLANE, False)
    S.frame(g)
    g.finish()
    assert g.pass_times(1)["shadow"] > 0.0
    g.close()


# ------------------------------------------------------------------------------------------------ 8. rank contexts

def test_rank_contexts_take_the_same_calls(gpu_engine):
    """tile_world = 2: every rank takes the same visibility calls; its owned tiles equal the single context's frame of that mask."""
    mask = _mask(gpu_engine, L)
    single = L.renderer(gpu_engine)
    L.populate(single)
    L.frame(single); L.frame(single)
    single.object_set_instance_visibility(SPHERES, mask)
    L.frame(single)
    want = _grab(single)
    single.close()
    world = 2
    for r in range(world):
        g = L.renderer(gpu_engine, tile_rank=r, tile_world=world)
        L.populate(g)
        L.frame(g); L.frame(g)
        g.object_set_instance_visibility(SPHERES, mask[:L.N // 2])
        g.object_set_instance_visibility(SPHERES, mask[L.N // 2:], L.N // 2)
        L.frame(g)
        g.finish()
        assert np.array_equal(g.read_tiles(), zdist.pack_tiles(want[0], r, world)), "rank %d" % r
        g.close()
    # the shadow pass split by i % world keeps using the full scene's instance index: the min of the two maps is the single map
    maps = []
    for r in range(world):
        g = L.renderer(gpu_engine)
        L.populate(g)
        g.set_shadow_partition(r, world)
        L.frame(g); L.frame(g)
        g.object_set_instance_visibility(SPHERES, mask)
        L.frame(g)
        g.finish()
        maps.append(g.shadowmap().copy())
        g.close()
    assert np.array_equal(np.minimum(maps[0], maps[1]).view(np.uint32), want[2])
