"""Moving instances between frames (zr_object_set_instances, zr_object_update_instances_async), bit for bit.

What an updated context draws must equal what a context built with the final instances draws: the work lists are rebuilt, the visibility
history, the bucket plan and the shadow flags are kept (the frame does not depend on them), and with two frames in flight an update
reaches only the frames enqueued after it.  Every comparison is exact.
"""
import numpy as np
import pytest

from parity_util import compare_all
from zeldaengine_amd import abi, dist as zdist, scenes

pytestmark = pytest.mark.gpu

W, H, SD, N = 320, 180, 512, 70000          # >= 65 536 instances: the instance-level work lists (k_cull_instances)
EYE, TARGET = np.array([12.0, -9.0, 7.0], np.float32), np.array([0.0, 0.0, 0.5], np.float32)
SPHERES = 1                                  # object index of the instanced spheres (add order: the plane is object 0)


def _instances():
    return scenes.generate_instances(N, 1.0, 14.0, 0.05, 0.2, seed=11)


def _scene(r, inst):
    r.set_cubemap(scenes.synthetic_cubemap(16))
    r.object_add(r.mesh_create(*scenes.grid_plane(40.0, 4, 0.0)))
    r.object_add(r.mesh_create(*scenes.uv_sphere(8, 5)), None, inst)


def _uniforms():
    w = scenes.sample_world()
    d, _, s = scenes.lights_from_world(w)
    w["PointLights"] = scenes.sample_point_lights(4)
    _, p, _ = scenes.lights_from_world(w)
    return abi.make_camera(tuple(EYE.tolist()), tuple(TARGET.tolist()), fov=50.0), d, p, s


def _frame(r, u):
    cam, d, p, s = u
    r.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
    r.render()


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
    if stats:
        assert a[3]["covered_pixels"] == b[3]["covered_pixels"], what


def _moves(inst, seed, frac=0.01):
    """About `frac` of the instances moved, turned and rescaled; one from outside the view into it, one from the view to behind the eye."""
    rng = np.random.default_rng(seed)
    new = inst.copy()
    fwd = (TARGET - EYE) / np.linalg.norm(TARGET - EYE)
    pos = inst["InstancePosition"]
    k_out = int(np.argmin((pos - EYE) @ fwd))                         # the farthest behind the eye: outside the frustum
    k_in = int(np.argmin(np.linalg.norm(pos[:, :2] - TARGET[:2], axis=1)))   # the nearest to the point looked at
    idx = rng.choice(len(inst), max(3, int(frac * len(inst))), replace=False)
    idx = np.unique(np.concatenate([idx, [k_out, k_in]])).astype(np.int64)
    new["InstancePosition"][idx, :2] += rng.normal(0.0, 0.6, (len(idx), 2)).astype(np.float32)
    new["InstanceRotation"][idx, 1] += rng.uniform(0.0, 3.0, len(idx)).astype(np.float32)
    new["InstancePScale"][idx] *= rng.uniform(0.6, 1.8, len(idx)).astype(np.float32)
    new["InstancePosition"][k_out] = TARGET + np.float32(0.25) * (EYE - TARGET)      # into view, near the middle of the screen
    new["InstancePScale"][k_out] = np.float32(0.6)
    new["InstancePosition"][k_in] = EYE - np.float32(2.0) * fwd                        # behind the eye
    return new, idx, k_out


@pytest.mark.parametrize("flags", [0, abi.FLAG_SHADOW_OCCLUSION, abi.FLAG_NO_HIZ])
def test_moved_instances_match_a_fresh_context(gpu_engine, flags):
    """Lists, plan and history stand (two frames), 1 % of the instances move with the camera and light still: the next frame equals a
    new context's.  A reused work list would miss the instance that moved into view and keep the one that left it."""
    inst, u = _instances(), _uniforms()
    a = gpu_engine.Renderer(W, H, SD, flags=flags)
    _scene(a, inst)
    for _ in range(2):
        _frame(a, u)
    before = _grab(a)
    assert before[3]["work_items"][1] >= 65536
    new, _, _ = _moves(inst, 5)
    a.object_set_instances(SPHERES, new)
    _frame(a, u)
    moved = _grab(a)
    _frame(a, u)
    again = _grab(a)
    a.close()
    b = gpu_engine.Renderer(W, H, SD, flags=flags)
    _scene(b, new)
    _frame(b, u)
    fresh = _grab(b)
    b.close()
    assert not np.array_equal(before[0], fresh[0])                   # the update shows
    _same(moved, fresh, "frame after the update")
    _same(again, fresh, "the frame after that")


def test_updates_through_both_forms_match_the_oracle(gpu_engine, oracle_lib):
    """A small instanced scene, updated through the host form and through the device form: every target equals the CPU oracle's
    frame of the final instances."""
    import torch
    cfg = scenes.config3(64, 256, 144)
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 256)
    gpu_engine.load_scene(g, cfg)
    g.render(); g.render()
    inst = cfg["objects"][0]["instances"]
    new = inst.copy()
    new["InstancePosition"][:8, 2] += np.float32(0.7)
    new["InstanceRotation"][:8, 0] += np.float32(0.4)
    g.object_set_instances(0, new[:8])
    sel = np.array([10, 20, 33, 63], np.int32)
    new["InstancePosition"][sel, :2] *= np.float32(0.5)
    new["InstancePScale"][sel] *= np.float32(1.5)
    dev = torch.device("cuda", 0)
    data = torch.from_numpy(new[sel].view(np.uint8).reshape(-1, 32).copy()).to(dev)
    idx = torch.from_numpy(sel).to(dev)
    torch.cuda.synchronize()
    g.object_update_instances_async(0, data, idx)
    g.render()
    g.finish()
    assert np.array_equal(g.object_get_instances(0)[1].view(np.uint8), new.view(np.uint8))
    cfg["objects"][0]["instances"] = new
    o = oracle_lib.Oracle(cfg["width"], cfg["height"], 256)
    oracle_lib.load_scene(o, cfg)
    o.render()
    assert o.covered_pixels() > 100
    diffs = compare_all(o, g)
    assert all(v == 0 for v in diffs.values()), diffs
    g.close()


@pytest.mark.parametrize("flags", [0, abi.FLAG_NO_CONE_CULL], ids=["culled", "no_cone_cull"])
def test_instances_turned_by_1e10_radians_match_the_oracle(gpu_engine, oracle_lib, flags):
    """Angles far outside zr_sincos's domain (|k| >= 2^31: a cast of k to int is undefined there, and x86 and gfx950 gave different
    quadrants) among ordinary instances, through zr_object_add (k_instance_prep) and through an update (k_instance_apply).  The sines
    are finite values of no meaning, so each such instance is scaled back to about its usual size; they cover pixels, and the frame equals the
    oracle's.

    Such a record is no rotation, and the culls' bounding-sphere and normal-cone tests take R for one (zr_cull.hip): they are skipped for it
    (zr_dev.h: is_rotation).  Before that the cone cull dropped meshlets that face the eye: 78 pixels of 36 864 differed with the culls on,
    none with the cone cull off - hence the two flag sets."""
    import ctypes as C
    cfg = scenes.config3(64, 256, 144)
    inst = cfg["objects"][0]["instances"]
    L = oracle_lib.lib()
    odd = {10: (1e10, 0.3, -0.2), 20: (0.1, -1e10, 0.0), 33: (0.0, 0.2, 5e9), 40: (3.4e9, 0.1, 0.2)}
    for k, e in odd.items():
        e = np.array(e, dtype=np.float32)
        r9 = np.zeros(9, dtype=np.float32)
        L.zo_kat_rotmat(e.ctypes.data_as(C.c_void_p), r9.ctypes.data_as(C.c_void_p))
        assert np.isfinite(r9).all() and np.abs(r9).max() > 10.0                 # far from a rotation
        inst["InstanceRotation"][k] = e
        inst["InstancePScale"][k] = np.float32(2.0) * inst["InstancePScale"][k] / np.abs(r9).max()
    start = inst.copy()
    start["InstanceRotation"][40] = (0.0, 0.0, 0.0)
    cfg["objects"][0]["instances"] = start
    g = gpu_engine.Renderer(cfg["width"], cfg["height"], 256, flags=flags)
    gpu_engine.load_scene(g, cfg)
    g.render(); g.render()
    g.object_set_instances(0, inst)                                              # instance 40 turns through k_instance_apply
    g.render()
    g.finish()
    cfg["objects"][0]["instances"] = inst
    o = oracle_lib.Oracle(cfg["width"], cfg["height"], 256)
    oracle_lib.load_scene(o, cfg)
    o.render()
    diffs = compare_all(o, g)
    assert all(v == 0 for v in diffs.values()), diffs
    g.close()
    hidden = inst.copy()
    hidden["InstancePScale"][list(odd)] = 0.0
    cfg["objects"][0]["instances"] = hidden
    p = oracle_lib.Oracle(cfg["width"], cfg["height"], 256)
    oracle_lib.load_scene(p, cfg)
    p.render()
    assert int((p.color() != o.color()).any(axis=2).sum()) > 20, "the turned instances cover no pixels: the case shows nothing"


def _step_range(inst, i):
    """Frame i's host-form update: a contiguous range of moved instances (a different one every frame)."""
    rng = np.random.default_rng(100 + i)
    first = int(rng.integers(0, N - 2000)); n = int(rng.integers(200, 2000))
    new = inst.copy()
    new["InstancePosition"][first:first + n, :2] += rng.normal(0.0, 0.8, (n, 2)).astype(np.float32)
    new["InstancePScale"][first:first + n] *= np.float32(1.0 + 0.05 * (i % 5))
    return new, first, n


def _step_sparse(inst, i):
    """Frame i's device-form update: scattered instances (one of them brought to the middle of the view every third frame)."""
    rng = np.random.default_rng(200 + i)
    idx = np.unique(rng.choice(N, 700, replace=False)).astype(np.int32)
    new = inst.copy()
    new["InstancePosition"][idx, :2] += rng.normal(0.0, 0.8, (len(idx), 2)).astype(np.float32)
    new["InstanceRotation"][idx, 2] += np.float32(0.3)
    if i % 3 == 0:
        new["InstancePosition"][idx[0]] = TARGET + np.float32(0.3) * (EYE - TARGET)
    return new, idx


def _serial_frames(gpu_engine, steps, flags):
    """The reference: one stream, the whole array set before every frame, finish() after it."""
    inst, u = _instances(), _uniforms()
    ref = gpu_engine.Renderer(W, H, SD, flags=flags | abi.FLAG_SERIAL_PASSES)
    _scene(ref, inst)
    want = []
    for new in steps:
        ref.object_set_instances(SPHERES, new)
        _frame(ref, u)
        ref.finish()
        want.append((ref.color().copy(), ref.shadowmap().view(np.uint32).copy()))
    assert ref.stats()["work_items"][0] >= 65536
    ref.close()
    return want


def _check_queued(got, want, SD_=SD):
    for i, (c, s) in enumerate(got):
        got_s = s.cpu().numpy().view(np.uint32).reshape(SD_, SD_)
        got_c = c.cpu().numpy().view(np.uint8).reshape(H, W, 4)
        assert np.array_equal(got_s, want[i][1]), "shadow map of queued frame %d: %d texels differ" % (i, int((got_s != want[i][1]).sum()))
        assert np.array_equal(got_c, want[i][0]), "colour of queued frame %d" % i


@pytest.mark.parametrize("flags", [0, abi.FLAG_SHADOW_OCCLUSION])
def test_host_updates_between_queued_frames(gpu_engine, flags):
    """14 frames back to back, each after a host-form update, copied out on the device; no finish() until all are enqueued.  Every frame
    equals the serial context's: an update reaches the frames after it and none before (two frames in flight, two instance planes)."""
    import torch
    FRAMES = 14
    inst, u = _instances(), _uniforms()
    steps, ranges, cur = [], [], inst
    for i in range(FRAMES):
        cur, first, n = _step_range(cur, i)
        steps.append(cur); ranges.append((first, n))
    want = _serial_frames(gpu_engine, steps, flags)
    g = gpu_engine.Renderer(W, H, SD, flags=flags)
    _scene(g, inst)
    dev = torch.device("cuda", 0)
    got = [(torch.zeros(W * H, dtype=torch.int32, device=dev), torch.zeros(SD * SD, dtype=torch.int32, device=dev)) for _ in range(FRAMES)]
    torch.cuda.synchronize()
    for i in range(FRAMES):
        first, n = ranges[i]
        g.object_set_instances(SPHERES, steps[i][first:first + n], first)
        _frame(g, u)
        g.copy_frame_async(got[i][0].data_ptr(), got[i][1].data_ptr())
    g.finish()
    assert g.stats()["overflow"] == 0
    _check_queued(got, want)
    assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), steps[-1].view(np.uint8))
    g.close()


def test_device_updates_from_a_torch_stream(gpu_engine):
    """As above, from torch tensors with an index list on a torch stream; after every call the tensors are overwritten on that stream
    (the library has read them by then, in that stream's order).  Out-of-range indices ride along and are ignored."""
    import torch
    FRAMES = 14
    inst, u = _instances(), _uniforms()
    steps, sparse, cur = [], [], inst
    for i in range(FRAMES):
        cur, idx = _step_sparse(cur, i)
        steps.append(cur); sparse.append(idx)
    want = _serial_frames(gpu_engine, steps, 0)
    g = gpu_engine.Renderer(W, H, SD)
    _scene(g, inst)
    dev = torch.device("cuda", 0)
    got = [(torch.zeros(W * H, dtype=torch.int32, device=dev), torch.zeros(SD * SD, dtype=torch.int32, device=dev)) for _ in range(FRAMES)]
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for i in range(FRAMES):
        idx = np.concatenate([sparse[i], np.array([N, N + 7, -1], np.int32)])          # the last three: >= the instance count
        vals = np.concatenate([steps[i][sparse[i]], np.zeros(3, abi.XkInstanceData)])
        with torch.cuda.stream(ts):
            d_idx = torch.from_numpy(idx).pin_memory().to(dev, non_blocking=True)
            d_val = torch.from_numpy(vals.view(np.uint8).reshape(-1, 32)).pin_memory().to(dev, non_blocking=True)
            g.object_update_instances_async(SPHERES, d_val, d_idx, stream=ts)
            d_val.fill_(0x7F)                                                          # overwritten behind the call, on its stream
            d_idx.fill_(3)
        _frame(g, u)
        g.copy_frame_async(got[i][0].data_ptr(), got[i][1].data_ptr())
    g.finish()
    ts.synchronize()
    assert g.stats()["overflow"] == 0
    _check_queued(got, want)
    assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), steps[-1].view(np.uint8))
    g.close()


def test_sparse_device_update_equals_a_full_host_update(gpu_engine):
    """An index-list update and zr_object_set_instances of the whole array with those entries changed give the same frame."""
    import torch
    inst, u = _instances(), _uniforms()
    new, idx, _ = _moves(inst, 9, 0.005)
    dev = torch.device("cuda", 0)
    frames = []
    for sparse in (True, False):
        g = gpu_engine.Renderer(W, H, SD)
        _scene(g, inst)
        _frame(g, u); _frame(g, u)
        if sparse:
            ix = np.concatenate([idx.astype(np.int32), np.array([N + 1000], np.int32)])
            vals = np.concatenate([new[idx], np.zeros(1, abi.XkInstanceData)])
            data = torch.from_numpy(vals.view(np.uint8).reshape(-1, 32).copy()).to(dev)
            torch.cuda.synchronize()
            g.object_update_instances_async(SPHERES, data, torch.from_numpy(ix).to(dev))
        else:
            g.object_set_instances(SPHERES, new)
        _frame(g, u)
        frames.append(_grab(g))
        assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), new.view(np.uint8))
        g.close()
    _same(frames[0], frames[1], "sparse against full")


def test_identity_queries_follow_moved_instances(gpu_engine):
    """An update leaves the scene as it is: the identity queries keep describing the last frame, and after the next frame pick finds the
    moved instance at its new place and the instance coverage adds up to the covered pixels."""
    inst, u = _instances(), _uniforms()
    g = gpu_engine.Renderer(W, H, SD)
    _scene(g, inst)
    g.set_id_capture(True)
    _frame(g, u); _frame(g, u)
    g.finish()
    cov_before = g.instance_coverage()
    new, _, k = _moves(inst, 3)
    g.object_set_instances(SPHERES, new)
    assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), new.view(np.uint8))
    # (no frame since the update: the queries answer for the frame before it, no ZR_ERR_STATE)
    assert np.array_equal(g.instance_coverage(), cov_before)
    g.pick(W // 2, H // 2)
    _frame(g, u)
    g.finish()
    hits, total = g.pick(W // 2, H // 2)
    assert total == 1 and (int(hits[0]["object"]), int(hits[0]["instance"])) == (SPHERES, k), hits
    cov = g.instance_coverage()
    assert int(cov.sum()) == g.stats()["covered_pixels"]
    base, _ = g.instance_slots()
    assert cov[base[SPHERES] + k] > 0
    g.close()


def test_bad_updates_are_refused_and_change_nothing(gpu_engine):
    """A non-instanced object, a range past the instance count, or a call between the stages of a frame: ZR_ERR_ARG / ZR_ERR_STATE,
    and the next frame is the frame without them."""
    import torch
    from zeldaengine_amd.engine import ZeldaRenderError
    inst, u = _instances(), _uniforms()
    g = gpu_engine.Renderer(W, H, SD)
    _scene(g, inst)
    _frame(g, u)
    moved = inst[:4].copy()
    moved["InstancePosition"][:, 2] += np.float32(3.0)
    dev = torch.device("cuda", 0)
    data = torch.from_numpy(moved.view(np.uint8).reshape(-1, 32).copy()).to(dev)
    torch.cuda.synchronize()
    for call, code in ((lambda: g.object_set_instances(0, moved), -1),                       # the plane: not instanced
                       (lambda: g.object_set_instances(SPHERES, moved, N - 3), -1),          # [N - 3, N + 1)
                       (lambda: g.object_set_instances(7, moved), -1),                       # no such object
                       (lambda: g.object_update_instances_async(0, data), -1),
                       (lambda: g.object_update_instances_async(SPHERES, data, first=N - 2), -1)):
        with pytest.raises(ZeldaRenderError) as e:
            call()
        assert e.value.code == code
    cam, d, p, s = u
    g.update_uniforms(cam, d, p, s, 0.0, 0.0, 1.0)
    g.render_shadow()
    for call in (lambda: g.object_set_instances(SPHERES, moved), lambda: g.object_update_instances_async(SPHERES, data)):
        with pytest.raises(ZeldaRenderError) as e:
            call()
        assert e.value.code == -6
    g.render_gbuffer(); g.render_lighting()
    _frame(g, u)
    got = _grab(g)
    assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), inst.view(np.uint8))
    g.close()
    b = gpu_engine.Renderer(W, H, SD)
    _scene(b, inst)
    _frame(b, u)
    # (images only: the statistics block of a frame that follows a staged frame counts differently, with or without updates)
    _same(got, _grab(b), "after refused updates", stats=False)
    b.close()


def test_rank_contexts_take_the_same_updates(gpu_engine):
    """tile_world = 2: every rank applies the same updates; its owned tiles equal the single context's frame."""
    inst, u = _instances(), _uniforms()
    new, _, _ = _moves(inst, 13)
    single = gpu_engine.Renderer(W, H, SD)
    _scene(single, inst)
    _frame(single, u); _frame(single, u)
    single.object_set_instances(SPHERES, new)
    _frame(single, u)
    want = _grab(single)[0]
    single.close()
    world = 2
    for r in range(world):
        g = gpu_engine.Renderer(W, H, SD, tile_rank=r, tile_world=world)
        _scene(g, inst)
        _frame(g, u); _frame(g, u)
        g.object_set_instances(SPHERES, new[:N // 2])
        g.object_set_instances(SPHERES, new[N // 2:], N // 2)
        _frame(g, u)
        g.finish()
        assert np.array_equal(g.read_tiles(), zdist.pack_tiles(want, r, world)), "rank %d" % r
        g.close()
