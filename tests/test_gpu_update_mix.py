"""Every kind of between-frames update in one gap between frames (csrc/zr_update.cpp): instances, instance visibility, vertices, a texture
and a whole object's visibility share one staging ring, one pair of events and one frame head.

Seven host-form updates between two frames - more than the ring's four slots, so a slot is waited for and reused, and one of them (a
192 x 192 image, 147 456 bytes: the smallest square above a slot's first capacity of 4 096 x 32 bytes) re-makes its slot - then one
device-form update of each kind on a side stream.  After each group two frames are rendered back to back with no finish() between them,
and both must equal a fresh context's frame of the final values: the first in colour and shadow map (copied out on the device: its
GBuffer copy is the other parity's and cannot be read back once the second frame is enqueued), the second in colour, all six targets
and the shadow map.  Every comparison is exact, and the read-backs return the values sent.
"""
import numpy as np
import pytest

from test_gpu_instance_update import _frame, _grab, _same, _uniforms
from test_gpu_mesh_update import _deform_sphere, _deform_terrain, _dev as _dev_verts
from test_gpu_texture_update import _dev as _dev_image, _variant
from zeldaengine_amd import abi, scenes

pytestmark = pytest.mark.gpu

W, H, SD, N, DIM = 96, 64, 128, 300, 192
PLANE, TERRAIN, SPHERES = 0, 1, 2            # object indices and mesh ids alike (creation order)


def _image():
    return scenes.synthetic_material(DIM)[0]


def _scene(r, state):
    """state: instances, instance mask, terrain vertices, sphere vertices, slot-0 image, plane shown"""
    inst, mask, tv, sv, img, plane = state
    r.set_cubemap(scenes.synthetic_cubemap(16))
    r.object_add(r.mesh_create(*scenes.grid_plane(40.0, 4, 0.0)))
    r.object_add(r.mesh_create(tv, scenes.grid_plane(12.0, 48, 0.02)[1]))
    m, keep = abi.make_material([img, None, None, None, None, None, None])
    r.object_add(r.mesh_create(sv, scenes.uv_sphere(8, 5)[1]), m, inst)
    return keep


def _fresh(gpu_engine, state, u):
    b = gpu_engine.Renderer(W, H, SD)
    keep = _scene(b, state)
    b.object_set_instance_visibility(SPHERES, state[1])
    b.object_set_visible(PLANE, state[5])
    _frame(b, u)
    out = _grab(b)
    b.close()
    del keep
    return out


def _two_frames(g, u, fresh, what):
    """Two frames back to back; both against `fresh`"""
    import torch
    dev = torch.device("cuda", 0)
    c0, s0 = torch.zeros(W * H, dtype=torch.int32, device=dev), torch.zeros(SD * SD, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _frame(g, u)
    g.copy_frame_async(c0.data_ptr(), s0.data_ptr())
    _frame(g, u)
    second = _grab(g)
    first_c, first_s = c0.cpu().numpy().view(np.uint8).reshape(H, W, 4), s0.cpu().numpy().view(np.uint32).reshape(SD, SD)
    assert np.array_equal(first_s, fresh[2]), "%s, first frame: shadow map, %d texels differ" % (what, int((first_s != fresh[2]).sum()))
    assert np.array_equal(first_c, fresh[0]), "%s, first frame: colour, %d pixels differ" % (what, int((first_c != fresh[0]).any(axis=2).sum()))
    _same(second, fresh, what + ", second frame")
    return second


def _check_readbacks(g, state, what):
    inst, mask, tv, sv, img, plane = state
    assert np.array_equal(g.object_get_instances(SPHERES)[1].view(np.uint8), inst.view(np.uint8)), what + ": instances"
    shown, vis = g.object_get_visibility(SPHERES)
    assert shown and np.array_equal(vis, mask), what + ": instance visibility"
    assert g.object_get_visibility(PLANE)[0] == plane, what + ": the plane's visibility"
    assert np.array_equal(g.mesh_get_vertices(TERRAIN).view(np.uint8), tv.view(np.uint8)), what + ": terrain vertices"
    assert np.array_equal(g.mesh_get_vertices(SPHERES).view(np.uint8), sv.view(np.uint8)), what + ": sphere vertices"
    assert np.array_equal(g.object_get_texture(SPHERES, 0)[0], img), what + ": texture level 0"


def test_all_kinds_of_update_in_one_gap(gpu_engine):
    import torch
    u = _uniforms()
    rng = np.random.default_rng(3)
    inst0 = scenes.generate_instances(N, 1.0, 8.0, 0.3, 0.8, seed=11)
    sv0, tv0 = scenes.uv_sphere(8, 5)[0], scenes.grid_plane(12.0, 48, 0.02)[0]
    img0 = _image()
    assert img0.nbytes == 147456 > 4096 * 32
    g = gpu_engine.Renderer(W, H, SD)
    keep = _scene(g, (inst0, None, tv0, sv0, img0, True))
    _frame(g, u); _frame(g, u)
    before = _grab(g)
    assert before[3]["covered_pixels"] > W * H // 4

    # ---- seven host-form updates between frames 2 and 3
    inst1 = inst0.copy()
    inst1["InstancePosition"][:, :2] += rng.normal(0.0, 0.5, (N, 2)).astype(np.float32)
    inst1["InstancePScale"] *= rng.uniform(0.7, 1.4, N).astype(np.float32)
    inst2 = inst1.copy()
    inst2["InstanceRotation"][:N // 2, 1] += np.float32(1.0)
    inst2["InstancePosition"][:N // 2, 2] += np.float32(0.4)
    mask1 = (rng.random(N) > 0.3).astype(np.uint8)
    tv1, sv1, img1 = _deform_terrain(tv0), _deform_sphere(sv0), _variant(img0, 1)
    g.object_set_instances(SPHERES, inst1)
    g.object_set_instance_visibility(SPHERES, mask1)
    g.mesh_set_vertices(TERRAIN, tv1)
    g.mesh_set_vertices(SPHERES, sv1)
    g.object_set_texture(SPHERES, 0, img1)                # (re-makes its ring slot: the first copy above the first capacity)
    g.object_set_instances(SPHERES, inst2[:N // 2])       # (the sixth staged copy: slot 1 again, behind the visibility scatter)
    g.object_set_visible(PLANE, False)
    state1 = (inst2, mask1, tv1, sv1, img1, False)
    fresh1 = _fresh(gpu_engine, state1, u)
    assert not np.array_equal(before[0], fresh1[0]) and not np.array_equal(before[2], fresh1[2])      # the updates show
    _two_frames(g, u, fresh1, "after the host forms")
    _check_readbacks(g, state1, "after the host forms")

    # ---- one device-form update of each kind, on a side stream
    sel = np.arange(0, N, 3, dtype=np.int32)
    inst3 = inst2.copy()
    inst3["InstancePosition"][sel, :2] *= np.float32(0.8)
    mask3 = mask1.copy()
    mask3[sel] = 1 - mask3[sel]
    tv3, img3 = _deform_terrain(tv0, 0.6, 1.5), _variant(img0, 2)
    dev = torch.device("cuda", 0)
    t_inst = torch.from_numpy(inst3[sel].view(np.uint8).reshape(-1, 32).copy()).to(dev)
    t_vis, t_idx = torch.from_numpy(mask3[sel].copy()).to(dev), torch.from_numpy(sel).to(dev)
    t_verts, t_img = _dev_verts(tv3), _dev_image(img3)
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    g.object_update_instances_async(SPHERES, t_inst, t_idx, stream=ts)
    g.object_update_instance_visibility_async(SPHERES, t_vis, t_idx, stream=ts)
    g.mesh_update_vertices_async(TERRAIN, t_verts, stream=ts)
    g.object_update_texture_async(SPHERES, 0, t_img, stream=ts)
    state3 = (inst3, mask3, tv3, sv1, img3, False)
    fresh3 = _fresh(gpu_engine, state3, u)
    assert not np.array_equal(fresh1[0], fresh3[0])
    _two_frames(g, u, fresh3, "after the device forms")
    ts.synchronize()
    _check_readbacks(g, state3, "after the device forms")
    g.close()
    del keep
