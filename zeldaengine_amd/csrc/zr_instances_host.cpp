// zr_instances_host.cpp — moving instances between frames: zr_object_set_instances (host data, through a pinned staging ring) and
// zr_object_update_instances_async (caller-owned device data, in the order of the caller's stream); hiding and showing them, and whole
// objects: zr_object_set_instance_visibility, zr_object_update_instance_visibility_async, zr_object_set_visible.  Kernels: zr_instances.hip.
//
// Ordering: zr_update.cpp.  An update writes only the raw values and the stale lists (k_instance_scatter, bracketed by zr_update_begin /
// zr_update_end); the records of plane p are rebuilt by k_instance_apply at the head of the next frame of parity p (zr_instances_apply,
// called by zr_update_frame behind its waits).
//
// Visibility rides on all of it ("Hiding and showing"): an instance's byte is scattered like a raw value and lands in the
// record's hidden word with the same apply; an object's ZR_OBJ_HIDDEN flag is written into the draw table of each parity at the head of
// that parity's next frame, behind the same waits.
#include <algorithm>
#include <cstring>

#include "zr_ctx.h"

// An object's first update: the parity-1 plane (a copy of the records every frame has read so far), the stale bits and lists, on x.
static int inst_init_object(zr_ctx* c, ZrSceneObject& o, hipStream_t x)
{
    if (o.upd.plane[1]) return ZR_OK;
    const size_t n = o.n_inst;
    ZrInstanceState S = {};
    S.raw = o.d_raw; S.plane[0] = o.d_inst; S.n_inst = o.n_inst;
    ZrOwn mem;                          // (the object's once both are made)
    hipError_t e = mem.alloc(&S.plane[1], n);
    if (e == hipSuccess) e = mem.alloc(&S.dirty, 3 * n + 2);
    if (e == hipSuccess) e = mem.alloc(&S.vis, n);
    if (e != hipSuccess) return zr_fail(c, ZR_ERR_OOM, std::string("instance update state: ") + hipGetErrorString(e));
    o.mem.adopt(std::move(mem));
    S.list[0] = S.dirty + n; S.list[1] = S.dirty + 2 * n; S.count = S.dirty + 3 * n;
    o.upd = S; o.pending[0] = o.pending[1] = 0; o.tab1 = false;
    HIPCHK(c, hipMemsetAsync(S.dirty, 0, n * sizeof(uint32_t), x));
    HIPCHK(c, hipMemsetAsync(S.count, 0, 2 * sizeof(uint32_t), x));
    HIPCHK(c, hipMemsetAsync(S.vis, 1, n, x));      // (every instance shown: the records so far say so)
    // (plane 0 is written only by applies of this object, and there has been none)
    HIPCHK(c, hipMemcpyAsync(S.plane[1], o.d_inst, n * sizeof(ZrInstance), hipMemcpyDeviceToDevice, x));
    return ZR_OK;
}

static int inst_object(zr_ctx* c, uint32_t index, uint32_t first, uint32_t n, const char* what, ZrSceneObject** out)
{
    if (int rc = zr_stage_idle(c, what)) return rc;
    if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": bad object index");
    ZrSceneObject& o = c->objects[index];
    if (!o.instanced || !o.d_raw) return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": object " + std::to_string(index) + " is not instanced");
    if ((uint64_t)first + n > o.n_inst)
        return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": instances [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) +
                                      ") beyond the object's " + std::to_string(o.n_inst));
    *out = &o;
    return ZR_OK;
}

// k_instance_scatter of (idx, data) - or, with `visible`, k_visibility_scatter of (idx, visible) - on stream x, behind the last apply and
// the last update
static int inst_enqueue(zr_ctx* c, ZrSceneObject& o, hipStream_t x, const uint32_t* idx, const XkInstanceData* data, uint32_t first, uint32_t n,
                        const uint8_t* visible = nullptr)
{
    int rc = inst_init_object(c, o, x);
    if (rc == ZR_OK) rc = zr_update_begin(c, x);
    if (rc) return rc;
    if (visible) zr_launch_visibility_scatter(idx, visible, first, n, o.upd, x);
    else zr_launch_instance_scatter(idx, data, first, n, o.upd, x);
    rc = zr_update_end(c, x);
    if (rc) return rc;
    for (auto& p : o.pending) p = (uint32_t)std::min<uint64_t>(o.n_inst, (uint64_t)p + n);
    return ZR_OK;
}

extern "C" int zr_object_set_instances(zr_ctx* c, uint32_t index, uint32_t first, const XkInstanceData* data, uint32_t n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrSceneObject* o = nullptr;
        int rc = inst_object(c, index, first, n, "zr_object_set_instances", &o);
        if (rc) return rc;
        if (n == 0) return ZR_OK;
        if (!data) return zr_fail(c, ZR_ERR_ARG, "zr_object_set_instances: no data");
        HIPCHK(c, hipSetDevice(c->device));
        rc = zr_update_host_form(c, data, (size_t)n * sizeof(XkInstanceData), [&](const void* staged, hipStream_t x) {
            return inst_enqueue(c, *o, x, nullptr, (const XkInstanceData*)staged, first, n);
        });
        if (rc) return rc;
        if (!o->host_stale) memcpy(o->inst.data() + first, data, (size_t)n * sizeof(XkInstanceData));      // (else the read-back brings it)
        return ZR_OK;
    });
}

extern "C" int zr_object_update_instances_async(zr_ctx* c, uint32_t index, uint32_t first, const uint32_t* idx_dev,
                                                const XkInstanceData* data_dev, uint32_t n, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrSceneObject* o = nullptr;
        int rc = inst_object(c, index, first, n, "zr_object_update_instances_async", &o);
        if (rc) return rc;
        if (n == 0) return ZR_OK;
        if (!data_dev || ((uintptr_t)data_dev & 3u) || ((uintptr_t)idx_dev & 3u))
            return zr_fail(c, ZR_ERR_ARG, "zr_object_update_instances_async: data_dev missing, or a buffer not 4-byte aligned");
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t x = hip_stream ? (hipStream_t)hip_stream : c->stream;
        rc = inst_enqueue(c, *o, x, idx_dev, data_dev, first, n);
        if (rc) return rc;
        o->host_stale = true;
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ hiding and showing

extern "C" int zr_object_set_instance_visibility(zr_ctx* c, uint32_t index, uint32_t first, const uint8_t* visible, uint32_t n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrSceneObject* o = nullptr;
        int rc = inst_object(c, index, first, n, "zr_object_set_instance_visibility", &o);
        if (rc) return rc;
        if (n == 0) return ZR_OK;
        if (!visible) return zr_fail(c, ZR_ERR_ARG, "zr_object_set_instance_visibility: no data");
        HIPCHK(c, hipSetDevice(c->device));
        rc = zr_update_host_form(c, visible, n, [&](const void* staged, hipStream_t x) {
            return inst_enqueue(c, *o, x, nullptr, nullptr, first, n, (const uint8_t*)staged);
        });
        if (rc) return rc;
        if (!o->vis_stale) {      // (else the read-back brings it)
            if (o->vis.empty()) o->vis.assign(o->n_inst, 1);
            for (uint32_t i = 0; i < n; ++i) o->vis[first + i] = visible[i] ? 1 : 0;
        }
        return ZR_OK;
    });
}

extern "C" int zr_object_update_instance_visibility_async(zr_ctx* c, uint32_t index, uint32_t first, const uint32_t* idx_dev,
                                                          const uint8_t* visible_dev, uint32_t n, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrSceneObject* o = nullptr;
        int rc = inst_object(c, index, first, n, "zr_object_update_instance_visibility_async", &o);
        if (rc) return rc;
        if (n == 0) return ZR_OK;
        if (!visible_dev || ((uintptr_t)idx_dev & 3u))
            return zr_fail(c, ZR_ERR_ARG, "zr_object_update_instance_visibility_async: visible_dev missing, or idx_dev not 4-byte aligned");
        if (c->scene_dirty) return zr_fail(c, ZR_ERR_STATE, "zr_object_update_instance_visibility_async: no frame has used this scene yet (use zr_object_set_instance_visibility)");
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t x = hip_stream ? (hipStream_t)hip_stream : c->stream;
        rc = inst_enqueue(c, *o, x, idx_dev, nullptr, first, n, visible_dev);
        if (rc) return rc;
        o->vis_stale = true;
        return ZR_OK;
    });
}

extern "C" int zr_object_set_visible(zr_ctx* c, uint32_t index, int visible)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = zr_stage_idle(c, "zr_object_set_visible")) return rc;
        if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, "zr_object_set_visible: bad object index");
        ZrSceneObject& o = c->objects[index];
        if (o.hidden == !visible) return ZR_OK;      // (no flip: nothing changes, the shadow map stays kept)
        if (c->scene_dirty) { o.hidden = !visible; return ZR_OK; }      // zr_scene_finalize writes the flag into the tables it makes
        // The draw table of each parity gets the flag at the head of that parity's next frame (zr_instances_apply), behind the same waits
        // as an instance apply; nothing is scattered, but the frames follow this point of x like any update: the parity-1 table may
        // just have been made on it.
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t x = zr_update_lane(c);
        int rc = zr_update_begin(c, x);
        if (rc == ZR_OK) rc = zr_update_end(c, x);
        if (rc) return rc;
        o.hidden = !visible; o.flag_pending[0] = o.flag_pending[1] = true;
        return ZR_OK;
    });
}

extern "C" int zr_object_get_visibility(zr_ctx* c, uint32_t index, int* object_visible, uint8_t* dst, uint32_t* n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, "zr_object_get_visibility: bad object index");
        ZrSceneObject& o = c->objects[index];
        if (object_visible) *object_visible = o.hidden ? 0 : 1;
        if (n) *n = o.instanced ? o.n_inst : 0u;
        if (!dst || !o.instanced) return ZR_OK;
        if (o.vis_stale) {
            HIPCHK(c, hipSetDevice(c->device));
            if (c->upd.ev_scatter) HIPCHK(c, hipEventSynchronize(c->upd.ev_scatter));      // the last update has landed in the bytes
            o.vis.resize(o.n_inst);
            HIPCHK(c, hipMemcpy(o.vis.data(), o.upd.vis, o.n_inst, hipMemcpyDeviceToHost));
            o.vis_stale = false;
        }
        if (o.vis.empty()) memset(dst, 1, o.n_inst);
        else memcpy(dst, o.vis.data(), o.n_inst);
        return ZR_OK;
    });
}

int zr_instances_sync_host(zr_ctx* c, ZrSceneObject& o)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->upd.ev_scatter) HIPCHK(c, hipEventSynchronize(c->upd.ev_scatter));      // the last update has landed in the raw values
    HIPCHK(c, hipMemcpy(o.inst.data(), o.d_raw, (size_t)o.n_inst * sizeof(XkInstanceData), hipMemcpyDeviceToHost));
    o.host_stale = false;
    return ZR_OK;
}

bool zr_instances_due(const zr_ctx* c, int par)
{
    for (const auto& o : c->objects) if (o.pending[par] != 0 || o.flag_pending[par] || (par == 1 && o.upd.plane[1] && !o.tab1)) return true;
    return false;
}

// zr_update_frame on stream s, behind its waits: the parity-1 table at the planes made since, the objects' flags, the stale records of plane `par`
int zr_instances_apply(zr_ctx* c, hipStream_t s, int par)
{
    for (auto& o : c->objects) {
        if (o.draw >= c->n_objs) return zr_fail(c, ZR_ERR_STATE, "instance update: object outside the draw table");
        if (par == 1 && o.upd.plane[1] && !o.tab1) { zr_launch_table_set_inst(c->d_objs_b[1], o.draw, o.upd.plane[1], s); o.tab1 = true; }
        if (o.flag_pending[par]) { zr_launch_table_set_hidden(c->d_objs_b[par], o.draw, o.hidden ? 1u : 0u, s); o.flag_pending[par] = false; }
        if (o.pending[par]) {
            zr_launch_instance_apply(o.upd, (uint32_t)par, o.pending[par], s);
            HIPCHK(c, hipMemsetAsync(o.upd.count + par, 0, sizeof(uint32_t), s));
            o.pending[par] = 0;
        }
    }
    return ZR_OK;
}
