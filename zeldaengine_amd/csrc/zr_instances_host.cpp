// zr_instances_host.cpp — moving instances between frames: zr_object_set_instances (host data, through a pinned staging ring) and
// zr_object_update_instances_async (caller-owned device data, in the order of the caller's stream); hiding and showing them, and whole
// objects: zr_object_set_instance_visibility, zr_object_update_instance_visibility_async, zr_object_set_visible.  Kernels: zr_instances.hip.
//
// Ordering ("Moving instances").  A frame of parity p reads the draw table and the instance planes of parity p; an update
// writes only the raw values and the stale lists, and the records of plane p are rebuilt at the head of the next frame of parity p, after
// the last frame that read plane p has finished.  So a frame already enqueued keeps the values it was enqueued with, and no update waits
// for a frame.  Raw values are written by k_instance_scatter and read by k_instance_apply: every scatter is ordered after the last apply
// (ev_apply), and every apply after the last scatter (ev_scatter).
//
// Visibility rides on all of it ("Hiding and showing"): an instance's byte is scattered like a raw value and lands in the
// record's hidden word with the same apply; an object's ZR_OBJ_HIDDEN flag is written into the draw table of each parity at the head of
// that parity's next frame, behind the same waits.
//
// Vertex updates (zr_mesh_update_host.cpp) keep the same contract with the same events, tables and staging ring: their scatter is
// bracketed by zr_update_begin / zr_update_end, their refit runs in zr_instances_frame beside the applies.
#include <algorithm>
#include <cstring>

#include "zr_ctx.h"

static int inst_init_ctx(zr_ctx* c)
{
    if (c->ev_scatter) return ZR_OK;
    HIPCHK(c, c->own.event(&c->ev_apply, hipEventDisableTiming));
    for (auto& r : c->inst_ring) HIPCHK(c, c->own.event(&r.ev, hipEventDisableTiming));
    HIPCHK(c, c->own.event(&c->ev_scatter, hipEventDisableTiming));      // (last: it marks the set as made)
    return ZR_OK;
}

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

// An update's scatter on stream x, first half: the context's update state; the parity-1 draw table; x behind the last apply (it read
// the raw values) and the last update (updates land in call order)
int zr_update_begin(zr_ctx* c, hipStream_t x)
{
    int rc = inst_init_ctx(c);
    if (rc) return rc;
    if (!c->inst_dual && !c->scene_dirty) {
        // the parity-1 draw table: table 0 as it stands (nothing writes it); the frame head points it at the parity-1 planes and mesh
        // sets.  (A dirty scene gets both tables from finalize_scene, before its next frame.)
        HIPCHK(c, c->tables.alloc(&c->d_objs_b[1], c->n_objs));
        HIPCHK(c, hipMemcpyAsync(c->d_objs_b[1], c->d_objs_b[0], (size_t)c->n_objs * sizeof(ZrObject), hipMemcpyDeviceToDevice, x));
        c->inst_dual = true;
    }
    if (c->apply_done && c->apply_s != x) HIPCHK(c, hipStreamWaitEvent(x, c->ev_apply, 0));
    if (c->scatter_s && c->scatter_s != x) HIPCHK(c, hipStreamWaitEvent(x, c->ev_scatter, 0));
    return ZR_OK;
}

// ... second half, behind the scatter kernel: the next frame of either parity waits for it
int zr_update_end(zr_ctx* c, hipStream_t x)
{
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_scatter, x));
    c->scatter_s = x; c->scatter_wait[0] = c->scatter_wait[1] = true;
    // The passes' work lists (k_cull_instances) hold the instances that passed the whole-mesh test: rebuilt by the next frame.  The visibility
    // history, the bucket plan and the shadow flags stay: the frame does not depend on them.
    c->list_valid[0] = c->list_valid[1] = false;
    // The kept shadow map goes too: a caster moved (instances) or changed shape (vertices - the lists are instance-level and would not
    // have needed rebuilding for that, the map does).  Said at enqueue time: x orders the scatter ahead of the next frame.
    zr_casters_changed(c);
    return ZR_OK;
}

// Host data through the pinned staging ring: `bytes` of src copied to a device slot on x (*dev); the caller records *ev behind the
// kernel that reads the slot.  src may be reused on return.
int zr_update_stage(zr_ctx* c, hipStream_t x, const void* src, size_t bytes, void** dev, hipEvent_t* ev)
{
    int rc = inst_init_ctx(c);
    if (rc) return rc;
    zr_ctx::InstStage& r = c->inst_ring[c->inst_slot++ % zr_ctx::INST_RING];
    HIPCHK(c, hipEventSynchronize(r.ev));          // the copy and the scatter that used this slot last are done
    if (r.cap < bytes) {
        r.mem.release(); r.h = nullptr; r.d = nullptr;
        r.cap = 0;
        size_t cap = 4096 * sizeof(XkInstanceData); while (cap < bytes) cap *= 2;
        HIPCHK(c, r.mem.host(&r.h, cap));
        HIPCHK(c, r.mem.alloc(&r.d, cap));
        r.cap = cap;
    }
    memcpy(r.h, src, bytes);
    HIPCHK(c, hipMemcpyAsync(r.d, r.h, bytes, hipMemcpyHostToDevice, x));
    *dev = r.d; *ev = r.ev;
    return ZR_OK;
}

static int inst_object(zr_ctx* c, uint32_t index, uint32_t first, uint32_t n, const char* what, ZrSceneObject** out)
{
    if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, std::string(what) + " between the stages of a frame (finish it with zr_render_lighting first)");
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
    int rc = inst_init_ctx(c);
    if (rc == ZR_OK) rc = inst_init_object(c, o, x);
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
        // the camera lane: an update that follows frame k is then ordered behind frame k's camera pipeline and ahead of frame k + 1's, with no
        // extra wait on the host's stream, where frame k's lighting runs
        hipStream_t x = c->cam_s ? c->cam_s : c->stream;
        void* staged = nullptr; hipEvent_t ev = nullptr;
        rc = zr_update_stage(c, x, data, (size_t)n * sizeof(XkInstanceData), &staged, &ev);
        if (rc) return rc;
        rc = inst_enqueue(c, *o, x, nullptr, (const XkInstanceData*)staged, first, n);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(ev, x));
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
        hipStream_t x = c->cam_s ? c->cam_s : c->stream;      // (the camera lane, as zr_object_set_instances)
        void* staged = nullptr; hipEvent_t ev = nullptr;
        rc = zr_update_stage(c, x, visible, n, &staged, &ev);
        if (rc) return rc;
        rc = inst_enqueue(c, *o, x, nullptr, nullptr, first, n, (const uint8_t*)staged);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(ev, x));
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
        if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_object_set_visible between the stages of a frame (finish it with zr_render_lighting first)");
        if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, "zr_object_set_visible: bad object index");
        ZrSceneObject& o = c->objects[index];
        if (o.hidden == !visible) return ZR_OK;      // (no flip: nothing changes, the shadow map stays kept)
        if (c->scene_dirty) { o.hidden = !visible; return ZR_OK; }      // finalize_scene writes the flag into the tables it makes
        // The draw table of each parity gets the flag at the head of that parity's next frame (zr_instances_frame), behind the same waits
        // as an instance apply; nothing is scattered, but the frames follow this point of x like any update: the parity-1 table may
        // just have been made on it.
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t x = c->cam_s ? c->cam_s : c->stream;
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
            if (c->ev_scatter) HIPCHK(c, hipEventSynchronize(c->ev_scatter));      // the last update has landed in the bytes
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
    if (c->ev_scatter) HIPCHK(c, hipEventSynchronize(c->ev_scatter));      // the last update has landed in the raw values
    HIPCHK(c, hipMemcpy(o.inst.data(), o.d_raw, (size_t)o.n_inst * sizeof(XkInstanceData), hipMemcpyDeviceToHost));
    o.host_stale = false;
    return ZR_OK;
}

// finalize_scene, after a full synchronisation and a new table 0 (the draw tables' owner released the old ones): the parity-1 table, when
// some object has been updated
int zr_instances_table(zr_ctx* c)
{
    c->inst_dual = false;
    c->inst_reader[0] = c->inst_reader[1] = 0;      // (nothing is in flight)
    bool any = false;
    for (auto& o : c->objects) { o.tab1 = false; o.flag_pending[0] = o.flag_pending[1] = false; any |= o.upd.plane[1] != nullptr; }      // (table 0 holds every flag)
    any |= zr_mesh_update_table(c);      // (meshes with a second set: both tables get their pointers and spheres from the next refits)
    if (!any) return ZR_OK;
    HIPCHK(c, c->tables.alloc(&c->d_objs_b[1], c->n_objs));
    HIPCHK(c, hipMemcpy(c->d_objs_b[1], c->d_objs_b[0], (size_t)c->n_objs * sizeof(ZrObject), hipMemcpyDeviceToDevice));
    c->inst_dual = true;
    return ZR_OK;
}

// frame_begin on stream s, after its wait for the frame two before: this frame's draw table; the updates due in this parity's planes
int zr_instances_frame(zr_ctx* c, hipStream_t s, int par)
{
    if (!c->inst_dual) {       // (no update since the scene was made: every frame reads table 0)
        c->d_objs = c->d_objs_b[0]; c->inst_reader[0] = c->frame_no + 1;
        return ZR_OK;
    }
    bool work = false;
    for (const auto& o : c->objects) work |= o.pending[par] != 0 || o.flag_pending[par] || (par == 1 && o.upd.plane[1] && !o.tab1);
    const bool refit = zr_mesh_update_due(c, par);
    work |= refit;
    if (c->scatter_wait[par]) {       // the raw values and lists as the last update left them
        if (c->scatter_s != s) HIPCHK(c, hipStreamWaitEvent(s, c->ev_scatter, 0));
        c->scatter_wait[par] = false;
    }
    if (work) {
        // The last frame that read this parity's table and planes: two lanes wait for the frame two before only (frame_begin), but until
        // the first update every frame read parity 0's, the one before this frame among them.  (On the host's stream every frame's
        // lighting pass - its last reader - is ahead of this point.)
        const uint64_t r = c->inst_reader[par];
        if (r && s != c->stream && (c->frame_no < 2 || r - 1 > c->frame_no - 2))
            HIPCHK(c, hipStreamWaitEvent(s, c->ev_end[(r - 1) % zr_ctx::END_RING], 0));
        if (c->apply_done && c->apply_s != s) HIPCHK(c, hipStreamWaitEvent(s, c->ev_apply, 0));      // (ev_apply keeps covering every apply)
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
        if (refit) { const int rc = zr_mesh_update_frame(c, s, par); if (rc) return rc; }      // this parity's set of every stale mesh
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_apply, s));
        c->apply_s = s; c->apply_done = true;
        if (s != c->stream) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_apply, 0));      // the shadow pipeline reads them there
    }
    c->d_objs = c->d_objs_b[par]; c->inst_reader[par] = c->frame_no + 1;
    return ZR_OK;
}
