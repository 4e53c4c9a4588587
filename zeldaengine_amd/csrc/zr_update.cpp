// zr_update.cpp — what orders the between-frames updates (instances, visibility, vertices, textures) against the frames in flight: the
// context's update state (zr_ctx::upd), the brackets round an update's kernels, the host forms' lane and staging ring, the parity-1
// draw table and the frame head.  What is specific to a kind of update - its refusals, its kernels, its host copies - lives with the
// kind: zr_instances_host.cpp, zr_mesh_update_host.cpp, zr_texture_update_host.cpp.
//
// Ordering ("Moving instances").  A frame of parity p reads the draw table and the instance planes / mesh sets of parity p;
// an update writes only the raw values and the stale lists, and parity p is brought up to date at the head of the next frame of parity p,
// after the last frame that read it has finished.  So a frame already enqueued keeps the values it was enqueued with, and no update
// waits for a frame.  Raw values are written by the scatters and read by the applies and refits: every scatter is ordered after the last
// apply (ev_apply), and every apply after the last scatter (ev_scatter).  Textures are rewritten in place and ordered against the frames
// on both sides instead (ev_tex; "Changing textures").
#include <cstring>

#include "zr_ctx.h"
#include "zr_srgb.h"

static int inst_init_ctx(zr_ctx* c)
{
    if (c->upd.ev_scatter) return ZR_OK;
    HIPCHK(c, c->own.event(&c->upd.ev_apply, hipEventDisableTiming));
    for (auto& r : c->upd.ring) HIPCHK(c, c->own.event(&r.ev, hipEventDisableTiming));
    HIPCHK(c, c->own.event(&c->upd.ev_scatter, hipEventDisableTiming));      // (last: it marks the set as made)
    return ZR_OK;
}

static int tex_init_ctx(zr_ctx* c)
{
    if (c->upd.ev_tex) return ZR_OK;
    if (!c->upd.d_srgb_thr) {
        float thr[256];
        zr_srgb_thresholds(thr);
        HIPCHK(c, c->own.alloc(&c->upd.d_srgb_thr, 256));
        HIPCHK(c, hipMemcpy(c->upd.d_srgb_thr, thr, sizeof thr, hipMemcpyHostToDevice));
    }
    HIPCHK(c, c->own.event(&c->upd.ev_tex, hipEventDisableTiming));      // (last: it marks the set as made)
    return ZR_OK;
}

// An update's scatter on stream x, first half: the context's update state; the parity-1 draw table; x behind the last apply (it read
// the raw values) and the last update (updates land in call order)
int zr_update_begin(zr_ctx* c, hipStream_t x)
{
    int rc = inst_init_ctx(c);
    if (rc) return rc;
    if (!c->upd.dual && !c->scene_dirty) {
        // the parity-1 draw table: table 0 as it stands (nothing writes it); the frame head points it at the parity-1 planes and mesh
        // sets.  (A dirty scene gets both tables from zr_scene_finalize, before its next frame.)
        HIPCHK(c, c->tables.alloc(&c->d_objs_b[1], c->n_objs));
        HIPCHK(c, hipMemcpyAsync(c->d_objs_b[1], c->d_objs_b[0], (size_t)c->n_objs * sizeof(ZrObject), hipMemcpyDeviceToDevice, x));
        c->upd.dual = true;
    }
    if (c->upd.apply_done && c->upd.apply_s != x) HIPCHK(c, hipStreamWaitEvent(x, c->upd.ev_apply, 0));
    if (c->upd.scatter_s && c->upd.scatter_s != x) HIPCHK(c, hipStreamWaitEvent(x, c->upd.ev_scatter, 0));
    return ZR_OK;
}

// ... second half, behind the scatter kernel: the next frame of either parity waits for it
int zr_update_end(zr_ctx* c, hipStream_t x)
{
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->upd.ev_scatter, x));
    c->upd.scatter_s = x; c->upd.scatter_wait[0] = c->upd.scatter_wait[1] = true;
    // The passes' work lists (k_cull_instances) hold the instances that passed the whole-mesh test: rebuilt by the next frame.  The visibility
    // history, the bucket plan and the shadow flags stay: the frame does not depend on them.
    zr_history_forgotten(c, ZR_HIST_LISTS);
    // The kept shadow map goes too: a caster moved (instances) or changed shape (vertices - the lists are instance-level and would not
    // have needed rebuilding for that, the map does).  Said at enqueue time: x orders the scatter ahead of the next frame.
    zr_casters_changed(c);
    return ZR_OK;
}

// "The end of frame f" (f < frame_no), for whoever waits for it: f's own event or, where f recorded none, a later one of the host's stream -
// recorded now, in the newest frame's name, if nothing behind f was (zr_frame_end.h).
int zr_frame_end(zr_ctx* c, uint64_t f, hipEvent_t* ev)
{
    const ZrEndAsk a = zr_end_ask(&c->end, f, c->frame_no);
    *ev = c->ev_end[a.frame % zr_ctx::END_RING];
    if (a.record) HIPCHK(c, hipEventRecord(*ev, c->stream));      // (every lighting pass so far is ahead of this point of the host's stream)
    return ZR_OK;
}
int zr_wait_frame_end(zr_ctx* c, hipStream_t x, uint64_t f)
{
    hipEvent_t end;
    if (int rc = zr_frame_end(c, f, &end)) return rc;
    HIPCHK(c, hipStreamWaitEvent(x, end, 0));
    return ZR_OK;
}

// A texture update's kernel on stream x, first half: the context's state; x behind the readers of the old image - the frame enqueued
// last, on both lanes (on the render stream its lighting pass is ahead of this point) - and behind the update before
int zr_update_tex_begin(zr_ctx* c, hipStream_t x)
{
    int rc = tex_init_ctx(c);
    if (rc) return rc;
    if (c->frame_no >= 1 && x != c->stream && (rc = zr_wait_frame_end(c, x, c->frame_no - 1)) != ZR_OK) return rc;
    if (c->upd.tex_s && c->upd.tex_s != x) HIPCHK(c, hipStreamWaitEvent(x, c->upd.ev_tex, 0));
    return ZR_OK;
}

// ... second half, behind the kernel: the next frame's first stream waits for it.  No list, plan, history or shadow map depends on a
// texel: of what the frames keep, only the GBuffer is invalidated.
int zr_update_tex_end(zr_ctx* c, hipStream_t x)
{
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->upd.ev_tex, x));
    c->upd.tex_s = x; c->upd.tex_wait = true;
    zr_surface_changed(c);      // (the GBuffer does: the next two frames resolve again, whatever else they keep)
    return ZR_OK;
}

// The host forms' lane, the camera lane: an update that follows frame k is then ordered behind frame k's camera pipeline and ahead of
// frame k + 1's, with no extra wait on the host's stream, where frame k's lighting runs
hipStream_t zr_update_lane(const zr_ctx* c) { return c->cam_s ? c->cam_s : c->stream; }

// Host data through the pinned staging ring: `bytes` of src copied to a device slot on x (*dev); the caller records *ev behind the
// kernel that reads the slot.  src may be reused on return.
static int update_stage(zr_ctx* c, hipStream_t x, const void* src, size_t bytes, void** dev, hipEvent_t* ev)
{
    int rc = inst_init_ctx(c);
    if (rc) return rc;
    zr_ctx::Update::Stage& r = c->upd.ring[c->upd.slot++ % zr_ctx::Update::RING];
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

int zr_update_host_form(zr_ctx* c, const void* src, size_t bytes, const std::function<int(const void*, hipStream_t)>& enqueue)
{
    return zr_update_host_form_on(c, zr_update_lane(c), src, bytes, enqueue);
}

int zr_update_host_form_on(zr_ctx* c, hipStream_t x, const void* src, size_t bytes, const std::function<int(const void*, hipStream_t)>& enqueue)
{
    void* staged = nullptr; hipEvent_t ev = nullptr;
    int rc = update_stage(c, x, src, bytes, &staged, &ev);
    if (rc == ZR_OK) rc = enqueue(staged, x);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(ev, x));
    return ZR_OK;
}

hipError_t zr_update_sync(zr_ctx* c)
{
    hipError_t e = hipSuccess;
    if (c->upd.ev_scatter) e = hipEventSynchronize(c->upd.ev_scatter);                       // the last instance / vertex update
    if (e == hipSuccess && c->upd.ev_tex) e = hipEventSynchronize(c->upd.ev_tex);            // the last texture update
    return e;
}

void zr_drop_draw_tables(zr_ctx* c) { c->tables.release(); c->d_objs_b[0] = c->d_objs_b[1] = c->d_objs = nullptr; c->upd.dual = false; }

// zr_scene_finalize, after a full synchronisation and a new table 0 (the draw tables' owner released the old ones): the parity-1 table, when
// some object has been updated
int zr_update_table(zr_ctx* c)
{
    c->upd.dual = false;
    c->upd.reader[0] = c->upd.reader[1] = 0;      // (nothing is in flight)
    bool any = false;
    for (auto& o : c->objects) { o.tab1 = false; o.flag_pending[0] = o.flag_pending[1] = false; any |= o.upd.plane[1] != nullptr; }      // (table 0 holds every flag)
    any |= zr_mesh_update_table(c);      // (meshes with a second set: both tables get their pointers and spheres from the next refits)
    if (!any) return ZR_OK;
    HIPCHK(c, c->tables.alloc(&c->d_objs_b[1], c->n_objs));
    HIPCHK(c, hipMemcpy(c->d_objs_b[1], c->d_objs_b[0], (size_t)c->n_objs * sizeof(ZrObject), hipMemcpyDeviceToDevice));
    c->upd.dual = true;
    return ZR_OK;
}

// frame_begin on stream s, after its wait for the frame two before: this frame's draw table; the updates due in this parity's planes and
// mesh sets; s - the frame's first stream - behind the last texture update (later frames follow this one on s, or wait for its end; the
// frame's other lane joins s before it samples)
int zr_update_frame(zr_ctx* c, hipStream_t s, int par)
{
    zr_ctx::Update& U = c->upd;
    if (!U.dual) {       // (no update since the scene was made: every frame reads table 0)
        c->d_objs = c->d_objs_b[0]; U.reader[0] = c->frame_no + 1;
    } else {
        const bool apply = zr_instances_due(c, par), refit = zr_mesh_update_due(c, par);
        if (U.scatter_wait[par]) {       // the raw values and lists as the last update left them
            if (U.scatter_s != s) HIPCHK(c, hipStreamWaitEvent(s, U.ev_scatter, 0));
            U.scatter_wait[par] = false;
        }
        if (apply || refit) {
            // The last frame that read this parity's table and planes: two lanes wait for the frame two before only (frame_begin), but until
            // the first update every frame read parity 0's, the one before this frame among them.  (On the host's stream every frame's
            // lighting pass - its last reader - is ahead of this point.)
            const uint64_t r = U.reader[par];
            if (r && s != c->stream && (c->frame_no < 2 || r - 1 > c->frame_no - 2))
                if (int rc = zr_wait_frame_end(c, s, r - 1)) return rc;
            if (U.apply_done && U.apply_s != s) HIPCHK(c, hipStreamWaitEvent(s, U.ev_apply, 0));      // (ev_apply keeps covering every apply)
            int rc = zr_instances_apply(c, s, par);
            if (rc == ZR_OK && refit) rc = zr_mesh_update_frame(c, s, par);      // this parity's set of every stale mesh
            if (rc) return rc;
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventRecord(U.ev_apply, s));
            U.apply_s = s; U.apply_done = true;
            if (s != c->stream) HIPCHK(c, hipStreamWaitEvent(c->stream, U.ev_apply, 0));      // the shadow pipeline reads them there
        }
        c->d_objs = c->d_objs_b[par]; U.reader[par] = c->frame_no + 1;
    }
    if (U.tex_wait) {
        if (U.tex_s != s) HIPCHK(c, hipStreamWaitEvent(s, U.ev_tex, 0));
        U.tex_wait = false;
    }
    return ZR_OK;
}
