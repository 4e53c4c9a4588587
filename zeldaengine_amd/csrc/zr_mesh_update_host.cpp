// zr_mesh_update_host.cpp — deforming meshes between frames: zr_mesh_set_vertices (host data, through the pinned staging ring),
// zr_mesh_update_vertices_async (caller-owned device data, in the order of the caller's stream) and zr_mesh_get_vertices.
// Kernels: zr_mesh_update.hip.
//
// Ordering: zr_update.cpp, with the same events, tables and ring as the instance updates.  A frame of parity p reads the draw table and
// the mesh set of parity p; an update writes only the raw vertices (k_vertex_scatter, bracketed by zr_update_begin / zr_update_end) and
// marks both sets stale here on the host; set p is refitted at the head of the next frame of parity p (zr_mesh_update_frame, called by
// zr_update_frame behind its waits: the last scatter, the last frame that read parity p, the last refit), and ev_apply follows the
// refit.  The vertex count, the index buffer and the meshlet partition never change.
#include <cmath>
#include <cstring>

#include "zr_ctx.h"

// A mesh's first update: the raw vertices, the flattened meshlet vertex indices, the parity-1 set; on x.  Set 0 is what upload_mesh made.
static int mesh_init(zr_ctx* c, ZrMesh& m, hipStream_t x)
{
    if (m.upd.raw) return ZR_OK;
    ZrMeshState S = {};
    const size_t nv = m.v.size(), ni = m.idx.size(), nm = m.ms.meshlets.size(), nmv = m.ms.mverts.size();
    ZrOwn mem;                          // (the mesh's once everything is made)
    uint32_t* mverts = nullptr; uint32_t* acc = nullptr;
    ZrMeshSet T = {};
    hipError_t e = mem.alloc(&S.raw, nv);
    if (e == hipSuccess) e = mem.alloc(&mverts, nmv);
    if (e == hipSuccess) e = mem.alloc(&acc, 16);
    if (e == hipSuccess) e = mem.alloc(&T.verts, nv);
    if (e == hipSuccess) e = mem.alloc(&T.rverts, nv);
    if (e == hipSuccess) e = mem.alloc(&T.rtris, std::max<size_t>(1, ni));
    if (e == hipSuccess) e = mem.alloc(&T.meshlets, nm);
    if (e == hipSuccess) e = mem.alloc(&T.mpos, nmv);
    if (e == hipSuccess) e = mem.alloc(&T.mbox, 2 * std::max<size_t>(1, nm));
    if (e != hipSuccess) return zr_fail(c, ZR_ERR_OOM, std::string("vertex update state: ") + hipGetErrorString(e));
    S.mverts = mverts; S.indices = m.d_idx; S.mtri = m.d_mtri;
    S.n_verts = (uint32_t)nv; S.n_tris = (uint32_t)(ni / 3); S.n_meshlets = (uint32_t)nm;
    S.set[0] = ZrMeshSet{ m.d_v, m.d_rv, m.d_rt, m.d_meshlets, m.d_mpos, m.d_mbox, acc };
    T.acc = acc + 8; S.set[1] = T;
    // the raw values: the vertices every frame has drawn so far (set 0's copy; the host's may be older after nothing - it is the same).
    // The parity-1 records: their offsets and counts; every value in set 1 comes from its first refit, before a frame reads it.
    HIPCHK(c, hipMemcpyAsync(S.raw, m.d_v, nv * sizeof(XkVertex), hipMemcpyDeviceToDevice, x));
    HIPCHK(c, hipMemcpyAsync(T.meshlets, m.d_meshlets, nm * sizeof(XkMeshlet), hipMemcpyDeviceToDevice, x));
    if (ni == 0) HIPCHK(c, hipMemsetAsync(T.rtris, 0, sizeof(ZrRVertex), x));
    if (nm == 0) HIPCHK(c, hipMemsetAsync(T.mbox, 0, 2 * sizeof(float4), x));
    for (int p = 0; p < 2; ++p) {       // the reductions' cells: least corner "nothing yet", the rest zero (k_table_set_mesh resets them)
        HIPCHK(c, hipMemsetAsync(acc + 8 * p, 0xFF, 3 * sizeof(uint32_t), x));
        HIPCHK(c, hipMemsetAsync(acc + 8 * p + 3, 0, 5 * sizeof(uint32_t), x));
    }
    // (pageable source: the copy is staged before this returns; ms.mverts never changes afterwards)
    HIPCHK(c, hipMemcpyAsync(mverts, m.ms.mverts.data(), nmv * sizeof(uint32_t), hipMemcpyHostToDevice, x));
    m.mem.adopt(std::move(mem));
    m.upd = S;
    // every frame so far may have read set 0, the one enqueued last among them: set 0's first refit waits for it (zr_update_frame)
    c->upd.reader[0] = std::max<uint64_t>(c->upd.reader[0], c->frame_no);
    return ZR_OK;
}

static int mesh_range(zr_ctx* c, uint32_t mesh_id, uint32_t first, uint32_t n, const char* what, ZrMesh** out)
{
    if (int rc = zr_stage_idle(c, what)) return rc;
    if (mesh_id >= c->meshes.size()) return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": bad mesh id");
    ZrMesh& m = c->meshes[mesh_id];
    if ((uint64_t)first + n > m.v.size())
        return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": vertices [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) +
                                      ") beyond the mesh's " + std::to_string(m.v.size()));
    *out = &m;
    return ZR_OK;
}

// k_vertex_scatter of src on stream x, behind the last refit and the last update; both sets are stale from here on
static int mesh_enqueue(zr_ctx* c, ZrMesh& m, hipStream_t x, const XkVertex* src, uint32_t first, uint32_t n)
{
    int rc = mesh_init(c, m, x);
    if (rc == ZR_OK) rc = zr_update_begin(c, x);
    if (rc) return rc;
    zr_launch_vertex_scatter(src, first, n, m.upd, x);
    rc = zr_update_end(c, x);      // (the whole-mesh sphere moves: the passes' work lists are rebuilt, the shadow map is drawn again; history, plan and flags stay)
    if (rc) return rc;
    m.stale[0] = m.stale[1] = true; m.ml_stale = true;
    return ZR_OK;
}

static void host_bounds(ZrMesh& m)
{
    for (XkMeshlet& d : m.ms.meshlets)
        zr_meshlet_bounds(m.v.data(), m.ms.mverts.data() + d.VertexOffset, d.VertexCount, m.ms.mtris.data() + d.TriangleOffset, d.TriangleCount, &d);
}

extern "C" int zr_mesh_set_vertices(zr_ctx* c, uint32_t mesh_id, uint32_t first, const XkVertex* v, uint32_t n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrMesh* m = nullptr;
        int rc = mesh_range(c, mesh_id, first, n, "zr_mesh_set_vertices", &m);
        if (rc) return rc;
        if (n == 0) return ZR_OK;
        if (!v) return zr_fail(c, ZR_ERR_ARG, "zr_mesh_set_vertices: no data");
        if (!m->uploaded) {
            // no frame has used the mesh: the host copy is all there is.  upload_mesh derives every buffer from it; the bounds of
            // meshlets already attached follow the vertices here.
            memcpy(m->v.data() + first, v, (size_t)n * sizeof(XkVertex));
            if (m->has_meshlets) host_bounds(*m);
            zr_casters_changed(c);
            return ZR_OK;
        }
        HIPCHK(c, hipSetDevice(c->device));
        rc = zr_update_host_form(c, v, (size_t)n * sizeof(XkVertex), [&](const void* staged, hipStream_t x) {
            return mesh_enqueue(c, *m, x, (const XkVertex*)staged, first, n);
        });
        if (rc) return rc;
        if (!m->v_stale) memcpy(m->v.data() + first, v, (size_t)n * sizeof(XkVertex));      // (else the read-back brings it)
        return ZR_OK;
    });
}

extern "C" int zr_mesh_update_vertices_async(zr_ctx* c, uint32_t mesh_id, uint32_t first, const XkVertex* v_dev, uint32_t n, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrMesh* m = nullptr;
        int rc = mesh_range(c, mesh_id, first, n, "zr_mesh_update_vertices_async", &m);
        if (rc) return rc;
        if (n == 0) return ZR_OK;
        if (!v_dev || ((uintptr_t)v_dev & 3u))
            return zr_fail(c, ZR_ERR_ARG, "zr_mesh_update_vertices_async: v_dev missing or not 4-byte aligned");
        if (!m->uploaded)
            return zr_fail(c, ZR_ERR_STATE, "zr_mesh_update_vertices_async: no frame has used mesh " + std::to_string(mesh_id) +
                                            " yet, it has no device copy to update: use zr_mesh_set_vertices (the host form) until one has");
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t x = hip_stream ? (hipStream_t)hip_stream : c->stream;
        rc = mesh_enqueue(c, *m, x, v_dev, first, n);
        if (rc) return rc;
        m->v_stale = true;
        return ZR_OK;
    });
}

extern "C" int zr_mesh_get_vertices(zr_ctx* c, uint32_t mesh_id, XkVertex* dst, uint32_t* n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size());
        ZrMesh& m = c->meshes[mesh_id];
        if (dst) { int rc = zr_mesh_sync_host(c, m, false); if (rc) return rc; }
        if (n) *n = (uint32_t)m.v.size();
        if (dst) memcpy(dst, m.v.data(), m.v.size() * sizeof(XkVertex));
        return ZR_OK;
    });
}

// The host copies after updates, with one synchronisation: the vertices from the raw array behind the last update; the meshlets' bounds
// from a set a frame head has refitted since the last update, else - no frame since - by the host's own statement of the same function.
int zr_mesh_sync_host(zr_ctx* c, ZrMesh& m, bool meshlets)
{
    if (!m.upd.raw || (!m.v_stale && !(meshlets && m.ml_stale))) return ZR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (m.v_stale) {
        if (c->upd.ev_scatter) HIPCHK(c, hipEventSynchronize(c->upd.ev_scatter));      // the last update has landed in the raw values
        HIPCHK(c, hipMemcpy(m.v.data(), m.upd.raw, m.v.size() * sizeof(XkVertex), hipMemcpyDeviceToHost));
        m.v_stale = false;
    }
    if (meshlets && m.ml_stale) {
        const int p = !m.stale[0] ? 0 : !m.stale[1] ? 1 : -1;
        if (p >= 0) {
            if (c->upd.ev_apply) HIPCHK(c, hipEventSynchronize(c->upd.ev_apply));      // (ev_apply covers every refit)
            HIPCHK(c, hipMemcpy(m.ms.meshlets.data(), m.upd.set[p].meshlets, m.ms.meshlets.size() * sizeof(XkMeshlet), hipMemcpyDeviceToHost));
            m.ml_stale = false;
        } else host_bounds(m);      // (ml_stale stays: once a frame has refitted a set, the next read-back takes the device's records)
    }
    return ZR_OK;
}

bool zr_mesh_update_due(const zr_ctx* c, int par)
{
    for (const auto& m : c->meshes) if (m.stale[par]) return true;
    return false;
}

// zr_update_frame on stream s, behind its waits: set `par` of every stale mesh from the raw vertices, the table of this parity at it
int zr_mesh_update_frame(zr_ctx* c, hipStream_t s, int par)
{
    for (auto& m : c->meshes) {
        if (!m.stale[par]) continue;
        zr_launch_mesh_refit(m.upd, (uint32_t)par, c->d_objs_b[par], c->n_objs, s);
        m.stale[par] = false;
    }
    return ZR_OK;
}

// zr_scene_finalize made table 0 from set 0 and the host's spheres (zr_update_table copies it to table 1): the next refit of each parity
// writes this parity's pointers and the current sphere into them.  Nothing is in flight.
bool zr_mesh_update_table(zr_ctx* c)
{
    bool any = false;
    for (auto& m : c->meshes) if (m.upd.raw) { m.stale[0] = m.stale[1] = true; any = true; }
    return any;
}
