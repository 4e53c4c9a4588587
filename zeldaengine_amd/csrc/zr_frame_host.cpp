// zr_frame_host.cpp — per-frame uniforms and the frame graph behind the C-ABI (zelda_render.h): zr_update_uniforms / zr_set_frame, the two
// geometry passes' kernel arguments (build_pass), frame_begin ... zr_render, and what a multi-GPU host puts between the stages (the
// shadow partition, the shadow map's tiles, pack / unpack, the caller's map).
//
// Host counterpart of XkZeldaEngineApp's UpdateUniformBuffer / RecordCommandBuffer / DrawFrame (ZE:4585, 3160, 1940).  GPU work is
// enqueued on two HIP streams (the host's render stream and the library's camera lane, see geometry_passes).
#include "zr_ctx.h"
#include "zr_math.h"

#include <cmath>
#include <cstring>

// A schedule constant, re-measured whenever the balance of the two lanes changes ("The schedule"; the others:
// zr_context.cpp): whether a frame that draws its shadow map records ev_cam ahead of its k_plan too (a frame that resolves on the host's
// stream always does).
#ifndef ZR_EV_CAM_AHEAD_OF_PLAN
#define ZR_EV_CAM_AHEAD_OF_PLAN 0
#endif
// ... and where the head of a zr_render frame that keeps camera pass and shadow map runs - the uniform upload and the one-pixel launch, some
// 15 us of latency ahead of k_lighting: 0 in series on the host's stream, 1 on the idle camera lane beside the previous frame's lighting
// pass, at the price of one event crossing (DESIGN.md section 7 has both, measured: 17 470 / 19 240 Mpixel/s).
#ifndef ZR_KEPT_HEAD_ON_LANE
#define ZR_KEPT_HEAD_ON_LANE 1
#endif

// ------------------------------------------------------------------------------------------------ uniforms

static float radiansf(float deg) { return deg * 0.01745329251994329576923690768489f; }
static void perspective_rh_zo(float fovy, float aspect, float zn, float zf, float* m)
{
    const float t = tanf(fovy / 2.0f);
    memset(m, 0, 64);
    m[0] = 1.0f / (aspect * t); m[5] = 1.0f / t; m[10] = zf / (zn - zf); m[11] = -1.0f; m[14] = -(zf * zn) / (zf - zn);
}
static void look_at_rh(zf3 eye, zf3 center, zf3 up, float* m)
{
    const zf3 f = zr_normalize_ieee(center - eye);          // (glm on the host: IEEE, not the shaders' inversesqrt)
    const zf3 s = zr_normalize_ieee(zr_cross(f, up));
    const zf3 u = zr_cross(s, f);
    m[0] = s.x; m[4] = s.y; m[8] = s.z; m[1] = u.x; m[5] = u.y; m[9] = u.z; m[2] = -f.x; m[6] = -f.y; m[10] = -f.z;
    m[3] = 0; m[7] = 0; m[11] = 0; m[12] = -zr_dot(s, eye); m[13] = -zr_dot(u, eye); m[14] = zr_dot(f, eye); m[15] = 1.0f;
}
static void rotate_z(float angle, float* m)
{
    const float cs = cosf(angle), sn = sinf(angle);
    memset(m, 0, 64);
    m[0] = cs; m[1] = sn; m[4] = -sn; m[5] = cs; m[10] = cs + (1.0f - cs); m[15] = 1.0f;
}

// UpdateWorld (ZE:4294-4308) + UpdateUniformBuffer (ZE:4585-4664) in game mode (editor bars = 0, ZE:4575-4579)
extern "C" int zr_update_uniforms(zr_ctx* c, const zr_camera* cam, const XkLight* dir, uint32_t n_dir, const XkLight* point,
                                  uint32_t n_point, const XkLight* spot, uint32_t n_spot, float roll_stage, float roll_light, float time)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, cam && n_dir <= XK_MAX_DIRECTIONAL_LIGHTS_NUM && n_point <= XK_MAX_POINT_LIGHTS_NUM && n_spot <= XK_MAX_SPOT_LIGHTS_NUM);
        ARGCHK(c, (n_dir == 0 || dir) && (n_point == 0 || point) && (n_spot == 0 || spot));
        // both geometry passes' kernel arguments are fixed when a frame begins (zr_render_shadow / zr_render_geometry): uniforms set between the
        // stages of a frame would reach its lighting pass only
        if (int rc = zr_stage_idle(c, "zr_update_uniforms")) return rc;
        XkView* V = &c->view;
        c->view_dirty = true;
        for (uint32_t i = 0; i < n_dir; ++i) V->DirectionalLights[i] = dir[i];
        for (uint32_t i = 0; i < n_point; ++i) V->PointLights[i] = point[i];
        for (uint32_t i = 0; i < n_spot; ++i) V->SpotLights[i] = spot[i];
        V->LightsCount[0] = (int32_t)n_dir; V->LightsCount[1] = (int32_t)n_point; V->LightsCount[2] = (int32_t)n_spot;
        V->LightsCount[3] = (int32_t)c->cube_levels;

        const zf3 pos = zr3(cam->Position[0], cam->Position[1], cam->Position[2]);
        const zf3 look = zr3(cam->Lookat[0], cam->Lookat[1], cam->Lookat[2]);
        const zf3 up = zr3(0.0f, 0.0f, 1.0f);
        const zf3 lightPos = zr3(V->DirectionalLights[0].Position[0], V->DirectionalLights[0].Position[1], V->DirectionalLights[0].Position[2]);
        float l2w[16], sview[16], sproj[16], cview[16], cproj[16];
        rotate_z(roll_stage, l2w);
        look_at_rh(lightPos, zr3(0.0f, 0.0f, 0.0f), up, sview);
        perspective_rh_zo(radiansf(cam->FOV), 1.0f, cam->zNear, cam->zFar, sproj);
        sproj[5] *= -1.0f;
        look_at_rh(pos, look, up, cview);
        perspective_rh_zo(radiansf(cam->FOV), (float)c->W / (float)c->H, cam->zNear, cam->zFar, cproj);
        memcpy(c->cam.Model, l2w, 64); memcpy(c->cam.View, cview, 64); memcpy(c->cam.Proj, cproj, 64);
        c->cam.Proj[5] *= -1.0f;
        zr_mat4_mul(cproj, cview, V->ViewProjSpace);
        zr_mat4_mul(sproj, sview, V->ShadowmapSpace);
        memcpy(V->LocalToWorld, l2w, 64);
        V->CameraInfo[0] = pos.x; V->CameraInfo[1] = pos.y; V->CameraInfo[2] = pos.z; V->CameraInfo[3] = cam->FOV;
        V->ViewportInfo[0] = (float)c->W; V->ViewportInfo[1] = (float)c->H; V->ViewportInfo[2] = 0.0f; V->ViewportInfo[3] = 0.0f;
        const uint32_t N = n_point;
        for (uint32_t i = 0; i < N; ++i) {           // point lights ride a spiral, JSON positions are overwritten (ZE:4637-4646)
            const float deg = ((float)i / (float)N) * 360.0f - roll_light * 100.0f;
            const float distance = ((float)i / (float)N) * 5.0f + 2.5f;
            V->PointLights[i].Position[0] = sinf(radiansf(deg)) * distance;
            V->PointLights[i].Position[1] = cosf(radiansf(deg)) * distance;
            V->PointLights[i].Position[2] = 1.5f;
            V->PointLights[i].Position[3] = 1.0f;
        }
        V->Time = time; V->zNear = cam->zNear; V->zFar = cam->zFar;
        memcpy(c->shadow.Model, l2w, 64); memcpy(c->shadow.View, sview, 64); memcpy(c->shadow.Proj, sproj, 64);
        c->frame_valid = true;
        return ZR_OK;
    });
}

extern "C" int zr_set_frame(zr_ctx* c, const XkUniformBufferMVP* cam, const XkUniformBufferMVP* sh, const XkView* v)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, cam && sh && v);
        ARGCHK(c, v->LightsCount[0] >= 0 && v->LightsCount[0] <= XK_MAX_DIRECTIONAL_LIGHTS_NUM && v->LightsCount[1] >= 0 &&
                  v->LightsCount[1] <= XK_MAX_POINT_LIGHTS_NUM);
        if (int rc = zr_stage_idle(c, "zr_set_frame")) return rc;
        c->cam = *cam; c->shadow = *sh; c->view = *v; c->view_dirty = true;
        c->frame_valid = true;
        return ZR_OK;
    });
}
extern "C" int zr_get_frame(zr_ctx* c, XkUniformBufferMVP* cam, XkUniformBufferMVP* sh, XkView* v)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (cam) *cam = c->cam;
        if (sh) *sh = c->shadow;
        if (v) *v = c->view;
        return ZR_OK;
    });
}
extern "C" int zr_set_debug_view(zr_ctx* c, uint32_t s) { if (!c) return ZR_ERR_ARG; return zr_guard(c, [&]() -> int { c->debug_view = s; return ZR_OK; }); }

// The winner planes: one per GBuffer copy, made on first use (every pixel "none"; pixels of other ranks' tiles stay so).  The resolve keeps
// each pixel's winning primitive id in them while the forward variant shades from them or id capture reads them (`what`: the caller, for the message).
int set_winner_planes(zr_ctx* c, bool forward, bool id_capture, const char* what)
{
    const size_t n = (size_t)c->W * c->H;
    for (FrameCopy& F : c->fc) {
        if ((forward || id_capture) && !F.prim_plane) {
            if (c->own.alloc(&F.prim_plane, n) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, std::string(what) + ": out of device memory");
            HIPCHK(c, zr_fill_sync({ { F.prim_plane, 0xFF, n * 4 } }));
        }
        F.G.prim = (forward || id_capture) ? F.prim_plane : nullptr;
    }
    zr_surface_changed(c);      // (a copy resolved without the plane does not hold it: no kept GBuffer across the swap)
    return ZR_OK;
}

// Forward variant (SH/Base.frag): the resolve additionally keeps each pixel's winning primitive id (set_winner_planes), and the lighting
// step runs k_forward on those instead of k_lighting on the GBuffer.
extern "C" int zr_set_shading(zr_ctx* c, uint32_t mode)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (mode != ZR_SHADING_DEFERRED && mode != ZR_SHADING_FORWARD) return zr_fail(c, ZR_ERR_ARG, "zr_set_shading: unknown mode");
        if (int rc = zr_stage_idle(c, "zr_set_shading", false)) return rc;
        if (mode == c->shading) return ZR_OK;
        HIPCHK(c, hipSetDevice(c->device));
        // frames in flight read / write the planes this call swaps in or out
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->cam_s) HIPCHK(c, hipStreamSynchronize(c->cam_s));
        const int rc = set_winner_planes(c, mode == ZR_SHADING_FORWARD, c->id_capture, "zr_set_shading");
        if (rc) return rc;
        c->shading = mode;
        return ZR_OK;
    });
}

static bool finite16(const float* m) { for (int i = 0; i < 16; ++i) if (!std::isfinite(m[i])) return false; return true; }
static bool rigid3(const float* m)     // upper 3x3 orthonormal, det > 0, last row 0 0 0 1
{
    const zf3 a = zr3(m[0], m[1], m[2]), b = zr3(m[4], m[5], m[6]), cc = zr3(m[8], m[9], m[10]);
    const float e = 1e-3f;
    if (fabsf(zr_dot(a, a) - 1) > e || fabsf(zr_dot(b, b) - 1) > e || fabsf(zr_dot(cc, cc) - 1) > e) return false;
    if (fabsf(zr_dot(a, b)) > e || fabsf(zr_dot(a, cc)) > e || fabsf(zr_dot(b, cc)) > e) return false;
    if (zr_dot(zr_cross(a, b), cc) <= 0) return false;
    return m[3] == 0 && m[7] == 0 && m[11] == 0 && m[15] == 1;
}

// Builds the kernarg block of one geometry pass.  Returns false when the pass cannot produce a fragment
// (non-finite PVM: every vertex is non-finite and every triangle is discarded).
static bool build_pass(const zr_ctx* c, const XkUniformBufferMVP& u, int mode, ZrPass* P)
{
    memset(P, 0, sizeof *P);
    float pv[16];
    zr_mat4_mul(u.Proj, u.View, pv);
    zr_mat4_mul(pv, u.Model, P->PVM);           // proj * view * model, left to right
    memcpy(P->M, u.Model, 64);
    P->mode = (uint32_t)mode;
    P->W = mode == ZR_MODE_SHADOW ? c->SD : c->W; P->H = mode == ZR_MODE_SHADOW ? c->SD : c->H;
    P->hw = 0.5f * (float)P->W; P->hh = 0.5f * (float)P->H;
    P->tiles_x = mode == ZR_MODE_SHADOW ? c->stiles_x : c->tiles_x; P->tiles_y = mode == ZR_MODE_SHADOW ? c->stiles_y : c->tiles_y;
    P->tile_rank = mode == ZR_MODE_SHADOW ? c->stile_rank : c->cfg.tile_rank; P->tile_world = mode == ZR_MODE_SHADOW ? c->stile_world : c->cfg.tile_world;
    P->inst_rank = mode == ZR_MODE_SHADOW ? c->shadow_rank : 0; P->inst_world = mode == ZR_MODE_SHADOW ? c->shadow_world : 1;
    P->images = !c->any_images ? 0u : c->mixed_images ? 2u : 1u;     // 1: every material with images has the packed form
    P->n_objects = c->n_objs; P->n_work = c->n_work; P->n_inst_total = c->n_inst_total; P->bin_capacity = c->bin_capacity;
    // the instance-level pre-pass pays for itself on big scenes; small ones go straight to a lane per meshlet-instance - unless this
    // context owns a share of the tiles (below): then the pre-pass leaves a RANK-LOCAL list and the culls walk 1 / N of the scene
    P->use_worklist = c->n_inst_total >= 65536u ? 1u : 0u;
    P->debug_skip = c->env_skip;
    if (ZR_TILE == 32) {      // (both passes: the shadow pass uses it for the instance-level "no texel centre" reject)
        // sphere_bounds() needs clip.x = p00 * x_view, clip.y = p11 * y_view, clip.z = p10 * z_view + p14, clip.w = -z_view and
        // view-space radii = object radii
        const float* pr = u.Proj;
        const bool centred = pr[1] == 0 && pr[2] == 0 && pr[3] == 0 && pr[4] == 0 && pr[6] == 0 && pr[7] == 0 && pr[8] == 0 && pr[9] == 0 &&
                             pr[11] == -1.0f && pr[12] == 0 && pr[13] == 0 && pr[15] == 0 && std::isfinite(pr[0]) && std::isfinite(pr[5]) &&
                             pr[0] != 0 && pr[5] != 0 && std::isfinite(pr[10]) && std::isfinite(pr[14]) && pr[14] < 0;
        zr_mat4_mul(u.View, u.Model, P->VM);
        P->p00 = pr[0]; P->p11 = pr[5];
        P->pz_a = -pr[10]; P->pz_b = pr[14];       // z_view = -d: (p10 * -d + p14) / d
        P->sphere_ok = (centred && rigid3(u.Model) && rigid3(u.View) && finite16(P->VM)) ? 1u : 0u;
        // (both passes: the camera pass against the frame's tiles, the shadow pass against the map's when the map is owned by tiles)
        P->rect_cull = (P->sphere_ok && P->tile_world > 1 && !(c->cfg.flags & ZR_FLAG_NO_RECT_CULL)) ? 1u : 0u;
        if (P->rect_cull) P->use_worklist = 1u;
    }
    {
        static const float ident[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
        P->m_identity = memcmp(u.Model, ident, 64) == 0 ? 1u : 0u;      // bitwise: a -0 entry would not do
    }
    if (!finite16(P->PVM)) return false;
    // frustum planes of proj*view in world space (sphere centres are taken to world space by M in the kernel)
    bool fr_ok = !(c->cfg.flags & ZR_FLAG_NO_FRUSTUM_CULL) && finite16(u.Model);
    if (fr_ok) {
        float rows[6][4];
        for (int k = 0; k < 4; ++k) {
            const float r0 = pv[k * 4 + 0], r1 = pv[k * 4 + 1], r2 = pv[k * 4 + 2], r3 = pv[k * 4 + 3];
            rows[0][k] = r3 + r0; rows[1][k] = r3 - r0; rows[2][k] = r3 + r1; rows[3][k] = r3 - r1; rows[4][k] = r2; rows[5][k] = r3 - r2;
        }
        for (int i = 0; i < 6 && fr_ok; ++i) {
            const float l = sqrtf(rows[i][0] * rows[i][0] + rows[i][1] * rows[i][1] + rows[i][2] * rows[i][2]);
            if (!(l > 1e-20f) || !std::isfinite(l)) { fr_ok = false; break; }
            for (int k = 0; k < 4; ++k) P->planes[i][k] = rows[i][k] / l;
        }
    }
    const bool m_rigid = rigid3(u.Model);
    if (m_rigid) P->m_scale = 1.002f;
    else { float s = 0; for (int cidx = 0; cidx < 3; ++cidx) for (int r = 0; r < 3; ++r) s += u.Model[cidx * 4 + r] * u.Model[cidx * 4 + r]; P->m_scale = sqrtf(s) * 1.002f; }
    if (!std::isfinite(P->m_scale)) fr_ok = false;
    P->frustum_ok = fr_ok ? 1u : 0u;
    // cone culling needs: rigid model and view, a perspective projection with its eye at the view origin, and the
    // engine's handedness (Proj[0][0] > 0, Proj[1][1] < 0 after the Vulkan y-flip, ZE:4624) so that CCW = front
    bool cone = mode == ZR_MODE_GBUFFER && !(c->cfg.flags & ZR_FLAG_NO_CONE_CULL) && m_rigid && rigid3(u.View);
    const float* pr = u.Proj;
    cone = cone && pr[3] == 0 && pr[7] == 0 && pr[11] == -1.0f && pr[15] == 0 && pr[1] == 0 && pr[2] == 0 && pr[4] == 0 && pr[6] == 0 &&
           pr[12] == 0 && pr[13] == 0 && pr[0] > 0 && pr[5] < 0;
    if (cone) {     // eye = -R^T t
        const float* v = u.View;
        P->cam_pos[0] = -(v[0] * v[12] + v[1] * v[13] + v[2] * v[14]);
        P->cam_pos[1] = -(v[4] * v[12] + v[5] * v[13] + v[6] * v[14]);
        P->cam_pos[2] = -(v[8] * v[12] + v[9] * v[13] + v[10] * v[14]);
    }
    P->cone_ok = cone ? 1u : 0u;
    return true;
}

// ------------------------------------------------------------------------------------------------ the frame

// Contexts whose map is never kept (every frame draws it): the host reduces or gathers a partitioned or caller-owned map in place;
// ZR_FLAG_NO_LIST_REUSE asks to recompute what standing inputs would let the library keep; ZR_FLAG_SHADOW_OCCLUSION forces a variant of
// the pass for A/B, whose per-frame history statistics are what its callers read.
static inline bool shadow_keepable(const zr_ctx* c)
{
    return !c->d_shadow_ext && c->cfg.tile_world <= 1u && c->shadow_world <= 1u && c->stile_world <= 1u &&
           !(c->cfg.flags & (ZR_FLAG_NO_LIST_REUSE | ZR_FLAG_SHADOW_OCCLUSION));
}

// Contexts that never keep round 2 of the camera pass (every two-round frame draws it): ZR_FLAG_NO_LIST_REUSE, as above.  A rank of a
// tile-partitioned frame keeps it like any other context: the statement is per pixel, and a rank's key buffer holds its own tiles only.
static inline bool camera_keepable(const zr_ctx* c)
{
    return !(c->cfg.flags & ZR_FLAG_NO_LIST_REUSE);
}

// count -> scan -> fill of the shadow pass's meshlet bins, from the cull's rects.  Z.phase 1 (occlusion culling): only the
// meshlet-instances flagged last frame are binned.
static void shadow_bin(zr_ctx* c, const ZrPass& P, const ZrHiz& Z, hipStream_t s)
{
    const zr_ctx::ShadowBins& sb = c->sb;
    const uint32_t *work = c->sc[0].work, *rects = c->sc[0].rects;
    zr_launch_bin_count(P, work, rects, sb.tile_count, Z, c->d_sstats, s);
    // A rank that owns a share of the shadow MAP (zr_set_shadow_tiles, four ranks or more) has a small pass beside a camera lane that is as
    // busy as ever: units of 128 entries on half the persistent grid leave that lane more of the machine (a rank of eight at config 4:
    // 0.779 -> 0.752 ms; 32 / 16 entries: 0.88 / 1.05 ms; 256: 0.754).  Units only get bigger here: the chunk table's capacity holds.
    const uint32_t chunk = c->stile_world >= 4u ? 2u * ZR_CHUNK : ZR_CHUNK;
    zr_launch_scan(sb.tile_count, sb.tile_offset, sb.tile_cursor, sb.chunk_offset, sb.chunk_tab, c->chunk_capacity, c->sn_tiles, c->bin_capacity,
                   c->d_sstats, 0, s, chunk);
    zr_launch_bin_fill(P, c->d_objs, work, rects, sb.tile_offset, sb.tile_cursor, sb.bins, Z, c->d_sstats, s);
}
// Which meshlet-instances round 2 of the camera pass draws (k_select: timed with the Hi-Z build; round 1's list comes from the cull).
static void tri_select(zr_ctx* c, const ZrPass& P, const ZrHiz& Z, int slot, hipStream_t s)
{
    zr_launch_select(P, c->d_objs, c->sc[1].work, c->sc[1].rects, Z, c->tb, c->d_stats, slot, s);
}
// One round of the triangle-binned camera pass: triangles -> records in their tiles' buckets (k_geom), tile raster (k_tile).  The buckets were
// laid out by the previous frame's k_plan; `count_first`: there is no usable plan (first frame of a scene, or the last plan was made by a
// two-round frame and this round draws everything) - k_geom runs once more ahead of the round, counting only, and k_plan lays the buckets
// out from that.
static void tri_raster(zr_ctx* c, const ZrPass& P, const ZrHiz& Z, int slot, hipStream_t s, bool last, bool count_first)
{
    if (P.n_work == 0) return;          // nothing to draw: the pass is its clear
    if (count_first) {
        zr_launch_geom(P, Z, c->tb, c->d_stats, slot, true, s);
        zr_launch_plan(c->tb, c->d_owned, c->n_owned, c->d_stats, true, c->bucket_pct, s);      // (exact: the round that follows appends what was just counted)
    }
    zr_launch_geom(P, Z, c->tb, c->d_stats, slot, false, s);
    // (the frame's last round also draws the slow triangles of both rounds: k_tile<LAST>)
    zr_launch_tile(P, c->tb, c->d_stats, slot, c->d_vis[c->fcur], c->raster_blocks, s, last, c->d_owned, c->n_owned);
}
// the shadow rasteriser over the bins (stage: see zr_launch_raster_chunks)
static void raster(zr_ctx* c, const ZrPass& P, hipStream_t s, int stage)
{
    zr_launch_raster_chunks(P, c->d_objs, c->sb.chunk_tab, c->sb.bins, c->d_sstats, 0, (uint32_t*)shadow_buf(c),
                            c->stile_world >= 4u ? c->shadow_blocks / 2u : c->shadow_blocks, s, c->d_slow0, c->slow0_cap, c->d_sowned, c->sn_tiles, stage);
}

// What a frame keeps of the frame before, decided once its two pass blocks are built (frame_begin) and before anything is enqueued;
// rebuild: the work lists this frame rebuilds, lane: its camera pipeline would run on the library's own stream.
static void keep_decisions(zr_ctx* c, uint32_t rebuild, bool lane)
{
    // the shadow pass's map as a whole while its block stands, no caster changed and the map stays where it is (shadow_pass)
    c->shadow_keep = shadow_keepable(c) && c->smap_valid && c->smap_epoch == c->caster_epoch && memcmp(&c->smap_key, &c->pass[0], sizeof(ZrPass)) == 0;
    // round 2 of the camera pass while the frame enqueued last drew or kept it from this very block, on a history of this very block, and
    // nothing the pass draws changed since (gbuffer_pass)
    c->frame_cam_epoch = c->camera_epoch;
    c->cam_same = c->cam_prev_valid && c->cam_prev_epoch == c->camera_epoch && memcmp(&c->cam_prev_key, &c->pass[1], sizeof(ZrPass)) == 0;
    c->round2_keep = camera_keepable(c) && c->cam_same && c->r2_settled;
    // the camera pass as a whole, GBuffer included, while beyond that nothing the resolve reads changed (surface_epoch) and both copies
    // of the GBuffer were resolved from these very inputs (g_gen: which run of equal inputs this frame belongs to): after two drawn frames
    // of one run the copies are the same bit for bit, and the frame lights its parity's copy.  Not with a skydome or while a copy still
    // waits for its overlay wipe (the sky key plane is single-buffered, see resolve_on_host_lane).  Such a frame enqueues nothing of the
    // camera pipeline and touches nothing of the lane's.
    if (!c->cam_same || c->surf_prev_epoch != c->surface_epoch) c->g_gen++;
    c->surf_prev_epoch = c->surface_epoch;
    const bool settled = c->round2_keep && !(rebuild & 2u) && c->vis_history && c->plan_valid && c->pass[1].n_work != 0 && !(c->cfg.flags & ZR_FLAG_NO_HIZ);
    const bool copies = c->fc[0].g_gen == c->g_gen && c->fc[1].g_gen == c->g_gen && !c->fc[0].overlay_dirty && !c->fc[1].overlay_dirty;
    c->camera_keep = settled && copies && !(c->sky_set && c->sky_enabled);
    // Its head - upload and one-pixel launch - runs on the idle lane where zr_render keeps the map too (ZR_KEPT_HEAD_ON_LANE).  The one-pixel
    // launch reads the map, and the lane has waited for the end of frame_no - 2 only: the map must have been drawn by that frame or an
    // earlier one (a map drawn by the frame before, on the host's stream, is behind nothing the lane has waited for).
    c->head_on_lane = ZR_KEPT_HEAD_ON_LANE && c->camera_keep && c->in_render && c->shadow_keep && lane && c->smap_frame + 2 <= c->frame_no;
}

// The frame in three stages so that a multi-GPU host can put collectives between them (zeldaengine_amd/dist.py):
//   zr_render_shadow    shadow pass (ZE:3239-3393) of this rank's share of the instances
//   zr_render_gbuffer   deferred-scene pass (ZE:3417-3480): cull + bin + raster + resolve of the owned tiles
//   zr_render_lighting  deferred-lighting pass (ZE:3531-3540) [+ skydome / background overlay]
// zr_render = all three.
// Start of a frame on stream s: pick this frame's copies of the double-buffered resources (key buffer included), make s wait until the
// frame that last used them (two frames ago: its resolve, if that ran on the host's stream, and its lighting pass) is done, reset the
// camera lane's statistics, upload the uniforms if this copy does not hold them yet.
static int frame_begin(zr_ctx* c, hipStream_t s)
{
    if (!c->frame_valid) return zr_fail(c, ZR_ERR_STATE, "no frame uniforms: call zr_update_uniforms or zr_set_frame first");
    if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_render_shadow out of order");
    if (c->debug_view == 9u && c->cfg.tile_world > 1u)
        return zr_fail(c, ZR_ERR_STATE, "debug view 9 (GBufferVis) re-samples the whole GBuffer: not available on a tile-partitioned context");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = zr_scene_finalize(c);
    if (rc) return rc;
    if (c->view.LightsCount[3] != (int32_t)c->cube_levels) { c->view.LightsCount[3] = (int32_t)c->cube_levels; c->view_dirty = true; }
    c->ids_frame = false; c->ids_this = c->id_capture;      // (the frame enqueued last is about to be this one)
    if (c->id_capture) { rc = ids_prepare(c); if (rc) return rc; }
    c->fcur = (int)(c->frame_no & 1u);
    FrameCopy& F = c->fc[c->fcur];
    // the frame's two geometry passes; a pass's work list on the device is rebuilt only when its block or the scene changed
    uint32_t rebuild = 0;
    for (int slot = 0; slot < 2; ++slot) {
        ZrPass& P = c->pass[slot];
        c->pass_live[slot] = build_pass(c, slot == 0 ? c->shadow : c->cam, slot == 0 ? ZR_MODE_SHADOW : ZR_MODE_GBUFFER, &P);
        if (!c->pass_live[slot]) P.n_work = 0;      // no finite vertex: the pass is its clear
        c->list_reuse[slot] = P.use_worklist && P.n_work != 0 && c->list_valid[slot] && memcmp(&c->list_key[slot], &P, sizeof P) == 0 &&
                              !(c->cfg.flags & ZR_FLAG_NO_LIST_REUSE);
        // (the list counts as standing only once its k_cull_instances has been enqueued: shadow_pass / gbuffer_pass set list_valid)
        if (P.use_worklist && P.n_work != 0 && !c->list_reuse[slot]) { rebuild |= 1u << slot; c->list_key[slot] = P; c->list_valid[slot] = false; }
    }
    keep_decisions(c, rebuild, s != c->stream);
    if (c->camera_keep && !c->head_on_lane) s = c->stream;
    // (two lanes: this frame's copies of the double-buffered resources were last used two frames ago, on the host's stream: read by the
    // lighting pass, and before it the keys reset and the GBuffer written by the resolve where that ran there.  Nothing else ties the lanes
    // together here: the shadow pipeline and a host-lane resolve keep statistics of their own)
    if (s != c->stream && c->frame_no >= 2) HIPCHK(c, hipStreamWaitEvent(s, c->ev_end[(c->frame_no - 2) % zr_ctx::END_RING], 0));
    // Consecutive camera pipelines share the triangle records, the plan and the camera lane's statistics (the key buffer is one of a pair,
    // like F), and are ordered by running on ONE stream.  A frame on the lane that follows a frame of the staged entry points (its camera
    // pipeline ran on the host's stream) waits for that frame's end instead.  The other way round the host's stream has waited for ev_cam
    // before that frame's lighting pass: the whole lane, k_plan included - unless that frame resolved on the host's stream, whose ev_cam
    // sits ahead of k_plan; then this frame's camera pipeline, if it runs on the host's stream, waits for the lane's end here.
    if (s != c->stream && c->frame_no >= 1 && c->gbuf_s && c->gbuf_s != s)
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_end[(c->frame_no - 1) % zr_ctx::END_RING], 0));
    // (a frame that keeps its camera pass touches nothing of the lane's: the wait, and the census's below, are left to the next drawn frame)
    if (!c->camera_keep && c->plan_behind_cam && s == c->stream && c->cam_s) { HIPCHK(c, hipEventRecord(c->ev_lane, c->cam_s)); HIPCHK(c, hipStreamWaitEvent(s, c->ev_lane, 0)); }
    if (!c->camera_keep) c->plan_behind_cam = false;
    // ... and by an identity census enqueued against them since (zr_instance_coverage_async, on the host's stream)
    if (F.ids_wait && !c->camera_keep) { if (s != c->stream) HIPCHK(c, hipStreamWaitEvent(s, F.ev_ids, 0)); F.ids_wait = false; }
    // this frame's draw table; the updates since the last frame of this parity go into its planes and sets, s behind the last texture update
    rc = zr_update_frame(c, s, c->fcur);
    if (rc) return rc;
    c->timing_now = c->timing_interval != 0 && c->frame_no % c->timing_interval == 0;     // pass events cost ~6 us of stream bubble each
    if (zr_ctx::TimedFrame* T = c->timed_frame()) HIPCHK(c, hipEventRecord(T->ev[zr_ctx::EV_BEGIN], s));
    if (c->view_dirty) { c->view_version++; c->view_dirty = false; }
    const XkView* src = nullptr;
    uint32_t k = 0;
    if (F.view_uploaded != c->view_version) {        // pinned ring slot: reused only after the kernel that read it last has run
        k = c->view_slot++ % zr_ctx::VIEW_RING;
        HIPCHK(c, hipEventSynchronize(c->view_ev[k]));
        memcpy(&c->h_view_ring[k], &c->view, sizeof(XkView));
        src = &c->h_view_ring[k];
    }
    c->list_rebuild_mask = rebuild;
    // zeroes the camera lane's statistics (the sticky overflow latch survives) and - when the camera list is rebuilt - its length; uploads
    // XkView.  The SHADOW list's length lives in the shadow pipeline's block and is reset on that pipeline's own stream (shadow_pass):
    // the previous frame's shadow pipeline may still be walking it while this kernel runs on the camera lane.
    // (a frame that keeps its camera pass keeps that pass's statistics: an upload, or nothing)
    if (!c->camera_keep || src) zr_launch_frame_begin(c->camera_keep ? nullptr : c->d_stats, src, F.view, c->camera_keep ? 0u : rebuild & 2u, s);
    if (src) { HIPCHK(c, hipEventRecord(c->view_ev[k], s)); F.view_uploaded = c->view_version; }
    return ZR_OK;
}

// shadow pass (ZE:3239-3393) of this rank's share of the instances, on stream s
static int shadow_pass(zr_ctx* c, hipStream_t s)
{
    zr_ctx::TimedFrame* const T = c->timed_frame();
    hipEvent_t* const ev = T ? T->ev : nullptr;
    const ZrPass& P = c->pass[0];      // (built by frame_begin)
    if (ev) T->kept = c->shadow_keep;
    if (c->shadow_keep) {
        // The map of the last drawn pass is this frame's, bit for bit: nothing is launched.  Its statistics block, last_work[0] and the
        // occlusion flags stay as that pass left them; a timed frame records its two events all the same (no elapsed-time call meets an
        // unrecorded one), and the sample counts as 0 (zr_get_pass_times_avg).
        if (ev) { HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_SHADOW_BINS], s)); HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_SHADOW], s)); }
        return ZR_OK;
    }
    c->last_work[0] = P.n_work;
    c->smap_valid = false;             // (until the whole pass is enqueued)
    // The pass draws into the copy that does NOT hold the current map and makes it the current one: from here on shadow_buf() is the map
    // being drawn.  No event guards the flip: everything that reads or writes either copy - this pipeline, the lighting passes and their
    // fused clear, the read-backs and copies - is enqueued on the host's stream, in frame order.
    if (!c->d_shadow_ext) c->smap ^= 1;
    // clear depth 1.0 (ZE:3248): a lighting pass since the copy's last draw already did it for the internal double-buffered map
    FrameCopy& F = c->fc[c->smap];
    if (c->d_shadow_ext || !F.shadow_cleared) zr_launch_fill32((uint32_t*)shadow_buf(c), 0x3F800000u, (size_t)c->SD * c->SD, s);
    F.shadow_cleared = false;
    ZrHiz Z; memset(&Z, 0, sizeof Z);
    // occlusion culling (k_shadow_occlusion): the first launch draws what was not hidden last frame, the rest is tested against the map.
    // It pays when casters pile up behind each other: the test + the late launch cost what a quarter of config 3's rasteriser does
    // (0.1 meshlet-instances per texel: 25 % hidden, frame 2.7 % slower); the same spheres at 0.21 / 0.31 / 0.52 per texel: frame 2 /
    // 8 / 10.5 % faster (tools/occlusion_threshold.py); 1 M instances (10 per texel): 10 % - on by itself from one per five texels.
    const bool occl = !(c->cfg.flags & ZR_FLAG_NO_SHADOW_OCCLUSION) && P.n_work != 0 && ZR_TILE == 32 && c->SD >= 4u &&
                      ((c->cfg.flags & ZR_FLAG_SHADOW_OCCLUSION) || 5ull * P.n_work >= (uint64_t)c->SD * c->SD);
    if (occl) { Z.pxrect = c->d_spxrect; Z.zmin = c->d_szmin; Z.vis_prev = c->d_sflag; Z.vis_stamp = 1u; Z.phase = 1u; }      // (the pass's own flags are 0 / 1)
    // a rebuilt work list starts from length 0 - zeroed HERE, in stream order behind the previous frame's shadow pipeline (k_cull_instances
    // grows it, every later kernel of the pipeline reads it)
    if (c->list_rebuild_mask & 1u) zr_launch_fill32(&c->d_sstats->n_vis_work[0], 0u, 1, s);
    zr_launch_cull_box(P, c->d_objs, c->sc[0].work, c->sc[0].rects, Z, c->d_sstats, 0, s, nullptr, nullptr, c->list_reuse[0]);
    if (c->list_rebuild_mask & 1u) c->list_valid[0] = true;
    shadow_bin(c, P, Z, s);
    if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_SHADOW_BINS], s));
    raster(c, P, s, occl ? 1 : 0);
    if (occl) {
        zr_launch_shadow_occlusion(P, c->d_objs, c->sc[0].work, c->sc[0].rects, c->d_spxrect, c->d_szmin, c->d_sflag, (const uint32_t*)shadow_buf(c),
                                   c->sb.bins, c->d_sstats, c->shadow_blocks * 8u, c->sflag_history ? (uint32_t)((c->shadow_draws + c->sflag_turn) & 3u) : 4u, s);      // (a turn per pass DRAWN: kept frames test nothing)
        c->sflag_history = true;
        raster(c, P, s, 2);
    }
    if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_SHADOW], s));
    HIPCHK(c, hipGetLastError());
    c->shadow_draws++;
    c->smap_key = P; c->smap_epoch = c->caster_epoch; c->smap_valid = true; c->smap_frame = c->frame_no;
    return ZR_OK;
}

// Where the frame's resolve runs.  Nothing later on the camera lane of the same frame needs its planes: only the same frame's lighting
// pass reads them, on the host's stream.  In a frame that keeps its shadow map that stream has nothing else to do, and the camera lane's
// chain of launches is the frame's period: the resolve then goes to the host's stream, ahead of the lighting pass, and k_mark leaves the
// next frame's camera lane the visibility history.  Only zr_render does this (a host may read the GBuffer after zr_render_geometry, and
// the staged entry points run on one stream anyway), only on two lanes, and not with a skydome (its key plane is single-buffered).
// (shadow_keep already implies an unpartitioned context: shadow_keepable.)
static inline bool resolve_on_host_lane(const zr_ctx* c, bool lanes)
{
    return lanes && c->in_render && c->shadow_keep && !(c->sky_set && c->sky_enabled);
}

// deferred-scene pass (ZE:3417-3480): cull + bin + raster + resolve of the owned tiles, on stream s.  defer_resolve: see above - the
// resolve is left to zr_render_lighting (deferred_resolve), the lane ends k_mark -> ev_cam -> k_plan.
static int gbuffer_pass(zr_ctx* c, hipStream_t s, bool defer_resolve = false)
{
    zr_ctx::TimedFrame* const T = c->timed_frame();
    hipEvent_t* const ev = T ? T->ev : nullptr;
    if (ev) { T->kept_camera = c->camera_keep; HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_CAMERA], s)); }
    if (c->camera_keep) {
        // The camera pass kept whole (frame_begin): both GBuffer copies, the key buffers, the visibility history and its stamp, the plan,
        // the statistics block and cov_block stay as the last drawn frame left them, and nothing is launched.  A timed frame records the
        // pass's events all the same, on the stream that lights it, and counts 0 for the cull, both rounds, Hi-Z and the resolve.
        if (ev) {
            T->kept_round2 = true; T->moved = false;
            for (int e : { zr_ctx::EV_CULL, zr_ctx::EV_ROUND1, zr_ctx::EV_HIZ, zr_ctx::EV_ROUND2, zr_ctx::EV_RESOLVE }) HIPCHK(c, hipEventRecord(ev[e], s));
        }
        return ZR_OK;
    }
    ZrPass P = c->pass[1];             // (built by frame_begin; the overlay fields are set below)
    c->gbuf_s = s;
    c->last_work[1] = P.n_work;
    c->r2_settled = c->cam_prev_valid = false;      // (until the whole pass is enqueued; frame_begin has read them)
    // Two-pass occlusion culling: round 1 draws the meshlet-instances that owned a pixel last frame, a Hi-Z pyramid of the
    // result rejects what it hides, round 2 draws the rest.  The depth test decides every pixel either way, so the frame does
    // not depend on the history; without one (first frame of a scene) or with ZR_FLAG_NO_HIZ everything is drawn at once.
    const bool hiz_on = !(c->cfg.flags & ZR_FLAG_NO_HIZ) && P.n_work != 0;
    ZrHiz Z = c->hiz;
    Z.tiles_x = c->tiles_x; Z.tile_rank = c->cfg.tile_rank; Z.tile_world = c->cfg.tile_world;
    Z.pxrect = hiz_on ? c->d_pxrect : nullptr; Z.zmin = hiz_on ? c->d_zmin : nullptr;
    Z.vis_prev = c->d_visflag[c->vis_cur ^ 1]; Z.vis_now = hiz_on ? c->d_visflag[c->vis_cur] : nullptr;
    // visibility marks are frame stamps (1 .. 255): the resolve writes this frame's, the culls compare with last frame's - nothing is cleared
    // (a stamp per pass DRAWN: a rest of any length leaves the stamps as an uninterrupted run of drawn frames would)
    const uint32_t vis_mark = 1u + (uint32_t)(c->cam_draws % 255u);
    Z.vis_stamp = c->vis_mark_prev;
    Z.phase = 0;
    static_assert(ZR_TILE == 32, "the triangle-binned camera pass is written for 32 x 32 tiles");
    c->last_two_round = hiz_on && c->vis_history;
    // (the cull kernel also compacts round 1's list - the survivors that owned a pixel last frame, or all of them)
    zr_launch_cull_box(P, c->d_objs, c->sc[1].work, c->sc[1].rects, Z, c->d_stats, 1, s, c->tb.sel, c->last_two_round ? Z.vis_prev : nullptr, c->list_reuse[1]);
    if (c->list_rebuild_mask & 2u) c->list_valid[1] = true;
    const bool two = c->last_two_round;
    // (the record buckets are planned from the previous frame: see tri_raster)
    const bool count_first = !c->plan_valid || (!two && c->plan_two_round);
    // Round 2 kept (zr_ctx::camera_epoch): the inputs are the previous frame's bit for bit, so round 1 - what owned a pixel of that frame -
    // leaves this frame's key buffer, and round 1 is the frame's last round: its k_tile draws the slow triangles.  The statistics and the
    // plan are those of round 2 as last drawn (k_plan); a timed frame records its events all the same and counts 0 for both passes.
    const bool keep = two && c->round2_keep && !count_first;
    if (ev) T->kept_round2 = keep;
    if (keep) {
        Z.phase = 1;
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_CULL], s));
        tri_raster(c, P, Z, 1, s, true, false);
        if (ev) { HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_ROUND1], s)); HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_HIZ], s)); }
    } else if (two) {
        Z.phase = 1;
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_CULL], s));
        tri_raster(c, P, Z, 1, s, false, count_first);
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_ROUND1], s));
        zr_launch_hiz_build(c->d_vis[c->fcur], c->W, c->H, Z, c->d_hiz_regions, c->n_hiz_regions, s);
        Z.phase = 2;
        tri_select(c, P, Z, 2, s);
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_HIZ], s));
        tri_raster(c, P, Z, 2, s, true, false);
    } else {
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_CULL], s));
        tri_raster(c, P, Z, 1, s, true, count_first);
        if (ev) { HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_ROUND1], s)); HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_HIZ], s)); }
    }
    {   // the overlay plane (skydome pixels) is written only when a skydome is drawn, or once more to wipe one that was
        const bool sky = c->sky_set && c->sky_enabled;
        P.write_overlay = (sky || c->fc[c->fcur].overlay_dirty) ? 1u : 0u;
        c->fc[c->fcur].overlay_dirty = sky;
        P.sky_keys = nullptr; P.sky_object = c->sky_object;
        if (sky && c->d_sky_keys) { zr_launch_sky_tiles(P, c->d_objs, c->d_owned, c->n_owned, c->d_sky_keys, s); P.sky_keys = c->d_sky_keys; }
    }
    if (ev) { HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_ROUND2], s)); T->moved = defer_resolve; }
    c->resolve_deferred = defer_resolve;
    if (defer_resolve) {
        // the history now, the planes later: the host's stream waits for everything up to here and resolves from the same keys
        zr_launch_mark(P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], Z.vis_now, s, vis_mark);
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_MARK], s));
        c->resolve_P = P; c->resolve_mark = vis_mark;
        HIPCHK(c, hipEventRecord(c->ev_cam, s)); c->camera_on_lane = true; c->plan_behind_cam = true;
    } else {
        zr_launch_resolve_gbuffer(P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], c->fc[c->fcur].G, c->d_lut, c->d_unorm_lut, Z.vis_now, c->d_stats, s, vis_mark);
        c->cov_block = c->d_stats; c->fc[c->fcur].g_gen = c->g_gen;
        if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_RESOLVE], s));
        if (ZR_EV_CAM_AHEAD_OF_PLAN && c->in_render && s != c->stream) { HIPCHK(c, hipEventRecord(c->ev_cam, s)); c->camera_on_lane = true; c->plan_behind_cam = true; }
    }
    c->vis_mark_prev = vis_mark; c->cam_draws++;
    if (P.n_work != 0) {     // the next frame's buckets, from this frame's counts: nothing of this frame waits for it
        zr_launch_plan(c->tb, c->d_owned, c->n_owned, c->d_stats, false, c->bucket_pct, s, keep ? ZR_PLAN_KEPT_ROUND2 : two ? ZR_PLAN_DREW_ROUND2 : ZR_PLAN_ONE_ROUND);
        c->plan_valid = true; c->plan_two_round = two;
    }
    c->r2_settled = two && c->cam_same;
    c->cam_prev_key = c->pass[1]; c->cam_prev_epoch = c->frame_cam_epoch; c->cam_prev_valid = hiz_on;
    if (hiz_on) { c->vis_history = true; c->vis_cur ^= 1; } else c->vis_history = false;
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}

extern "C" int zr_render_shadow(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->camera_on_lane = false;
        int rc = frame_begin(c, c->stream);
        if (rc == ZR_OK) rc = shadow_pass(c, c->stream);
        if (rc == ZR_OK) HIPCHK(c, hipEventRecord(c->ev_join, c->stream));
        if (rc == ZR_OK) c->stage = 1;
        return rc;
    });
}

extern "C" int zr_render_gbuffer(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->stage != 1) return zr_fail(c, ZR_ERR_STATE, "zr_render_gbuffer out of order");
        HIPCHK(c, hipSetDevice(c->device));
        const int rc = gbuffer_pass(c, c->stream);
        if (rc == ZR_OK) c->stage = 2;
        return rc;
    });
}

static int empty_pixel_pass(zr_ctx* c, hipStream_t s);
// Both geometry passes of a frame.  Two lanes (unless ZR_FLAG_SERIAL_PASSES): the camera pipeline on cam_s; the shadow pipeline on
// the host's stream, where the lighting pass will follow.  The next frame's camera pipeline starts as soon as this one's is
// through, next to this frame's lighting; its shadow pipeline follows the lighting.  A frame that keeps its shadow map has no shadow
// pipeline: in zr_render its resolve takes that place on the host's stream (resolve_on_host_lane), next to the next frame's camera
// pipeline.  Never more than two kernels side by side: a third only takes occupancy from the other two (measured).
static int geometry_passes(zr_ctx* c)
{
    const bool lanes = !(c->cfg.flags & ZR_FLAG_SERIAL_PASSES) && c->cam_s != nullptr;
    int rc;
    c->camera_on_lane = false;
    if (lanes) {
        // Every event record / wait is a barrier packet, worth 5-10 us of bubble on the stream it sits on, and the host's stream
        // (lighting -> shadow pipeline -> lighting ...) is the lane the frame rate hangs on: it waits for the camera lane once per frame
        // (before the lighting pass) and for nothing else.  The shadow pipeline needs nothing of frame_begin's - its matrices are kernel
        // arguments, its statistics a block of its own that it resets itself, work-list length included.
        rc = frame_begin(c, c->cam_s);
        if (rc != ZR_OK) return rc;
        rc = shadow_pass(c, c->stream);
        if (rc == ZR_OK && !c->in_render) HIPCHK(c, hipEventRecord(c->ev_join, c->stream));      // (zr_stream_wait_shadow: a host that puts a collective behind the shadow pass)
        const bool defer = resolve_on_host_lane(c, lanes);
        if (rc == ZR_OK) rc = gbuffer_pass(c, c->camera_keep ? c->stream : c->cam_s, defer);      // (kept whole: its events only, where the frame is lit)
        // (a deferred resolve: ev_cam is already recorded, behind k_mark and ahead of k_plan - the lighting lane does not wait for the plan)
        if (rc == ZR_OK && c->head_on_lane) {      // (ZR_KEPT_HEAD_ON_LANE: the one-pixel launch behind the upload, the host's stream behind both)
            rc = empty_pixel_pass(c, c->cam_s);
            if (rc == ZR_OK) { HIPCHK(c, hipEventRecord(c->ev_cam, c->cam_s)); c->camera_on_lane = true; }
        }
        if (rc == ZR_OK && !c->camera_on_lane && !c->camera_keep) { HIPCHK(c, hipEventRecord(c->ev_cam, c->cam_s)); c->camera_on_lane = true; }
    } else {
        rc = frame_begin(c, c->stream);
        if (rc != ZR_OK) return rc;
        rc = shadow_pass(c, c->stream);
        if (rc == ZR_OK) HIPCHK(c, hipEventRecord(c->ev_join, c->stream));
        if (rc == ZR_OK) rc = gbuffer_pass(c, c->stream);
    }
    if (rc == ZR_OK) c->stage = 2;
    return rc;
}

extern "C" int zr_render_geometry(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return geometry_passes(c); });
}

extern "C" int zr_stream_wait_shadow(zr_ctx* c, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, c->ev_join, 0));
        return ZR_OK;
    });
}

static void light_params(const zr_ctx* c, ZrLightParams* Lp)
{
    ZrLightParams& L = *Lp; memset(&L, 0, sizeof L);
    static const float Bias[16] = { 0.5f, 0, 0, 0, 0, 0.5f, 0, 0, 0, 0, 1, 0, 0.5f, 0.5f, 0, 1 };
    zr_mat4_mul(Bias, c->view.ShadowmapSpace, L.SB);
    L.W = c->W; L.H = c->H; L.SD = c->SD; L.tiles_x = c->tiles_x; L.debug_view = c->debug_view;
    L.cube_dim = c->cube_dim; L.cube_levels = c->cube_levels; L.tile_world = c->cfg.tile_world;
    L.packed_out = (c->cfg.tile_world > 1 || (c->cfg.flags & ZR_FLAG_PACKED_TILES)) ? 1u : 0u;
    L.debug_skip = c->env_skip_light;
    L.bg_enabled = (c->bg_set && c->bg_enabled) ? 1u : 0u;
    L.has_overlay = c->fc[c->fcur].overlay_dirty ? 1u : 0u;     // set by this frame's gbuffer pass
    { const int32_t np = c->view.LightsCount[1]; L.light_list = (np >= c->env_light_list_min && np <= XK_MAX_POINT_LIGHTS_NUM) ? 1u : 0u; }
    L.bg.data = c->d_bg; L.bg.w = c->bg_w; L.bg.h = c->bg_h; L.bg.levels = c->bg_levels; L.bg._pad = 0;
}

// The lighting shader's colour for a pixel that still holds every target's clear value: one launch of the lighting kernel over a
// one-pixel GBuffer.  It needs the finished shadow map (PCF at world position 0) and the frame's uniforms, nothing else.  View 6
// (the quad's interpolated vertex colour) depends on the pixel position, so it goes without.
static int empty_pixel_pass(zr_ctx* c, hipStream_t s)
{
    c->empty_ready = false;
    if (c->debug_view == 6u || c->env_no_empty_px || c->shading == ZR_SHADING_FORWARD) return ZR_OK;      // (forward: an empty pixel is the clear colour)
    ZrLightParams L; light_params(c, &L);
    L.W = 1; L.H = 1; L.tiles_x = 1; L.packed_out = 0; L.bg_enabled = 0;
    zr_launch_lighting(L, c->fc[c->fcur].view, c->d_sowned, 1, c->Gclear, shadow_buf(c), c->cube, c->d_lut, c->d_unorm_lut, c->fc[c->fcur].empty_rgba, s);
    HIPCHK(c, hipGetLastError());
    c->empty_ready = true;
    return ZR_OK;
}

// The resolve of a frame whose camera lane left it to the host's stream (gbuffer_pass), behind the wait for ev_cam: same launch, same
// keys; the history is already marked (vis_now = nullptr) and the coverage tally goes to the frame copy's own block, zeroed here.
static int deferred_resolve(zr_ctx* c, hipStream_t s)
{
    zr_ctx::TimedFrame* const T = c->timed_frame();
    hipEvent_t* const ev = T ? T->ev : nullptr;
    ZrDevStats* const tally = c->d_rstats[c->fcur];
    zr_launch_fill32(tally->covered_part, 0u, 32, s);
    if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_HOST_RESOLVE], s));
    zr_launch_resolve_gbuffer(c->resolve_P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], c->fc[c->fcur].G, c->d_lut, c->d_unorm_lut, nullptr, tally, s, c->resolve_mark);
    if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_RESOLVE], s));
    c->cov_block = tally; c->resolve_deferred = false; c->fc[c->fcur].g_gen = c->g_gen;
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}

static int lighting_pass(zr_ctx* c, hipStream_t s)
{
    zr_ctx::TimedFrame* const T = c->timed_frame();
    hipEvent_t* const ev = T ? T->ev : nullptr;
    ZrLightParams L; light_params(c, &L);
    const FrameCopy& F = c->fc[c->fcur];
    L.empty_rgba = c->empty_ready ? F.empty_rgba : nullptr;
    // The next DRAWN shadow pass follows on this stream and rasterises into the OTHER copy of the map, which nothing reads or
    // writes while this pass runs: clear it here - once; a run of frames that keep their map finds it clear and writes nothing.
    FrameCopy& next = c->fc[c->smap ^ 1];
    if (c->n_owned && s == c->stream && !c->d_shadow_ext && !next.shadow_cleared) { L.clear_next = (uint32_t*)next.shadow; L.clear_n = c->SD * c->SD; next.shadow_cleared = true; }
    uint32_t* const frame_out = L.packed_out ? (c->d_tiles_ext ? c->d_tiles_ext : c->d_tiles) : c->d_color;
    if (c->shading == ZR_SHADING_FORWARD) {
        // Base.frag over the winners the resolve recorded, with this frame's camera block (frame_begin built it; the overlay fields play no part)
        if (L.clear_next) { zr_launch_fill32(L.clear_next, 0x3F800000u, L.clear_n, s); L.clear_next = nullptr; }
        zr_launch_forward(c->pass[1], L, F.view, c->d_objs, c->d_owned, c->n_owned, F.G, shadow_buf(c), c->cube, c->d_lut, c->d_unorm_lut, frame_out, s);
    } else {
        zr_launch_lighting(L, F.view, c->d_owned, c->n_owned, F.G, shadow_buf(c), c->cube, c->d_lut, c->d_unorm_lut, frame_out, s);
        if (c->debug_view == 9u)        // GBufferVis mosaic over the lit frame (needs the whole GBuffer: single-rank contexts only)
            zr_launch_gbuffer_vis(L, F.view, F.G, shadow_buf(c), c->cube, c->d_lut, c->d_color, s);
    }
    if (ev) HIPCHK(c, hipEventRecord(ev[zr_ctx::EV_LIGHTING], s));
    HIPCHK(c, hipEventRecord(c->ev_end[c->frame_no % zr_ctx::END_RING], s));      // this frame's GBuffer / shadow map / uniforms copies are free again
    HIPCHK(c, hipGetLastError());
    if (c->timing_now) c->sample_no++;
    c->rendered = true; c->frame_no++; c->stage = 0;
    c->ids_frame = c->ids_this; c->ids.gen = c->scene_gen;
    return ZR_OK;
}

extern "C" int zr_render_lighting(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->stage != 2) return zr_fail(c, ZR_ERR_STATE, "zr_render_lighting out of order");
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t ls = c->stream;
        // The one wait of the host's stream per frame: the camera lane's GBuffer (or, where the resolve follows here, its keys and history
        // marks: ev_cam is then recorded ahead of the lane's k_plan) - and, ahead of it on that lane, this frame's k_frame_begin, whose
        // uniforms the empty-pixel pass below reads (the shadow pipeline before it needed nothing of them and did not wait).
        if (c->camera_on_lane) HIPCHK(c, hipStreamWaitEvent(ls, c->ev_cam, 0));
        int rc = c->resolve_deferred ? deferred_resolve(c, ls) : ZR_OK;
        if (rc == ZR_OK && !c->head_on_lane) rc = empty_pixel_pass(c, ls); // the shadow map (possibly reduced over ranks by the host) is final only now
        if (rc == ZR_OK) rc = lighting_pass(c, ls);
        return rc;
    });
}

// RecordCommandBuffer (ZE:3160-3744) + vkQueueSubmit (ZE:2014): shadow -> deferred scene -> deferred lighting, with two
// frames in flight as in the reference (MAX_FRAMES_IN_FLIGHT, ZE:77).
// The shadow pass and the deferred-scene pass do not depend on each other, and the next frame's geometry does not depend on this
// frame's lighting.  zr_render therefore runs two lanes: the camera pipeline on the library's high-priority stream cam_s, and
// shadow pipeline -> lighting on the host's stream.  Whatever the host enqueues on its stream after zr_render is ordered after
// the finished frame, as before.  ZR_FLAG_SERIAL_PASSES keeps everything on the one stream, as the staged entry points do.
// A frame that keeps its shadow map resolves on the host's stream (resolve_on_host_lane): camera lane ... -> k_tile -> k_mark -> ev_cam
// -> k_plan, host's stream wait -> k_resolve_gbuffer -> one-pixel launch -> k_lighting -> ev_end.
// A frame that keeps its whole camera pass (frame_begin: camera_keep) has no camera pipeline: host's stream upload -> [shadow pipeline] ->
// one-pixel launch -> k_lighting -> ev_end, over the GBuffer copy of its parity as the last two drawn frames left both; where it keeps its
// map too (and has kept it for a frame), upload -> one-pixel launch -> ev_cam run on the lane beside the previous frame's k_lighting, and the host's stream waits for ev_cam.
extern "C" int zr_render(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->in_render = true;
        int rc = geometry_passes(c);
        if (rc == ZR_OK) rc = zr_render_lighting(c);
        c->in_render = false;
        if (rc != ZR_OK) c->stage = 0;
        return rc;
    });
}

// Multi-GPU shadow pass: this context draws instances i with i % world == rank (non-instanced draws count as instance 0).
// The per-rank shadow maps must be min-reduced before zr_render_lighting.  rank 0 / world 1 = the whole scene (default).
extern "C" int zr_set_shadow_partition(zr_ctx* c, uint32_t rank, uint32_t world)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, world >= 1 && rank < world);
        if (world > 1 && c->stile_world > 1) return zr_fail(c, ZR_ERR_STATE, "zr_set_shadow_partition: the map is already owned by tiles (zr_set_shadow_tiles)");
        c->shadow_rank = rank; c->shadow_world = world; zr_casters_changed(c);
        return ZR_OK;
    });
}

// Multi-GPU shadow pass, second form: the MAP is owned by light-space super-tiles exactly as the frame is owned by screen super-tiles
// (zr_tile_owner on the map's 32 x 32-texel tiles).  This context then draws only the casters whose texel box can reach a tile it owns
// (rank-local work list, instance- and meshlet-level rejects before any vertex work) - drawn whole, so its owned tiles are bit for
// bit the single-GPU map's - and the ranks exchange their tiles with ONE all-gather: zr_shadow_pack -> all-gather -> zr_shadow_unpack.
// No reduction: every texel has one owner.  rank 0 / world 1 = the whole map (default).
extern "C" int zr_set_shadow_tiles(zr_ctx* c, uint32_t rank, uint32_t world)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, world >= 1 && rank < world);
        if (int rc = zr_stage_idle(c, "zr_set_shadow_tiles", false)) return rc;
        if (world > 1 && c->shadow_world > 1) return zr_fail(c, ZR_ERR_STATE, "zr_set_shadow_tiles: the casters are already split by instance (zr_set_shadow_partition)");
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->stile_mem.release(); c->d_sowned_rank = c->d_stile_map = nullptr;
        c->stile_rank = 0; c->stile_world = 1; c->s_slots_per_rank = c->sn_tiles; c->n_sowned_rank = 0;
        c->list_valid[0] = false; zr_casters_changed(c);
        if (world == 1) return ZR_OK;
        const ZrTilePartition P = zr_partition(c->stiles_x, c->stiles_y, world, rank);
        HIPCHK(c, upload(c->stile_mem, &c->d_sowned_rank, P.owned)); HIPCHK(c, upload(c->stile_mem, &c->d_stile_map, P.map));
        c->stile_rank = rank; c->stile_world = world; c->s_slots_per_rank = P.slots_per_rank; c->n_sowned_rank = (uint32_t)P.owned.size();
        return ZR_OK;
    });
}
// bytes of one rank's packed share (slots_per_rank tiles of 32 x 32 floats; the all-gathered buffer holds world times that)
extern "C" int zr_shadow_tiles_bytes(zr_ctx* c, size_t* bytes_per_rank)
{
    if (!c || !bytes_per_rank) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        *bytes_per_rank = (size_t)(c->stile_world > 1 ? c->s_slots_per_rank : c->sn_tiles) * ZR_TILE * ZR_TILE * 4;
        return ZR_OK;
    });
}
// The owned tiles of the map just rasterised -> packed_dev (slot k = the k-th owned tile, unused slots keep depth 1.0), on `hip_stream`
// (NULL = the render stream, behind the shadow pass).
extern "C" int zr_shadow_pack(zr_ctx* c, void* packed_dev, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, packed_dev != nullptr);
        if (c->stile_world <= 1) return zr_fail(c, ZR_ERR_STATE, "zr_shadow_pack: the shadow map is not owned by tiles (zr_set_shadow_tiles)");
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
        zr_launch_pack_tiles((const uint32_t*)shadow_buf(c), c->d_sowned_rank, c->n_sowned_rank, (uint32_t*)packed_dev, c->SD, c->SD, c->stiles_x, 0x3F800000u, s);
        HIPCHK(c, hipGetLastError());
        return ZR_OK;
    });
}
// The all-gathered buffer (world x bytes_per_rank, rank-major) -> this frame's shadow map, every tile from its owner, on `hip_stream`
// (NULL = the render stream: call it before zr_render_lighting).
extern "C" int zr_shadow_unpack(zr_ctx* c, const void* gathered_dev, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, gathered_dev != nullptr);
        if (c->stile_world <= 1) return zr_fail(c, ZR_ERR_STATE, "zr_shadow_unpack: the shadow map is not owned by tiles (zr_set_shadow_tiles)");
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
        zr_launch_untile((const uint32_t*)gathered_dev, c->d_stile_map, (uint32_t*)shadow_buf(c), c->SD, c->SD, c->stiles_x, c->sn_tiles, s);
        HIPCHK(c, hipGetLastError());
        return ZR_OK;
    });
}

// Caller-owned shadow map (float[shadow_dim^2], e.g. a torch tensor RCCL reduces in place); NULL = the internal one.
extern "C" int zr_set_shadow_buffer(zr_ctx* c, void* ptr)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->d_shadow_ext = (float*)ptr; zr_casters_changed(c);
        return ZR_OK;
    });
}

