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

// What the schedule reads under its own names (zr_frame_plan.h is plain C++ and sees neither header) is what the library means by them.
static_assert(ZRP_NO_HIZ == ZR_FLAG_NO_HIZ && ZRP_SERIAL_PASSES == ZR_FLAG_SERIAL_PASSES && ZRP_NO_LIST_REUSE == ZR_FLAG_NO_LIST_REUSE &&
              ZRP_NO_SHADOW_OCCLUSION == ZR_FLAG_NO_SHADOW_OCCLUSION && ZRP_SHADOW_OCCLUSION == ZR_FLAG_SHADOW_OCCLUSION &&
              ZRP_SHADING_FORWARD == ZR_SHADING_FORWARD, "zr_frame_plan.h: flags");
static_assert((int)ZR_ROUNDS_ONE == ZR_PLAN_ONE_ROUND && (int)ZR_ROUNDS_TWO == ZR_PLAN_DREW_ROUND2 && (int)ZR_ROUNDS_TWO_KEPT == ZR_PLAN_KEPT_ROUND2, "zr_frame_plan.h: rounds");
static_assert(ZR_TILE == 32, "the triangle-binned camera pass and the shadow pass's occlusion culling are written for 32 x 32 tiles");

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

// What of the uniforms depends on the extent, from the lens of the last zr_update_uniforms (zr_ctx::lens) and the camera's View as that
// call left it: the camera's projection, ViewProjSpace, ViewportInfo.  zr_update_uniforms ends with it, zr_resize calls it again.
void zr_uniforms_reproject(zr_ctx* c)
{
    XkView* V = &c->view;
    float cproj[16];
    perspective_rh_zo(radiansf(c->lens.fov), (float)c->W / (float)c->H, c->lens.zn, c->lens.zf, cproj);
    memcpy(c->cam.Proj, cproj, 64);
    c->cam.Proj[5] *= -1.0f;
    zr_mat4_mul(cproj, c->cam.View, V->ViewProjSpace);
    V->ViewportInfo[0] = (float)c->W; V->ViewportInfo[1] = (float)c->H; V->ViewportInfo[2] = 0.0f; V->ViewportInfo[3] = 0.0f;
    c->view_dirty = true;
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
        float l2w[16], sview[16], sproj[16], cview[16];
        rotate_z(roll_stage, l2w);
        look_at_rh(lightPos, zr3(0.0f, 0.0f, 0.0f), up, sview);
        perspective_rh_zo(radiansf(cam->FOV), 1.0f, cam->zNear, cam->zFar, sproj);
        sproj[5] *= -1.0f;
        look_at_rh(pos, look, up, cview);
        memcpy(c->cam.Model, l2w, 64); memcpy(c->cam.View, cview, 64);
        c->lens.valid = true; c->lens.fov = cam->FOV; c->lens.zn = cam->zNear; c->lens.zf = cam->zFar;
        zr_uniforms_reproject(c);       // cam.Proj, ViewProjSpace, ViewportInfo
        zr_mat4_mul(sproj, sview, V->ShadowmapSpace);
        memcpy(V->LocalToWorld, l2w, 64);
        V->CameraInfo[0] = pos.x; V->CameraInfo[1] = pos.y; V->CameraInfo[2] = pos.z; V->CameraInfo[3] = cam->FOV;
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
        c->frame_valid = true; c->lens.valid = false;      // (the caller's own: a resize leaves them as given)
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
            if (c->ext.alloc(&F.prim_plane, n) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, std::string(what) + ": out of device memory");
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
//
// What a frame does is decided once, by zr_frame_plan() (zr_frame_plan.h), when the frame begins; everything below does what the plan says
// on the stream the plan names, and tells zr_frame_carry() when a stage is enqueued.

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
                   c->d_sstats, s, chunk);
    zr_launch_bin_fill(P, c->d_objs, work, rects, sb.tile_offset, sb.tile_cursor, sb.bins, Z, c->d_sstats, s);
}
// Which meshlet-instances round 2 of the camera pass draws (k_select: timed with the Hi-Z build; round 1's list comes from the cull).
static void tri_select(zr_ctx* c, const ZrPass& P, const ZrHiz& Z, int slot, hipStream_t s)
{
    zr_launch_select(P, c->d_objs, c->sc[1].work, c->sc[1].rects, Z, c->tb, c->d_stats, slot, s);
}
// One round of the triangle-binned camera pass: triangles -> records in their tiles' buckets (k_geom), tile raster (k_tile).  The buckets were
// laid out by the previous frame's k_plan; `count_first` (ZrFramePlan): k_geom runs once more ahead of the round, counting only, and k_plan
// lays the buckets out from that.
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
    zr_launch_raster_chunks(P, c->d_objs, c->sb.chunk_tab, c->sb.bins, c->d_sstats, (uint32_t*)shadow_buf(c),
                            c->stile_world >= 4u ? c->shadow_blocks / 2u : c->shadow_blocks, s, c->d_slow0, c->slow0_cap, c->d_sowned, c->sn_tiles, stage);
}

// The frame in three stages so that a multi-GPU host can put collectives between them (zeldaengine_amd/dist.py):
//   zr_render_shadow    shadow pass (ZE:3239-3393) of this rank's share of the instances
//   zr_render_gbuffer   deferred-scene pass (ZE:3417-3480): cull + bin + raster + resolve of the owned tiles
//   zr_render_lighting  deferred-lighting pass (ZE:3531-3540) [+ skydome / background overlay]
// zr_render = all three.
// Start of a frame: build its two pass blocks, gather what the schedule reads and plan the frame (c->facts, c->plan); then its head, on the
// plan's stream: pick this frame's copies of the double-buffered resources (key buffer included), wait for whoever used them last, reset
// the camera lane's statistics, upload the uniforms if this copy does not hold them yet.
static int frame_begin(zr_ctx* c, ZrEntry entry)
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

    ZrFrameFacts& f = c->facts;
    f.flags = c->cfg.flags; f.tile_world = c->cfg.tile_world; f.shadow_world = c->shadow_world; f.stile_world = c->stile_world;
    f.map_external = c->d_shadow_ext != nullptr; f.sky = c->sky_set && c->sky_enabled; f.shading = c->shading; f.SD = c->SD;
    f.entry = entry; f.has_lane = c->cam_s != nullptr; f.frame_no = c->frame_no;
    f.caster_epoch = c->caster_epoch; f.camera_epoch = c->camera_epoch; f.surface_epoch = c->surface_epoch;
    for (int slot = 0; slot < 2; ++slot) {      // the frame's two geometry passes
        ZrPass& P = c->pass[slot];
        c->pass_live[slot] = build_pass(c, slot == 0 ? c->shadow : c->cam, slot == 0 ? ZR_MODE_SHADOW : ZR_MODE_GBUFFER, &P);
        if (!c->pass_live[slot]) P.n_work = 0;      // no finite vertex: the pass is its clear
        f.n_work[slot] = P.n_work; f.use_worklist[slot] = P.use_worklist != 0;
        f.block_is_list[slot] = memcmp(&c->list_key[slot], &P, sizeof P) == 0;
    }
    for (int i = 0; i < 2; ++i) { f.copy_gen[i] = c->fc[i].g_gen; f.copy_overlay[i] = c->fc[i].overlay_dirty; f.copy_ids_wait[i] = c->fc[i].ids_wait; }
    f.shadow_is_map = memcmp(&c->smap_key, &c->pass[0], sizeof(ZrPass)) == 0;
    f.camera_is_prev = memcmp(&c->cam_prev_key, &c->pass[1], sizeof(ZrPass)) == 0;
    zr_light_facts(c, &f);
    c->plan = zr_frame_plan(f, c->carry);
    if (c->plan.light_fill && !zr_light_plane_make(c)) { f.light_plane_ok = false; c->plan = zr_frame_plan(f, c->carry); }      // (no room for it: plan again, without)
    const ZrFramePlan& p = c->plan;
    c->carry = zr_frame_carry(c->carry, f, p, ZR_STAGE_HEAD);
    if (p.shadow_list_rebuild) c->list_key[0] = c->pass[0];
    if (p.camera_list_rebuild) c->list_key[1] = c->pass[1];

    const hipStream_t s = lane_stream(c, p.head);
    if (p.wait_end2 && (rc = zr_wait_frame_end(c, s, c->frame_no - 2)) != ZR_OK) return rc;
    if (p.wait_end1 && (rc = zr_wait_frame_end(c, s, c->frame_no - 1)) != ZR_OK) return rc;
    if (p.wait_lane_end) { HIPCHK(c, hipEventRecord(c->ev_lane, c->cam_s)); HIPCHK(c, hipStreamWaitEvent(s, c->ev_lane, 0)); }
    if (p.wait_ids) HIPCHK(c, hipStreamWaitEvent(s, F.ev_ids, 0));
    if (p.ids_taken) F.ids_wait = false;
    // this frame's draw table; the updates since the last frame of this parity go into its planes and sets, s behind the last texture update
    rc = zr_update_frame(c, s, c->fcur);
    if (rc) return rc;
    c->timing_now = c->timing_interval != 0 && c->frame_no % c->timing_interval == 0;     // pass events cost ~6 us of stream bubble each
    if (zr_ctx::TimedFrame* T = c->timed_frame()) T->rule = zr_timed_rule(p);      // what this sample records, and what its figures read
    TIMED(c, EV_BEGIN);
    if (c->view_dirty) { c->view_version++; c->view_dirty = false; }
    if (p.light_args) {
        // One launch: its uniforms travel as arguments.  No ring slot, no upload, no k_frame_begin - and F.view_uploaded stays as it is: the
        // next frame that reads F.view finds it stale and uploads.  The ring's slots paced the host to VIEW_RING frames ahead of the
        // device; without them that bound is kept by hand, on the newest end recorded that far back (zr_frame_end.h: VIEW_RING + every - 1).
        if (const uint64_t pace = zr_end_pace(&c->end, c->frame_no)) HIPCHK(c, hipEventSynchronize(c->ev_end[(pace - 1) % zr_ctx::END_RING]));
        return ZR_OK;
    }
    return zr_frame_uniforms(c, s, p.reset_stats, p.reset_camera_list);
}

int zr_frame_uniforms(zr_ctx* c, hipStream_t s, bool reset_stats, bool reset_camera_list)
{
    FrameCopy& F = c->fc[c->fcur];
    const XkView* src = nullptr;
    uint32_t k = 0;
    if (F.view_uploaded != c->view_version) {        // pinned ring slot: reused only after the kernel that read it last has run
        k = c->view_slot++ % zr_ctx::VIEW_RING;
        HIPCHK(c, hipEventSynchronize(c->view_ev[k]));
        memcpy(&c->h_view_ring[k], &c->view, sizeof(XkView));
        src = &c->h_view_ring[k];
    }
    // zeroes the camera lane's statistics (the sticky overflow latch survives) and - when the camera list is rebuilt - its length; uploads
    // XkView.  The SHADOW list's length lives in the shadow pipeline's block and is reset on that pipeline's own stream (shadow_pass):
    // the previous frame's shadow pipeline may still be walking it while this kernel runs on the camera lane.
    // (a frame that keeps its camera pass keeps that pass's statistics: an upload, or nothing)
    if (reset_stats || src) zr_launch_frame_begin(reset_stats ? c->d_stats : nullptr, src, F.view, reset_camera_list ? 2u : 0u, s);
    if (src) { HIPCHK(c, hipEventRecord(c->view_ev[k], s)); F.view_uploaded = c->view_version; }
    return ZR_OK;
}

// shadow pass (ZE:3239-3393) of this rank's share of the instances, drawn on stream s
static int shadow_draw(zr_ctx* c, hipStream_t s)
{
    const ZrFramePlan& p = c->plan;
    const ZrPass& P = c->pass[0];      // (built by frame_begin)
    c->last_work[0] = P.n_work;
    // The pass draws into the copy that does NOT hold the current map and makes it the current one: from here on shadow_buf() is the map
    // being drawn.  No event guards the flip: everything that reads or writes either copy - this pipeline, the lighting passes and their
    // fused clear, the read-backs and copies - is enqueued on the host's stream, in frame order.
    if (!c->d_shadow_ext) c->smap ^= 1;
    // clear depth 1.0 (ZE:3248): a lighting pass since the copy's last draw already did it for the internal double-buffered map
    FrameCopy& F = c->fc[c->smap];
    if (c->d_shadow_ext || !F.shadow_cleared) zr_launch_fill32((uint32_t*)shadow_buf(c), 0x3F800000u, (size_t)c->SD * c->SD, s);
    F.shadow_cleared = false;
    ZrHiz Z; memset(&Z, 0, sizeof Z);
    if (p.shadow_occlusion) { Z.pxrect = c->d_spxrect; Z.zmin = c->d_szmin; Z.vis_prev = c->d_sflag; Z.vis_stamp = 1u; Z.phase = 1u; }      // (the pass's own flags are 0 / 1)
    // a rebuilt work list starts from length 0 - zeroed HERE, in stream order behind the previous frame's shadow pipeline (k_cull_instances
    // grows it, every later kernel of the pipeline reads it)
    if (p.shadow_list_rebuild) zr_launch_fill32(&c->d_sstats->n_vis_work[0], 0u, 1, s);
    zr_launch_cull_box(P, c->d_objs, c->sc[0].work, c->sc[0].rects, Z, c->d_sstats, 0, s, nullptr, nullptr, p.shadow_list_reuse);
    shadow_bin(c, P, Z, s);
    TIMED(c, EV_SHADOW_BINS);
    raster(c, P, s, p.shadow_occlusion ? 1 : 0);
    if (p.shadow_occlusion) {
        zr_launch_shadow_occlusion(P, c->d_objs, c->sc[0].work, c->sc[0].rects, c->d_spxrect, c->d_szmin, c->d_sflag, (const uint32_t*)shadow_buf(c),
                                   c->sb.bins, c->d_sstats, c->shadow_blocks * 8u, c->carry.sflag_history ? (uint32_t)((c->shadow_draws + c->sflag_turn) & 3u) : 4u, s);      // (a turn per pass DRAWN: kept frames test nothing)
        raster(c, P, s, 2);
    }
    TIMED(c, EV_SHADOW);
    HIPCHK(c, hipGetLastError());
    c->shadow_draws++;
    c->smap_key = P; c->carry = zr_frame_carry(c->carry, c->facts, p, ZR_STAGE_SHADOW);
    return ZR_OK;
}

// The frame's shadow stage: the pass drawn, or kept - the map of the last drawn pass is this frame's, bit for bit: nothing is launched, and
// its statistics block, last_work[0] and the occlusion flags stay as that pass left them.
static int shadow_pass(zr_ctx* c)
{
    const ZrFramePlan& p = c->plan;
    if (p.shadow == ZR_LANE_NONE) TIMED(c, EV_SHADOW_BINS, EV_SHADOW);
    else if (int rc = shadow_draw(c, lane_stream(c, p.shadow))) return rc;
    if (p.ev_join) HIPCHK(c, hipEventRecord(c->ev_join, c->stream));
    return ZR_OK;
}

// deferred-scene pass (ZE:3417-3480): cull + bin + raster + resolve of the owned tiles, on the plan's stream.  Where the plan leaves the
// resolve to zr_render_lighting (deferred_resolve), the lane ends k_mark -> ev_cam -> k_plan.
static int gbuffer_pass(zr_ctx* c)
{
    const ZrFramePlan& p = c->plan;
    if (p.camera == ZR_LANE_NONE) {
        // The camera pass kept whole: both GBuffer copies, the key buffers, the visibility history and its stamp, the plan, the statistics
        // block and cov_block stay as the last drawn frame left them, and nothing is launched.  (Where the lighting's span starts:
        // zr_timed.h - a frame that is one launch records nothing here.)
        TIMED(c, EV_CAMERA, EV_CULL, EV_ROUND1, EV_HIZ, EV_ROUND2, EV_RESOLVE);
        return ZR_OK;
    }
    const hipStream_t s = lane_stream(c, p.camera);
    TIMED(c, EV_CAMERA);
    ZrPass P = c->pass[1];             // (built by frame_begin; the overlay fields are set below)
    c->last_work[1] = P.n_work;
    // Two-pass occlusion culling (ZrFramePlan::rounds).  The depth test decides every pixel either way, so the frame does not depend on
    // the history.
    ZrHiz Z = c->hiz;
    Z.tiles_x = c->tiles_x; Z.tile_rank = c->cfg.tile_rank; Z.tile_world = c->cfg.tile_world;
    Z.pxrect = p.hiz_on ? c->d_pxrect : nullptr; Z.zmin = p.hiz_on ? c->d_zmin : nullptr;
    Z.vis_prev = c->d_visflag[c->vis_cur ^ 1]; Z.vis_now = p.hiz_on ? c->d_visflag[c->vis_cur] : nullptr;
    // visibility marks are frame stamps (1 .. 255): the resolve writes this frame's, the culls compare with last frame's - nothing is cleared
    // (a stamp per pass DRAWN: a rest of any length leaves the stamps as an uninterrupted run of drawn frames would)
    const uint32_t vis_mark = 1u + (uint32_t)(c->cam_draws % 255u);
    Z.vis_stamp = c->vis_mark_prev;
    Z.phase = 0;
    c->last_two_round = p.rounds != ZR_ROUNDS_ONE;
    // (the cull kernel also compacts round 1's list - the survivors that owned a pixel last frame, or all of them)
    zr_launch_cull_box(P, c->d_objs, c->sc[1].work, c->sc[1].rects, Z, c->d_stats, 1, s, c->tb.sel, c->last_two_round ? Z.vis_prev : nullptr, p.camera_list_reuse);
    TIMED(c, EV_CULL);
    if (c->last_two_round) Z.phase = 1;
    // Round 2 kept: round 1 - what owned a pixel of the previous frame - leaves this frame's key buffer, and round 1 is the frame's last
    // round: its k_tile draws the slow triangles.  The statistics and the plan are those of round 2 as last drawn (k_plan).
    tri_raster(c, P, Z, 1, s, p.rounds != ZR_ROUNDS_TWO, p.count_first);
    TIMED(c, EV_ROUND1);
    if (p.rounds == ZR_ROUNDS_TWO) {
        zr_launch_hiz_build(c->d_vis[c->fcur], c->W, c->H, Z, c->d_hiz_regions, c->n_hiz_regions, s);
        Z.phase = 2;
        tri_select(c, P, Z, 2, s);
        TIMED(c, EV_HIZ);
        tri_raster(c, P, Z, 2, s, true, false);
    } else
        TIMED(c, EV_HIZ);
    {   // the overlay plane (skydome pixels) is written only when a skydome is drawn, or once more to wipe one that was
        const bool sky = c->sky_set && c->sky_enabled;
        P.write_overlay = (sky || c->fc[c->fcur].overlay_dirty) ? 1u : 0u;
        c->fc[c->fcur].overlay_dirty = sky;
        P.sky_keys = nullptr; P.sky_object = c->sky_object;
        if (sky && c->d_sky_keys) { zr_launch_sky_tiles(P, c->d_objs, c->d_owned, c->n_owned, c->d_sky_keys, s); P.sky_keys = c->d_sky_keys; }
    }
    TIMED(c, EV_ROUND2);
    if (p.resolve_deferred) {
        // the history now, the planes later: the host's stream waits for everything up to here and resolves from the same keys
        zr_launch_mark(P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], Z.vis_now, s, vis_mark);
        TIMED(c, EV_MARK);
        c->resolve_P = P; c->resolve_mark = vis_mark;
    } else {
        zr_launch_resolve_gbuffer(P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], c->fc[c->fcur].G, c->d_lut, c->d_unorm_lut, Z.vis_now, c->d_stats, s, vis_mark);
        c->cov_block = c->d_stats; c->fc[c->fcur].g_gen = p.g_gen;
        TIMED(c, EV_RESOLVE);
    }
    if (p.ev_cam == ZR_EVCAM_BEHIND_MARK || p.ev_cam == ZR_EVCAM_BEHIND_RESOLVE) HIPCHK(c, hipEventRecord(c->ev_cam, s));
    c->vis_mark_prev = vis_mark; c->cam_draws++;
    // the next frame's buckets, from this frame's counts: nothing of this frame waits for it
    if (P.n_work != 0) zr_launch_plan(c->tb, c->d_owned, c->n_owned, c->d_stats, false, c->bucket_pct, s, p.rounds);
    if (p.hiz_on) c->vis_cur ^= 1;
    HIPCHK(c, hipGetLastError());
    c->cam_prev_key = c->pass[1]; c->carry = zr_frame_carry(c->carry, c->facts, p, ZR_STAGE_CAMERA);
    return ZR_OK;
}

extern "C" int zr_render_gbuffer(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->stage != 1) return zr_fail(c, ZR_ERR_STATE, "zr_render_gbuffer out of order");
        HIPCHK(c, hipSetDevice(c->device));
        const int rc = gbuffer_pass(c);
        if (rc == ZR_OK) c->stage = 2;
        return rc;
    });
}

extern "C" int zr_stream_wait_shadow(zr_ctx* c, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, c->ev_join, 0));
        return ZR_OK;
    });
}

// Both geometry passes of a frame.  Two lanes (zr_frame_plan): the camera pipeline on cam_s; the shadow pipeline on the host's stream,
// where the lighting pass will follow.  The next frame's camera pipeline starts as soon as this one's is through, next to this frame's
// lighting; its shadow pipeline follows the lighting.  The shadow pipeline needs nothing of the head's - its matrices are kernel
// arguments, its statistics a block of its own that it resets itself, work-list length included.  A frame that keeps its shadow map has no
// shadow pipeline: in zr_render its resolve takes that place on the host's stream, next to the next frame's camera pipeline.  Never more
// than two kernels side by side: a third only takes occupancy from the other two (measured).
static int geometry_passes(zr_ctx* c, ZrEntry entry)
{
    const ZrFramePlan& p = c->plan;
    int rc = frame_begin(c, entry);
    if (rc == ZR_OK) rc = shadow_pass(c);
    if (rc == ZR_OK) rc = gbuffer_pass(c);
    if (rc == ZR_OK && p.one_pixel == ZR_LANE_CAM) rc = empty_pixel_pass(c);      // (a kept frame's head on the lane: behind the upload)
    if (rc == ZR_OK && (p.ev_cam == ZR_EVCAM_BEHIND_ONE_PIXEL || p.ev_cam == ZR_EVCAM_LANE_END)) HIPCHK(c, hipEventRecord(c->ev_cam, c->cam_s));
    if (rc == ZR_OK) c->stage = 2;
    return rc;
}

extern "C" int zr_render_shadow(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        int rc = frame_begin(c, ZR_ENTRY_STAGED);
        if (rc == ZR_OK) rc = shadow_pass(c);
        if (rc == ZR_OK) c->stage = 1;
        return rc;
    });
}

extern "C" int zr_render_geometry(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return geometry_passes(c, ZR_ENTRY_GEOMETRY); });
}

// The resolve of a frame whose camera lane left it to the host's stream (gbuffer_pass), behind the wait for ev_cam: same launch, same
// keys; the history is already marked (vis_now = nullptr) and the coverage tally goes to the frame copy's own block, zeroed here.
static int deferred_resolve(zr_ctx* c)
{
    const hipStream_t s = lane_stream(c, c->plan.resolve);
    ZrDevStats* const tally = c->d_rstats[c->fcur];
    zr_launch_fill32(tally->covered_part, 0u, 32, s);
    TIMED(c, EV_HOST_RESOLVE);
    zr_launch_resolve_gbuffer(c->resolve_P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], c->fc[c->fcur].G, c->d_lut, c->d_unorm_lut, nullptr, tally, s, c->resolve_mark);
    TIMED(c, EV_RESOLVE);
    c->cov_block = tally; c->fc[c->fcur].g_gen = c->plan.g_gen;
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}

// The lighting stage behind the geometry passes.  set_device: the staged entry point's call (zr_render's frame_begin has made the device
// current for the whole call: once per zr_render).
static int lighting_stage(zr_ctx* c, bool set_device)
{
    if (c->stage != 2) return zr_fail(c, ZR_ERR_STATE, "zr_render_lighting out of order");
    if (set_device) HIPCHK(c, hipSetDevice(c->device));
    const ZrFramePlan& p = c->plan;
    // The one wait of the host's stream per frame: the camera lane's GBuffer (or, where the resolve follows here, its keys and history
    // marks: ev_cam is then recorded ahead of the lane's k_plan) - and, ahead of it on that lane, this frame's k_frame_begin, whose
    // uniforms the empty-pixel pass below reads (the shadow pipeline before it needed nothing of them and did not wait).
    if (p.host_waits_ev_cam) HIPCHK(c, hipStreamWaitEvent(lane_stream(c, p.lighting), c->ev_cam, 0));
    int rc = p.resolve_deferred ? deferred_resolve(c) : ZR_OK;
    if (rc == ZR_OK && p.one_pixel != ZR_LANE_CAM) rc = empty_pixel_pass(c); // the shadow map (possibly reduced over ranks by the host) is final only now
    if (rc == ZR_OK) rc = lighting_pass(c);
    return rc;
}
extern "C" int zr_render_lighting(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return lighting_stage(c, true); });
}

// RecordCommandBuffer (ZE:3160-3744) + vkQueueSubmit (ZE:2014): shadow -> deferred scene -> deferred lighting, with two
// frames in flight as in the reference (MAX_FRAMES_IN_FLIGHT, ZE:77).
// The shadow pass and the deferred-scene pass do not depend on each other, and the next frame's geometry does not depend on this
// frame's lighting.  zr_render therefore runs two lanes: the camera pipeline on the library's high-priority stream cam_s, and
// shadow pipeline -> lighting on the host's stream.  Whatever the host enqueues on its stream after zr_render is ordered after
// the finished frame, as before.  ZR_FLAG_SERIAL_PASSES keeps everything on the one stream, as the staged entry points do.
// A frame that keeps its shadow map resolves on the host's stream: camera lane ... -> k_tile -> k_mark -> ev_cam -> k_plan, host's stream
// wait -> k_resolve_gbuffer -> one-pixel launch -> k_lighting -> ev_end.
// A frame that keeps its whole camera pass has no camera pipeline: host's stream upload -> [shadow pipeline] -> one-pixel launch ->
// k_lighting -> ev_end, over the GBuffer copy of its parity as the last two drawn frames left both; where it keeps its map too (and has
// kept it for a frame), upload -> one-pixel launch -> ev_cam run on the lane beside the previous frame's k_lighting, and the host's stream waits for ev_cam.
extern "C" int zr_render(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        int rc = geometry_passes(c, ZR_ENTRY_RENDER);
        if (rc == ZR_OK) rc = lighting_stage(c, false);
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
        zr_history_forgotten(c, ZR_HIST_SHADOW_LIST); zr_casters_changed(c);
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

