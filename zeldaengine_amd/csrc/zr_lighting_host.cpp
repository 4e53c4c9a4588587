// zr_lighting_host.cpp — the lighting stage of a frame (zr_frame_host.cpp has the stages before it): the pass's uniforms, the one-pixel
// launch, the pass itself, and the plane of standing terms a resting frame's pass reads instead of computing them (zr_frame_plan.h decides:
// ZrFramePlan::light_keep / light_fill; DESIGN.md section 5, "The schedule").
#include "zr_ctx.h"
#include "zr_math.h"

#include <cstring>

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

// Whether the frame's lighting pass takes the empty-pixel shortcut (empty_pixel_pass below).
static bool empty_px_on(const zr_ctx* c) { return c->shading != ZR_SHADING_FORWARD && c->debug_view != 6u && !c->env_no_empty_px; }

// The standing uniforms: everything shade_standing (zr_shade.h) reads that is neither the pixel's GBuffer values, the shadow map nor the
// cubemap's texels - L.SB, SD, the camera position, LightsCount[0] and [3], the directional light records in use, the cubemap's shape,
// debug_skip.  Unused records are zero, so that two keys compare byte for byte.
static void light_key(const zr_ctx* c, zr_ctx::LightKey* K)
{
    ZrLightParams L; light_params(c, &L);
    memset(K, 0, sizeof *K);
    memcpy(K->SB, L.SB, sizeof K->SB); memcpy(K->cam, c->view.CameraInfo, sizeof K->cam);
    K->SD = L.SD; K->max_mips = (uint32_t)c->view.LightsCount[3]; K->cube_dim = L.cube_dim; K->cube_levels = L.cube_levels; K->debug_skip = L.debug_skip;
    const int32_t nd = c->view.LightsCount[0];
    K->n_dir = (uint32_t)nd;
    for (int32_t i = 0; i < nd && i < XK_MAX_DIRECTIONAL_LIGHTS_NUM; ++i) K->dir[i] = c->view.DirectionalLights[i];
}

// Whether the point lights fit the one launch (k_lighting_rest): they travel in its argument, its records exist, and the view is not the
// one k_gbuffer_vis finishes from XkView.
static bool rest_launch_fits(const zr_ctx* c)
{
    const int32_t np = c->view.LightsCount[1];
    return np >= 0 && np <= ZR_REST_ARG_LIGHTS && c->lk.rest != nullptr && c->debug_view != 9u;
}

void zr_light_facts(zr_ctx* c, ZrFrameFacts* f)
{
    light_key(c, &c->lk.now);
    f->light_plane_ok = !c->lk.alloc_failed;
    f->light_uniforms_same = c->lk.plane != nullptr && memcmp(&c->lk.now, &c->lk.key, sizeof c->lk.key) == 0;
    f->cube_gen = c->cube_gen;
    f->light_empty_px = empty_px_on(c);
    // (the slot is made with the plane, by the first frame planned to fill: a context that has neither yet counts as one that gets it)
    f->light_slot = zr_lighting_rest_available() && (c->lk.rest != nullptr || (c->lk.plane == nullptr && !c->lk.alloc_failed));
    f->light_by_arg = zr_lighting_rest_available() && f->light_empty_px && rest_launch_fits(c);
}

// The plane is made when the first frame is planned to fill it: 32 B x W x H (66 MB at 1080p, 265 MB at 2160p), through the extent's
// owner (zr_ctx::ext: a resize releases it, and the first resting frame at the new extent makes its successor).  No room: the context simply never keeps - that is no error.  With it, in an allocation of their own, the slot and the records
// of the one-launch resting frame (ZrRestRecord: 512 B per owned tile); no room for those: the context keeps as a context without them.
bool zr_light_plane_make(zr_ctx* c)
{
    if (c->lk.plane) return true;
    if (!c->lk.alloc_failed && c->ext.alloc(&c->lk.plane, 2 * (size_t)c->W * c->H) != hipSuccess) {
        (void)hipGetLastError();      // (the refusal is not the frame's error)
        c->lk.plane = nullptr; c->lk.alloc_failed = true;
    }
    if (c->lk.plane && !c->lk.rest && zr_lighting_rest_available() &&
        c->ext.alloc(&c->lk.rest, ZR_REST_SLOT + (size_t)c->n_owned * ZR_REST_RECORDS_PER_TILE * (sizeof(ZrRestRecord) / sizeof(float4))) != hipSuccess) {
        (void)hipGetLastError();
        c->lk.rest = nullptr;
    }
    // ... and, with those, the marks of the parts a resting frame leaves as they stand (k_lighting_stand), zero-filled on the stream every
    // lighting pass runs on; no room: the context rests through k_lighting_rest
    if (c->lk.rest && !c->lk.marks && !c->lk.settle_off) {
        const size_t n = (size_t)c->n_owned * zr_lighting_stand_parts();
        if (c->ext.alloc(&c->lk.marks, n) != hipSuccess || hipMemsetAsync(c->lk.marks, 0, (n ? n : 1) * sizeof(uint32_t), c->stream) != hipSuccess) {
            (void)hipGetLastError();
            c->lk.marks = nullptr;
        }
        zr_settle_forget(&c->lk.settle);
    }
    return c->lk.plane != nullptr;
}

// The lighting shader's colour for a pixel that still holds every target's clear value: one launch of the lighting kernel over a
// one-pixel GBuffer.  It needs the finished shadow map (PCF at world position 0) and the frame's uniforms, nothing else.  View 6
// (the quad's interpolated vertex colour) depends on the pixel position, so it goes without.  It never reads the plane.  In a frame that
// fills the plane it fills too, the same kernel over a plane of its own: the slot (zr_ctx::LightKeep::rest, W = H = 1: rest[0], rest[1])
// then holds the cleared pixel's standing terms, which the one-launch resting frames shade it from - whether or not this frame's shortcut
// is on (a fill in debug view 6 serves the views after it).
int empty_pixel_pass(zr_ctx* c)
{
    c->empty_ready = false;
    const bool fill_slot = c->plan.light_fill && c->lk.rest != nullptr;
    if (c->plan.one_pixel == ZR_LANE_NONE || (!empty_px_on(c) && !fill_slot)) return ZR_OK;
    ZrLightParams L; light_params(c, &L);
    L.W = 1; L.H = 1; L.tiles_x = 1; L.packed_out = 0; L.bg_enabled = 0;
    zr_launch_lighting(L, c->fc[c->fcur].view, c->d_sowned, 1, c->Gclear, shadow_buf(c), c->cube, c->d_lut, c->d_unorm_lut, c->fc[c->fcur].empty_rgba,
                       lane_stream(c, c->plan.one_pixel), fill_slot ? ZR_LIGHT_FILL : ZR_LIGHT_PLAIN, fill_slot ? c->lk.rest : nullptr);
    HIPCHK(c, hipGetLastError());
    c->empty_ready = empty_px_on(c);
    return ZR_OK;
}

// What k_lighting_rest takes instead of XkView (ZrRestArgs).
static void rest_args(const zr_ctx* c, ZrRestArgs* R)
{
    const XkView& V = c->view;
    memset(R, 0, sizeof *R);
    memcpy(R->cam, V.CameraInfo, sizeof R->cam);
    R->nDir = (uint32_t)V.LightsCount[0]; R->nPoint = (uint32_t)V.LightsCount[1];
    for (uint32_t i = 0; i < R->nPoint && i < ZR_REST_ARG_LIGHTS; ++i) {
        memcpy(R->pt[i].color, V.PointLights[i].Color, sizeof R->pt[i].color);
        memcpy(R->pt[i].pos_falloff, V.PointLights[i].Position, 3 * sizeof(float));
        R->pt[i].pos_falloff[3] = V.PointLights[i].Direction[3];
    }
}

// Whether the library can vouch for every writer of the resting frame's target (zr_settle.h): its own buffer (a caller-owned tiles buffer
// alternates, and the native multi-GPU host's with it), one rank (a rank of several hands its tiles to a collective: out of scope), its
// address never handed to a caller who may write through it, the marks made, and ZR_NO_REST_SETTLE not set.
static bool settle_allowed(const zr_ctx* c)
{
    return c->lk.marks != nullptr && !c->lk.settle_off && !c->lk.handed_out && c->d_tiles_ext == nullptr && c->dist == nullptr && c->cfg.tile_world <= 1u;
}
// The byte image of what a settled part's colour, and where it lies, depend on - everything the launch reads but the point lights and the
// GBuffer pointers (resting frames alternate between the two copies, which camera_keep guarantees equal) - and the next map's clear.
static void settle_key(const zr_ctx* c, const ZrLightParams& L, const ZrRestArgs& R, const uint32_t* out, zr_ctx::SettleKey* K)
{
    memset(K, 0, sizeof *K);
    K->L = L; K->L.clear_next = nullptr; K->L.clear_n = 0;
    memcpy(K->cam, R.cam, sizeof K->cam); K->nDir = R.nDir; K->n_owned = c->n_owned;
    K->out = out; K->plane = c->lk.plane; K->rest = c->lk.rest; K->owned = c->d_owned; K->marks = c->lk.marks;
}

int lighting_pass(zr_ctx* c)
{
    const ZrFramePlan& p = c->plan;
    const hipStream_t s = lane_stream(c, p.lighting);
    ZrLightParams L; light_params(c, &L);
    const FrameCopy& F = c->fc[c->fcur];
    L.empty_rgba = c->empty_ready ? F.empty_rgba : nullptr;
    // The next DRAWN shadow pass follows on this stream and rasterises into the OTHER copy of the map, which nothing reads or
    // writes while this pass runs: clear it here - once; a run of frames that keep their map finds it clear and writes nothing.
    FrameCopy& next = c->fc[c->smap ^ 1];
    if (c->n_owned && !c->d_shadow_ext && !next.shadow_cleared) { L.clear_next = (uint32_t*)next.shadow; L.clear_n = c->SD * c->SD; next.shadow_cleared = true; }
    uint32_t* const frame_out = L.packed_out ? (c->d_tiles_ext ? c->d_tiles_ext : c->d_tiles) : c->d_color;
    // What the plan decided about the plane holds unless the debug view or the cubemap changed between the stages of the frame (the
    // staged entry points: neither call is refused there): then this pass ignores the plane, and the next resting frame fills it.
    // A frame planned as one launch (light_args) had no one-pixel launch and uploaded nothing: when it is demoted, or the view now is 9
    // (k_gbuffer_vis reads XkView), it shades every pixel itself and gets its uniforms here, on this stream.
    ZrLightMode mode = p.light_keep ? ZR_LIGHT_KEPT : p.light_fill ? ZR_LIGHT_FILL : ZR_LIGHT_PLAIN;
    const bool shortcut_as_planned = p.light_args ? empty_px_on(c) : c->facts.light_empty_px == c->empty_ready;
    bool by_arg = p.light_args && rest_launch_fits(c);
    if (mode != ZR_LIGHT_PLAIN && (c->facts.cube_gen != c->cube_gen || !shortcut_as_planned || !c->lk.plane || c->shading == ZR_SHADING_FORWARD || (p.light_args && !by_arg))) {
        mode = ZR_LIGHT_PLAIN; by_arg = false; zr_history_forgotten(c, ZR_HIST_LIGHT_PLANE);
    }
    if (p.light_args && !by_arg) { if (int rc = zr_frame_uniforms(c, s, false, false)) return rc; }
    bool stood = false;      // the pass is a k_lighting_stand launch: every other pass writes the target behind that kernel's back
    if (c->shading == ZR_SHADING_FORWARD) {
        // Base.frag over the winners the resolve recorded, with this frame's camera block (frame_begin built it; the overlay fields play no part)
        if (L.clear_next) { zr_launch_fill32(L.clear_next, 0x3F800000u, L.clear_n, s); L.clear_next = nullptr; }
        zr_launch_forward(c->pass[1], L, F.view, c->d_objs, c->d_owned, c->n_owned, F.G, shadow_buf(c), c->cube, c->d_lut, c->d_unorm_lut, frame_out, s);
    } else if (by_arg) {
        ZrRestArgs R; rest_args(c, &R);
        // (the same frame and the same marks either way: k_lighting_lead decides a part once, k_lighting_stand in each of its waves)
        const ZrRestLaunch which = !settle_allowed(c) ? ZR_REST_EVERY_PIXEL : c->lk.lead_off ? ZR_REST_STAND : ZR_REST_LEAD;
        uint32_t gen = 0u;
        if (which != ZR_REST_EVERY_PIXEL) {
            zr_ctx::SettleKey K; settle_key(c, L, R, frame_out, &K);
            ZrSettleFacts sf; sf.stand = true; sf.key_same = memcmp(&K, &c->lk.settle_key, sizeof K) == 0;
            const ZrSettleStep step = zr_settle_step(c->lk.settle, sf);
            if (step.wipe) HIPCHK(c, hipMemsetAsync(c->lk.marks, 0, (size_t)c->n_owned * zr_lighting_stand_parts() * sizeof(uint32_t), s));
            gen = step.gen; c->lk.settle = step.next; c->lk.settle_key = K; stood = true;
        }
        zr_launch_lighting_rest(L, R, c->d_owned, c->n_owned, F.G, c->d_lut, c->d_unorm_lut, frame_out, s, c->lk.plane, c->lk.rest, which, c->lk.marks, gen);
        c->lk.by_arg++;
    } else {
        zr_launch_lighting(L, F.view, c->d_owned, c->n_owned, F.G, shadow_buf(c), c->cube, c->d_lut, c->d_unorm_lut, frame_out, s, mode, c->lk.plane, c->lk.rest);
        if (c->debug_view == 9u)        // GBufferVis mosaic over the lit frame (needs the whole GBuffer: single-rank contexts only)
            zr_launch_gbuffer_vis(L, F.view, F.G, shadow_buf(c), c->cube, c->d_lut, c->d_color, s);
    }
    if (!stood) c->lk.settle = zr_settle_step(c->lk.settle, ZrSettleFacts{}).next;
    TIMED(c, EV_LIGHTING);
    // This frame's GBuffer / shadow map / uniforms copies are free again.  Inside a run of one-launch frames only every few frames say so:
    // whoever asks for another's end is handed a later one (zr_frame_end.h).
    const bool end_recorded = zr_end_records(c->end, c->frame_no, p.light_args);
    if (end_recorded) HIPCHK(c, hipEventRecord(c->ev_end[c->frame_no % zr_ctx::END_RING], s));
    zr_end_enqueued(&c->end, c->frame_no, p.light_args, end_recorded);
    HIPCHK(c, hipGetLastError());
    if (mode == ZR_LIGHT_FILL) { c->lk.key = c->lk.now; c->carry = zr_frame_carry(c->carry, c->facts, p, ZR_STAGE_LIGHTING); }
    c->lk.last = (uint32_t)mode; c->lk.count[mode]++;
    if (c->timing_now) c->sample_no++;
    c->rendered = true; c->frame_no++; c->stage = 0;
    c->ids_frame = c->ids_this; c->ids.gen = c->scene_gen;
    return ZR_OK;
}

static_assert(ZR_LIGHT_PLANE_IGNORED == (uint32_t)ZR_LIGHT_PLAIN && ZR_LIGHT_PLANE_FILLED == (uint32_t)ZR_LIGHT_FILL && ZR_LIGHT_PLANE_READ == (uint32_t)ZR_LIGHT_KEPT,
              "zelda_render.h: what a lighting pass did with the plane");

extern "C" int zr_get_light_keep(zr_ctx* c, zr_light_keep* out, size_t bytes)
{
    if (!c || !out) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        zr_light_keep k;
        memset(&k, 0, sizeof k);
        k.last = c->rendered ? c->lk.last : ZR_LIGHT_PLANE_IGNORED;
        k.ignored = c->lk.count[ZR_LIGHT_PLAIN]; k.filled = c->lk.count[ZR_LIGHT_FILL]; k.read = c->lk.count[ZR_LIGHT_KEPT];
        k.plane_bytes = c->lk.plane ? 32ull * c->W * c->H : 0ull;
        k.read_by_arg = c->lk.by_arg;
        memcpy(out, &k, bytes < sizeof k ? bytes : sizeof k);
        return ZR_OK;
    });
}

// The marks of the frame enqueued last, read back (waits for that frame): out[part] = 1 where the part stands settled - its mark is the
// current generation.  Nothing stands unless that frame was a stand launch.  For tests and tools: nothing is counted per frame.
static int settled_parts(zr_ctx* c, std::vector<uint8_t>* out)
{
    out->assign((size_t)c->n_owned * zr_lighting_stand_parts(), 0);
    if (!c->lk.marks || !c->lk.settle.standing || c->lk.settle.gen == 0u || out->empty()) return ZR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = zr_finish(c);
    if (rc) return rc;
    std::vector<uint32_t> m(out->size());
    HIPCHK(c, hipMemcpy(m.data(), c->lk.marks, m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < m.size(); ++k) (*out)[k] = m[k] == c->lk.settle.gen ? 1 : 0;
    return ZR_OK;
}
extern "C" int zr_get_rest_settled(zr_ctx* c, uint32_t* parts, uint32_t* settled)
{
    if (!c || !parts || !settled) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        std::vector<uint8_t> st;
        int rc = settled_parts(c, &st);
        if (rc) return rc;
        *parts = (uint32_t)st.size(); *settled = 0;
        for (uint8_t v : st) *settled += v;
        return ZR_OK;
    });
}
// ... and which: a byte per part (owned tile slot * 2 + half), `bytes` of them = zr_get_rest_settled's parts
extern "C" int zr_get_rest_settled_parts(zr_ctx* c, uint8_t* standing, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (standing || bytes == 0) && bytes == (size_t)c->n_owned * zr_lighting_stand_parts());
        std::vector<uint8_t> st;
        int rc = settled_parts(c, &st);
        if (rc) return rc;
        if (bytes) memcpy(standing, st.data(), bytes);
        return ZR_OK;
    });
}
