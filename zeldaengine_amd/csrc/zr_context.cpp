// zr_context.cpp — the context's lifetime behind the C-ABI (zelda_render.h): zr_create / zr_destroy, the last error, the host's stream,
// "everything the library has enqueued" (zr_sync_all) and the tile partition that the context and the multi-GPU hosts share.
//
// Nothing here computes a pixel on the CPU and there is no fallback: without a usable HIP device zr_create fails.
#include "zr_ctx.h"
#include "zr_math.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>

int zr_fail(zr_ctx* c, int code, const std::string& msg)
{
    if (c) { try { c->err = msg; } catch (...) { c->err.clear(); } }      // (called from catch blocks: must not throw itself)
    return code;
}

int zr_stage_idle(zr_ctx* c, const char* what, bool hint)
{
    if (c->stage == 0) return ZR_OK;
    return zr_fail(c, ZR_ERR_STATE, std::string(what) + (hint ? " between the stages of a frame (finish it with zr_render_lighting first)"
                                                              : " between the stages of a frame"));
}

// Everything the library has enqueued: the host's stream (shadow pipeline, lighting) and its own camera lane.
hipError_t zr_sync_all(zr_ctx* c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->cam_s) e = hipStreamSynchronize(c->cam_s);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (the host's stream may have been made to wait for the lanes)
    if (e == hipSuccess) e = zr_dist_sync(c);           // the native multi-GPU host's collective stream, if any
    if (e == hipSuccess) e = zr_update_sync(c);         // the last updates (on callers' streams)
    return e;
}

// ------------------------------------------------------------------------------------------------ lifetime

static void default_lights(XkView* v)
{   // XkLight() default constructor, ZE:779
    XkLight d; memset(&d, 0, sizeof d);
    d.Color[0] = d.Color[1] = d.Color[2] = d.Color[3] = 1.0f; d.Direction[2] = 1.0f; d.Direction[3] = 1.0f;
    for (auto& l : v->DirectionalLights) l = d;
    for (auto& l : v->PointLights) l = d;
    for (auto& l : v->SpotLights) l = d;
}

ZrTilePartition zr_partition(uint32_t tiles_x, uint32_t tiles_y, uint32_t world, uint32_t rank)
{
    ZrTilePartition P;
    P.map.resize((size_t)tiles_x * tiles_y);
    std::vector<uint32_t> counts(world, 0u);
    for (uint32_t t = 0; t < tiles_x * tiles_y; ++t) {
        const uint32_t o = zr_tile_owner(t % tiles_x, t / tiles_x, world);
        P.map[t] = counts[o]++;                          // slot within its owner, for now
        if (o == rank) P.owned.push_back(t);
    }
    for (uint32_t n : counts) P.slots_per_rank = std::max(P.slots_per_rank, n);
    for (uint32_t t = 0; t < tiles_x * tiles_y; ++t) P.map[t] += zr_tile_owner(t % tiles_x, t / tiles_x, world) * P.slots_per_rank;
    return P;
}

// Schedule constants that are re-measured whenever the balance of the two lanes changes ("The schedule"): the camera lane's
// stream priority (0 lowest, 1 normal, 2 highest) and k_tile's persistent grid in workgroups per CU.  (The third, ZR_EV_CAM_AHEAD_OF_PLAN,
// is zr_frame_plan.h's.)
#ifndef ZR_CAM_PRIORITY
#define ZR_CAM_PRIORITY 0
#endif
#ifndef ZR_TILE_WG_PER_CU
#define ZR_TILE_WG_PER_CU 12u
#endif

// zr_create's device half, straight through: it returns at the first failure, and the caller releases the partial context as
// zr_destroy releases any other.  This is the context's half - what no extent sizes: streams, events, the shadow map's two copies, the
// uniforms' copies, the statistics blocks, the look-up tables, the map's tile list, the clear pixel; the extent's half is
// zr_extent_create (zr_resize.cpp), which zr_resize goes through again.
static int create_device_state(zr_ctx* c)
{
    ZrOwn& A = c->own;
    HIPCHK(c, A.stream(&c->own_stream));
    c->stream = c->own_stream;
    for (auto& fr : c->timed) for (auto& e : fr.ev) HIPCHK(c, A.event(&e));
    for (auto& e : c->ev_end) HIPCHK(c, A.event(&e));
    for (FrameCopy& F : c->fc) HIPCHK(c, A.event(&F.ev_ids, hipEventDisableTiming));
    for (FrameCopy& F : c->fc) {        // two frames in flight: see zr_ctx.h
        HIPCHK(c, A.alloc(&F.shadow, (size_t)c->SD * c->SD)); HIPCHK(c, A.alloc(&F.view, 1)); HIPCHK(c, A.alloc(&F.empty_rgba, 1));
    }
    HIPCHK(c, A.alloc(&c->d_stats, 1));
    HIPCHK(c, A.alloc(&c->d_sstats, 1));       // the shadow pipeline's own block (see zr_ctx.h)
    for (auto& r : c->d_rstats) HIPCHK(c, A.alloc(&r, 1));      // ... and a host-lane resolve's, per frame copy
    c->cov_block = c->d_stats;
    HIPCHK(c, A.alloc(&c->d_lut, 256));
    HIPCHK(c, hipMemcpy(c->d_lut, c->lut, sizeof c->lut, hipMemcpyHostToDevice));
    {
        std::vector<float> ul(1280);
        for (int i = 0; i < 256; ++i) {
            ul[(size_t)i] = (float)i / 255.0f;
            if (fmaf((float)i, ZR_UNORM8_HI, (float)i * ZR_UNORM8_LO) != ul[(size_t)i])        // the packed sampler's division-free decode
                return zr_fail(c, ZR_ERR_DEVICE, "ZR_UNORM8_HI / ZR_UNORM8_LO do not decode c / 255 exactly");
        }
        for (int i = 0; i < 1024; ++i) ul[256 + (size_t)i] = (float)i / 1023.0f;
        HIPCHK(c, A.alloc(&c->d_unorm_lut, ul.size()));
        HIPCHK(c, hipMemcpy(c->d_unorm_lut, ul.data(), ul.size() * 4, hipMemcpyHostToDevice));
    }

    // the shadow map is rendered whole on every rank (the screen's tiles: zr_extent_create)
    c->stiles_x = (c->SD + ZR_TILE - 1) / ZR_TILE; c->stiles_y = c->stiles_x; c->sn_tiles = c->stiles_x * c->stiles_y;
    if (c->sn_tiles > 16000u) return zr_fail(c, ZR_ERR_ARG, "too many tiles");   // binning histograms (4 B per tile, dynamic) + a few static words must fit the default 64 KB of LDS per workgroup
    std::vector<uint32_t> sowned(c->sn_tiles);
    for (uint32_t t = 0; t < c->sn_tiles; ++t) sowned[t] = t;
    HIPCHK(c, upload(A, &c->d_sowned, sowned));
    {   // the clear values of ZE:3427-3433, as resolve_pixel writes them for an empty pixel
        HIPCHK(c, A.alloc(&c->d_clear_px, 64));
        uint32_t px[16] = { 0 };
        px[0] = 0x3F800000u;                    // depth 1.0
        px[1] = 0xFF000000u; px[2] = 0u; px[3] = 0xFF000000u; px[4] = 0xFF000000u;   // SceneColor, A, B, C
        px[6] = 0u; px[7] = 0x3C000000u;        // D = (0, 0, 0, 1) as fp16
        px[8] = 0u;                             // overlay
        HIPCHK(c, hipMemcpy(c->d_clear_px, px, sizeof px, hipMemcpyHostToDevice));
        uint32_t* w = (uint32_t*)c->d_clear_px;
        c->Gclear.depth = (float*)w; c->Gclear.scene_color = w + 1; c->Gclear.gA = w + 2; c->Gclear.gB = w + 3; c->Gclear.gC = w + 4;
        c->Gclear.gD = (uint2*)(w + 6); c->Gclear.overlay = w + 8;
    }
    {   // environment switches, read once
#ifdef ZR_DIAG       // work-skipping / printing switches: diagnostic builds only (zeldaengine_amd.build.build(extra_flags=["-DZR_DIAG"]))
        const char* e;
        if ((e = getenv("ZR_DEBUG_SKIP"))) c->env_skip = (uint32_t)atoi(e);                 // 1: no pixel walk, 2: no triangle phase
        if ((e = getenv("ZR_DEBUG_SKIP_LIGHT"))) c->env_skip_light = (uint32_t)atoi(e);     // bits: 1 PCF, 2 lights, 4 reflection
        if ((e = getenv("ZR_LIGHT_LIST_MIN"))) c->env_light_list_min = atoi(e);
        c->env_no_empty_px = getenv("ZR_NO_EMPTY_PIXEL") != nullptr;
#endif
        // every build: the resting frame through k_lighting_rest, every pixel written (the control of k_lighting_stand's A/B, and its test's)
        c->lk.settle_off = getenv("ZR_NO_REST_SETTLE") != nullptr;
        c->lk.lead_off = getenv("ZR_NO_LEAD_WAVE") != nullptr;
        // ... and how often a frame inside a run of one-launch frames records its end (zr_frame_end.h; 1: every frame, as all others do)
        c->end.every = ZR_REST_END_EVERY_DEFAULT;
        if (const char* r = getenv("ZR_REST_END_EVERY")) { const int v = atoi(r); c->end.every = v < 1 ? 1u : (uint32_t)v > kZrEndEveryMax ? kZrEndEveryMax : (uint32_t)v; }
    }
    HIPCHK(c, A.host(&c->h_view_ring, zr_ctx::VIEW_RING));
    for (auto& e : c->view_ev) HIPCHK(c, A.event(&e, hipEventDisableTiming));
    {   // The camera lane must not share a hardware queue with the host's stream (HIP multiplexes streams onto a few of them and
        // two streams on one queue run strictly one after the other).  Streams of different priority come from different queue
        // pools.  Which priority: the frame's period is the HOST's lane (lighting -> shadow pipeline), and since the camera lane lost its
        // two scans and two index passes per frame (round 6: tile buckets) it no longer fills the period - at the highest priority it
        // took from the host lane what it saved itself (5 300 Mpixel/s), at the lowest the host lane keeps its share (5 540; normal: 5 470).
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        HIPCHK(c, A.stream(&c->cam_s, ZR_CAM_PRIORITY == 2 ? greatest : ZR_CAM_PRIORITY == 1 ? (least + greatest) / 2 : least));
    }
    HIPCHK(c, A.event(&c->ev_cam, hipEventDisableTiming)); HIPCHK(c, A.event(&c->ev_join, hipEventDisableTiming));
    HIPCHK(c, A.event(&c->ev_lane, hipEventDisableTiming));
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->raster_blocks = (uint32_t)prop.multiProcessorCount * ZR_TILE_WG_PER_CU; }      // k_tile's persistent grid (6 workgroups fit a CU: two rounds of them; A/B 4 / 6 / 8 / 12 / 16 / 32 per CU -> 5 133 / 5 250 / 5 294 / 5 344 / 5 327 / 5 277 Mpixel/s)
    c->shadow_blocks = c->raster_blocks / ZR_TILE_WG_PER_CU * 8u;      // the shadow rasteriser's persistent grid stays at 8 per CU
    c->slow0_cap = std::max<uint32_t>(c->slow0_cap, 128u * c->sn_tiles);      // (a clipped triangle is listed once per tile of its meshlet)
    HIPCHK(c, A.alloc(&c->d_slow0, 4ull * c->slow0_cap));
#ifdef ZR_DIAG
    if (const char* e = getenv("ZR_RASTER_BLOCKS")) c->raster_blocks = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("ZR_SHADOW_BLOCKS")) c->shadow_blocks = (uint32_t)std::max(1, atoi(e));
#endif
    HIPCHK(c, zr_fill_sync({ { c->d_stats, 0, sizeof(ZrDevStats) }, { c->d_sstats, 0, sizeof(ZrDevStats) },
                             { c->d_rstats[0], 0, sizeof(ZrDevStats) }, { c->d_rstats[1], 0, sizeof(ZrDevStats) } }));
    if (int rc = zr_extent_create(c)) return rc;      // everything the extent sizes
    // The runtime backs an event with a signal on its FIRST record and grows that pool in batches, which blocks the host for
    // milliseconds at unpredictable frames of a short run: record every event once now.
    for (auto& fr : c->timed) for (auto& e : fr.ev) HIPCHK(c, hipEventRecord(e, c->stream));
    for (auto& e : c->ev_end) HIPCHK(c, hipEventRecord(e, c->stream));
    for (auto& e : c->view_ev) HIPCHK(c, hipEventRecord(e, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZR_OK;
}

extern "C" int zr_create(const zr_config* cfg, zr_ctx** out)
{
    if (!cfg || !out) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        *out = nullptr;
        if (cfg->width == 0 || cfg->height == 0 || cfg->width > 255u * ZR_TILE || cfg->height > 255u * ZR_TILE) return ZR_ERR_ARG;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZR_ERR_DEVICE;
        if (cfg->device < 0 || cfg->device >= ndev) return ZR_ERR_DEVICE;
        if (hipSetDevice(cfg->device) != hipSuccess) return ZR_ERR_DEVICE;
        zr_ctx* c = new zr_ctx();
        c->cfg = *cfg;
        if (c->cfg.tile_world == 0) c->cfg.tile_world = 1;
        if (c->cfg.tile_rank >= c->cfg.tile_world) { delete c; return ZR_ERR_ARG; }
        c->device = cfg->device;
        c->W = cfg->width; c->H = cfg->height; c->SD = cfg->shadow_dim ? cfg->shadow_dim : XK_SHADOWMAP_DIM;
        if (c->SD > 255u * ZR_TILE) { delete c; return ZR_ERR_ARG; }
        if (c->cfg.flags & ZR_FLAG_MESHLET_BINS) { delete c; return ZR_ERR_UNSUPPORTED; }      // a reserved bit (refused before anything is allocated)
        c->debug_view = cfg->debug_view;
        memset(&c->cam, 0, sizeof c->cam); memset(&c->shadow, 0, sizeof c->shadow); memset(&c->view, 0, sizeof c->view);
        default_lights(&c->view);
        for (int i = 0; i < 256; ++i) c->lut[i] = zr_srgb_decode8((uint32_t)i);
        int rc = zr_guard(c, [&]() { return create_device_state(c); });      // (a guard of its own: what it throws must not skip zr_destroy)
        if (rc == ZR_OK && zr_set_cubemap(c, nullptr, 0) != ZR_OK) rc = ZR_ERR_DEVICE;
        if (rc != ZR_OK) { zr_destroy(c); return rc; }
        *out = c;
        return ZR_OK;
    });
}

extern "C" void zr_destroy(zr_ctx* c)
{
    if (!c) return;
    try {
        zr_livelink_stop(c);
        (void)hipSetDevice(c->device);
        (void)zr_sync_all(c);                  // including a geometry stage whose lighting pass never came
        zr_dist_destroy(c);
        delete c;                              // every owner releases what it made; the context's own (streams last) after the others
    } catch (...) {}
}

extern "C" const char* zr_last_error(const zr_ctx* c) { return c ? c->err.c_str() : "no context (no usable HIP device?)"; }

extern "C" int zr_tile_size(void) { return ZR_TILE; }

extern "C" uint32_t zr_tile_owner(uint32_t tx, uint32_t ty, uint32_t world)
{
    return world <= 1 ? 0u : ((tx >> ZR_SUPERTILE_SHIFT) + (ty >> ZR_SUPERTILE_SHIFT) * ZR_SUPERTILE_SKEW) % world;
}

extern "C" int zr_tile_partition(uint32_t width, uint32_t height, uint32_t world, uint32_t rank, uint32_t* owned, uint32_t* n_owned, uint32_t* slots_per_rank)
{
    if (!width || !height || !world || rank >= world || !n_owned || !slots_per_rank) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        const ZrTilePartition P = zr_partition((width + ZR_TILE - 1) / ZR_TILE, (height + ZR_TILE - 1) / ZR_TILE, world, rank);
        if (owned) std::copy(P.owned.begin(), P.owned.end(), owned);
        *n_owned = (uint32_t)P.owned.size(); *slots_per_rank = P.slots_per_rank;
        return ZR_OK;
    });
}

extern "C" int zr_set_stream(zr_ctx* c, void* s)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        hipStream_t ns = s ? (hipStream_t)s : c->own_stream;
        // frames in flight are ordered by their place on the host's stream (frame_begin relies on it): a change of stream drains them
        if (ns != c->stream && c->rendered) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, zr_sync_all(c)); }
        if (ns != c->stream) { zr_casters_changed(c); zr_history_forgotten(c, ZR_HIST_LIGHT_PLANE); }      // (the kept map's two copies, and the lighting pass's plane, are ordered by their place on the host's stream too)
        c->stream = ns;
        return ZR_OK;
    });
}

extern "C" uint32_t zr_abi_version(void) { return ZR_ABI_VERSION; }
