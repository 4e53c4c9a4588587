// zr_host.cpp — context, scene upload, per-frame uniforms and the frame graph behind the C-ABI (zelda_render.h).
//
// Host counterpart of XkZeldaEngineApp's CreateEngineScene / UpdateUniformBuffer / RecordCommandBuffer / DrawFrame
// (ZE:4140, 4585, 3160, 1940).  GPU work is enqueued on two HIP streams (the host's render stream and the library's camera
// lane, see geometry_passes); nothing here computes a pixel on the CPU and there is no fallback: without a usable HIP device
// zr_create fails.
#include "zr_ctx.h"
#include "zr_math.h"
#include "zr_srgb.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <cstdlib>

int zr_fail(zr_ctx* c, int code, const std::string& msg)
{
    if (c) { try { c->err = msg; } catch (...) { c->err.clear(); } }      // (called from catch blocks: must not throw itself)
    return code;
}

// Everything the library has enqueued: the host's stream (shadow pipeline, lighting) and its own camera lane.
hipError_t zr_sync_all(zr_ctx* c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->cam_s) e = hipStreamSynchronize(c->cam_s);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (the host's stream may have been made to wait for the lanes)
    if (e == hipSuccess) e = zr_dist_sync(c);           // the native multi-GPU host's collective stream, if any
    if (e == hipSuccess && c->ev_scatter) e = hipEventSynchronize(c->ev_scatter);      // the last instance update (on a caller's stream)
    if (e == hipSuccess && c->ev_tex) e = hipEventSynchronize(c->ev_tex);              // the last texture update (likewise)
    return e;
}

static const uint8_t kDefaultTexel[7][4] = {    // ZE:4951-4978: default_{grey,black,white,normal,white,black,white}.png
    {127,127,127,255}, {0,0,0,255}, {255,255,255,255}, {127,127,255,255}, {255,255,255,255}, {0,0,0,255}, {255,255,255,255}
};

float zr_srgb_decode8(uint32_t c)
{
    double x = (double)c / 255.0;
    double l = (x <= 0.04045) ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
    return (float)l;
}
// srgb_encode8: zr_srgb.h (the texture updates build their threshold table from the same function)

// ------------------------------------------------------------------------------------------------ lifetime

static void default_lights(XkView* v)
{   // XkLight() default constructor, ZE:779
    XkLight d; memset(&d, 0, sizeof d);
    d.Color[0] = d.Color[1] = d.Color[2] = d.Color[3] = 1.0f; d.Direction[2] = 1.0f; d.Direction[3] = 1.0f;
    for (auto& l : v->DirectionalLights) l = d;
    for (auto& l : v->PointLights) l = d;
    for (auto& l : v->SpotLights) l = d;
}

template <typename T> static hipError_t upload(ZrOwn& own, T** d, const std::vector<T>& h)
{
    hipError_t e = own.alloc(d, h.size());
    if (e != hipSuccess) return e;
    return h.empty() ? hipSuccess : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Tile ownership (zr_tile_owner) of a grid of tiles among `world` ranks: the tiles `rank` owns, in increasing index = its slots in the
// packed buffer; map: tile -> owner * slots_per_rank + slot (k_untile); slots_per_rank: the most tiles any rank owns.
struct ZrTilePartition { std::vector<uint32_t> owned, map; uint32_t slots_per_rank = 0; };
static ZrTilePartition zr_partition(uint32_t tiles_x, uint32_t tiles_y, uint32_t world, uint32_t rank)
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
// stream priority (0 lowest, 1 normal, 2 highest), k_tile's persistent grid in workgroups per CU, and whether a frame that draws its
// shadow map records ev_cam ahead of its k_plan too (a frame that resolves on the host's stream always does).
#ifndef ZR_CAM_PRIORITY
#define ZR_CAM_PRIORITY 0
#endif
#ifndef ZR_TILE_WG_PER_CU
#define ZR_TILE_WG_PER_CU 12u
#endif
#ifndef ZR_EV_CAM_AHEAD_OF_PLAN
#define ZR_EV_CAM_AHEAD_OF_PLAN 0
#endif

// zr_create's device half, straight through: it returns at the first failure, and the caller releases the partial context as
// zr_destroy releases any other
static int create_device_state(zr_ctx* c)
{
    ZrOwn& A = c->own;
    HIPCHK(c, A.stream(&c->own_stream));
    c->stream = c->own_stream;
    for (auto& fr : c->evr) for (auto& e : fr) HIPCHK(c, A.event(&e));
    for (auto& e : c->ev_end) HIPCHK(c, A.event(&e));
    for (FrameCopy& F : c->fc) HIPCHK(c, A.event(&F.ev_ids, hipEventDisableTiming));
    const size_t n = (size_t)c->W * c->H;
    for (FrameCopy& F : c->fc) {        // two frames in flight: see zr_ctx.h
        GBufferPtrs& G = F.G;
        HIPCHK(c, A.alloc(&G.depth, n)); HIPCHK(c, A.alloc(&G.scene_color, n)); HIPCHK(c, A.alloc(&G.gA, n)); HIPCHK(c, A.alloc(&G.gB, n));
        HIPCHK(c, A.alloc(&G.gC, n)); HIPCHK(c, A.alloc(&G.gD, n)); HIPCHK(c, A.alloc(&G.overlay, n));
        HIPCHK(c, A.alloc(&F.shadow, (size_t)c->SD * c->SD)); HIPCHK(c, A.alloc(&F.view, 1)); HIPCHK(c, A.alloc(&F.empty_rgba, 1));
    }
    HIPCHK(c, A.alloc(&c->d_color, n)); HIPCHK(c, A.alloc(&c->d_stats, 1));
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

    // screen tiles: camera target partitioned t % world == rank; the shadow map is rendered whole on every rank
    c->tiles_x = (c->W + ZR_TILE - 1) / ZR_TILE; c->tiles_y = (c->H + ZR_TILE - 1) / ZR_TILE; c->n_tiles = c->tiles_x * c->tiles_y;
    c->stiles_x = (c->SD + ZR_TILE - 1) / ZR_TILE; c->stiles_y = c->stiles_x; c->sn_tiles = c->stiles_x * c->stiles_y;
    if (c->n_tiles > 16000u || c->sn_tiles > 16000u) return zr_fail(c, ZR_ERR_ARG, "too many tiles");   // binning histograms (4 B per tile, dynamic) + a few static words must fit the default 64 KB of LDS per workgroup
    const ZrTilePartition tp = zr_partition(c->tiles_x, c->tiles_y, c->cfg.tile_world, c->cfg.tile_rank);
    std::vector<uint32_t> sowned(c->sn_tiles);
    for (uint32_t t = 0; t < c->sn_tiles; ++t) sowned[t] = t;
    c->slots_per_rank = tp.slots_per_rank; c->n_owned = (uint32_t)tp.owned.size();
    HIPCHK(c, upload(A, &c->d_tile_map, tp.map)); HIPCHK(c, upload(A, &c->d_owned, tp.owned)); HIPCHK(c, upload(A, &c->d_sowned, sowned));
    HIPCHK(c, A.alloc(&c->d_tiles, (size_t)c->slots_per_rank * ZR_TILE * ZR_TILE));
    const uint32_t mt = (c->n_tiles > c->sn_tiles ? c->n_tiles : c->sn_tiles) * ZR_TSTRIDE + 1;     // (the bins use the first sn_tiles + 1 words)
    HIPCHK(c, A.alloc(&c->sb.tile_count, mt)); HIPCHK(c, A.alloc(&c->sb.tile_offset, mt));
    HIPCHK(c, A.alloc(&c->sb.tile_cursor, mt)); HIPCHK(c, A.alloc(&c->sb.chunk_offset, mt));
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
    for (auto& v : c->d_vis) HIPCHK(c, A.alloc(&v, n));
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->raster_blocks = (uint32_t)prop.multiProcessorCount * ZR_TILE_WG_PER_CU; }      // k_tile's persistent grid (6 workgroups fit a CU: two rounds of them; A/B 4 / 6 / 8 / 12 / 16 / 32 per CU -> 5 133 / 5 250 / 5 294 / 5 344 / 5 327 / 5 277 Mpixel/s)
    c->shadow_blocks = c->raster_blocks / ZR_TILE_WG_PER_CU * 8u;      // the shadow rasteriser's persistent grid stays at 8 per CU
    c->slow0_cap = std::max<uint32_t>(c->slow0_cap, 128u * c->sn_tiles);      // (a clipped triangle is listed once per tile of its meshlet)
    HIPCHK(c, A.alloc(&c->d_slow0, 4ull * c->slow0_cap));
#ifdef ZR_DIAG
    if (const char* e = getenv("ZR_RASTER_BLOCKS")) c->raster_blocks = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("ZR_SHADOW_BLOCKS")) c->shadow_blocks = (uint32_t)std::max(1, atoi(e));
#endif
    size_t hiz_texels = 0;
    {   // Hi-Z pyramid: level l = max depth per (8 << l)^2 pixel block
        for (int l = 0; l < 4; ++l) { c->hiz.hw[l] = (c->W + (8u << l) - 1) / (8u << l); c->hiz.hh[l] = (c->H + (8u << l) - 1) / (8u << l); hiz_texels += (size_t)c->hiz.hw[l] * c->hiz.hh[l]; }
        c->hiz.fw = (c->W + 3u) / 4u; c->hiz.fh = (c->H + 3u) / 4u;
        hiz_texels += (size_t)c->hiz.fw * c->hiz.fh;
        HIPCHK(c, A.alloc(&c->d_hiz, hiz_texels));
        static_assert(ZR_TILE == 32 && ZR_SUPERTILE_SHIFT >= 1, "a 64 x 64 region of the pyramid must lie inside one super-tile");
        std::vector<uint32_t> regions;
        for (uint32_t ry = 0; ry < (c->H + 63u) / 64u; ++ry)
            for (uint32_t rx = 0; rx < (c->W + 63u) / 64u; ++rx)
                if (zr_tile_owner(rx * 2u, ry * 2u, c->cfg.tile_world) == c->cfg.tile_rank) regions.push_back(rx | ry << 16);
        c->n_hiz_regions = (uint32_t)regions.size();
        HIPCHK(c, A.alloc(&c->d_hiz_regions, regions.size()));
        if (!regions.empty()) HIPCHK(c, hipMemcpy(c->d_hiz_regions, regions.data(), regions.size() * 4, hipMemcpyHostToDevice));
        float* p = c->d_hiz;
        for (int l = 0; l < 4; ++l) { c->hiz.lvl[l] = p; p += (size_t)c->hiz.hw[l] * c->hiz.hh[l]; }
        c->hiz.fine = p;
    }
    HIPCHK(c, zr_fill_sync({ { c->fc[0].G.overlay, 0, n * 4 }, { c->fc[1].G.overlay, 0, n * 4 },
                             { c->d_stats, 0, sizeof(ZrDevStats) }, { c->d_sstats, 0, sizeof(ZrDevStats) }, { c->d_color, 0, n * 4 },
                             { c->d_rstats[0], 0, sizeof(ZrDevStats) }, { c->d_rstats[1], 0, sizeof(ZrDevStats) },
                             { c->d_tiles, 0, (size_t)c->slots_per_rank * ZR_TILE * ZR_TILE * 4 },
                             { c->sb.tile_count, 0, mt * 4 },       // k_bin_count counts into zeroes (k_scan zeroes the counts
                             { c->sb.tile_cursor, 0, mt * 4 },      // and the cursors again for the fill and the next frame)
                             { c->d_hiz, 0, hiz_texels * sizeof(float) } }));      // texels over other ranks' regions stay 0 ("hidden")
    for (auto& v : c->d_vis) zr_launch_fill64(v, (unsigned long long)0x3F800000u << 32 | ZR_EMPTY_PRIM, n, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // The runtime backs an event with a signal on its FIRST record and grows that pool in batches, which blocks the host for
    // milliseconds at unpredictable frames of a short run: record every event once now.
    for (auto& fr : c->evr) for (auto& e : fr) HIPCHK(c, hipEventRecord(e, c->stream));
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
        if (ns != c->stream) zr_casters_changed(c);      // (the kept map's two copies are ordered by their place on the host's stream too)
        c->stream = ns;
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ scene

extern "C" int zr_mesh_create(zr_ctx* c, const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, uint32_t* mesh_id)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, v && idx && mesh_id && nv > 0 && ni > 0 && ni % 3 == 0);
        for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) return zr_fail(c, ZR_ERR_ARG, "index out of range");
        ZrMesh m;
        m.v.assign(v, v + nv); m.idx.assign(idx, idx + ni);
        c->meshes.push_back(std::move(m));
        *mesh_id = (uint32_t)c->meshes.size() - 1;
        return ZR_OK;
    });
}

static int validate_meshlets(zr_ctx* c, const ZrMesh& m, const XkMeshlet* ml, uint32_t nm, size_t nmv, const uint32_t* mv,
                             size_t nmt, const uint8_t* mt)
{
    for (uint32_t i = 0; i < nm; ++i) {
        if (ml[i].VertexCount == 0 || ml[i].VertexCount > 64 || ml[i].TriangleCount == 0 || ml[i].TriangleCount > 128)
            return zr_fail(c, ZR_ERR_ARG, "meshlet exceeds 64 vertices / 128 triangles");
        if ((size_t)ml[i].VertexOffset + ml[i].VertexCount > nmv || (size_t)ml[i].TriangleOffset + 3u * ml[i].TriangleCount > nmt)
            return zr_fail(c, ZR_ERR_ARG, "meshlet range out of bounds");
        for (uint32_t k = 0; k < ml[i].VertexCount; ++k)
            if (mv[ml[i].VertexOffset + k] >= m.v.size()) return zr_fail(c, ZR_ERR_ARG, "meshlet vertex index out of range");
        for (uint32_t k = 0; k < 3u * ml[i].TriangleCount; ++k)
            if (mt[ml[i].TriangleOffset + k] >= ml[i].VertexCount) return zr_fail(c, ZR_ERR_ARG, "meshlet triangle corner out of range");
    }
    return ZR_OK;
}

extern "C" int zr_mesh_set_meshlets(zr_ctx* c, uint32_t mesh_id, const XkMeshlet* ml, uint32_t nm, const uint32_t* mv, size_t nmv, const uint8_t* mt, size_t nmt)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size() && ml && nm && mv && mt);
        ZrMesh& m = c->meshes[mesh_id];
        if (m.uploaded) return zr_fail(c, ZR_ERR_STATE, "mesh already in use by a rendered scene");
        int rc = validate_meshlets(c, m, ml, nm, nmv, mv, nmt, mt);
        if (rc) return rc;
        // CreateMeshVertexBuffers<XkMeshIndirect> (ZE:4733-4756): the draw becomes "meshlet by meshlet"; rebuild the
        // draw-order index buffer accordingly so primitive ids follow meshlet order.
        m.ms.meshlets.assign(ml, ml + nm); m.ms.mverts.assign(mv, mv + nmv); m.ms.mtris.assign(mt, mt + nmt);
        // Every cull trusts the bounding sphere to enclose the meshlet's vertices (and the cone to describe its triangles): a record
        // whose sphere does not is recomputed (ZM:149-166 fills them from meshopt_computeMeshletBounds, so a sound file never is).
        for (uint32_t i = 0; i < nm; ++i) {
            XkMeshlet& d = m.ms.meshlets[i];
            bool ok = std::isfinite(d.BoundsRadius) && d.BoundsRadius >= 0.0f;
            for (uint32_t k = 0; ok && k < d.VertexCount; ++k) {
                const float* q = m.v[mv[d.VertexOffset + k]].Position;
                const double dx = (double)q[0] - d.BoundsCenter[0], dy = (double)q[1] - d.BoundsCenter[1], dz = (double)q[2] - d.BoundsCenter[2];
                if (!(std::sqrt(dx * dx + dy * dy + dz * dz) <= (double)d.BoundsRadius * (1.0 + 1e-5) + 1e-30)) ok = false;
            }
            if (!ok) {
                XkMeshlet b = d;
                zr_meshlet_bounds(m.v.data(), mv + d.VertexOffset, d.VertexCount, mt + d.TriangleOffset, d.TriangleCount, &b);
                d = b;
            }
        }
        m.ms.tri_order.clear(); m.idx.clear();
        uint32_t base = 0;
        for (uint32_t i = 0; i < nm; ++i) {
            XkMeshlet& d = m.ms.meshlets[i];
            d.BindlessContext = base;
            for (uint32_t t = 0; t < d.TriangleCount; ++t) {
                for (int k = 0; k < 3; ++k) m.idx.push_back(mv[d.VertexOffset + mt[d.TriangleOffset + 3u * t + (uint32_t)k]]);
                m.ms.tri_order.push_back(base + t);
            }
            base += d.TriangleCount;
        }
        m.has_meshlets = true; zr_casters_changed(c);
        return ZR_OK;
    });
}

extern "C" int zr_mesh_build_meshlets(zr_ctx* c, uint32_t mesh_id, uint32_t max_v, uint32_t max_t, float cone_weight)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size());
        if (max_v == 0) max_v = 64;
        if (max_t == 0) max_t = 124;
        ARGCHK(c, max_v >= 3 && max_v <= 64 && max_t >= 1 && max_t <= 128);
        ZrMesh& m = c->meshes[mesh_id];
        if (m.uploaded) return zr_fail(c, ZR_ERR_STATE, "mesh already in use by a rendered scene");
        zr_build_meshlets(m.v.data(), (uint32_t)m.v.size(), m.idx.data(), (uint32_t)m.idx.size(), max_v, max_t, cone_weight, &m.ms);
        m.has_meshlets = true; zr_casters_changed(c);
        return ZR_OK;
    });
}

// Context-free form of the clusteriser: the ZeldaMeshlet tool's BuildMeshlets (ZM:132-172) as a library call.  Pure host
// code (runs without a GPU).  Pass NULL outputs to query the sizes.  tri_order[k] = index-buffer triangle of slot k.
extern "C" int zr_meshlets_build(const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, uint32_t max_v, uint32_t max_t, float cone_weight, XkMeshlet* ml, uint32_t* nm, uint32_t* mv, size_t* nmv, uint8_t* mt, size_t* nmt, uint32_t* tri_order)
{
    if (!v || !idx || !nm || !nmv || !nmt || nv == 0 || ni == 0 || ni % 3) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        if (max_v == 0) max_v = 64;
        if (max_t == 0) max_t = 124;
        if (max_v < 3 || max_v > 64 || max_t < 1 || max_t > 128) return ZR_ERR_ARG;
        for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) return ZR_ERR_ARG;
        ZrMeshletSet ms;
        zr_build_meshlets(v, nv, idx, ni, max_v, max_t, cone_weight, &ms);
        *nm = (uint32_t)ms.meshlets.size(); *nmv = ms.mverts.size(); *nmt = ms.mtris.size();
        if (ml) { memcpy(ml, ms.meshlets.data(), ms.meshlets.size() * sizeof(XkMeshlet)); for (uint32_t i = 0; i < *nm; ++i) ml[i].BindlessContext = 0; }
        if (mv) memcpy(mv, ms.mverts.data(), ms.mverts.size() * 4);
        if (mt) memcpy(mt, ms.mtris.data(), ms.mtris.size());
        if (tri_order) memcpy(tri_order, ms.tri_order.data(), ms.tri_order.size() * 4);
        return ZR_OK;
    });
}

extern "C" int zr_mesh_get_meshlets(zr_ctx* c, uint32_t mesh_id, XkMeshlet* ml, uint32_t* nm, uint32_t* mv, size_t* nmv, uint8_t* mt, size_t* nmt)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size());
        ZrMesh& m = c->meshes[mesh_id];
        if (ml) { int rc = zr_mesh_sync_host(c, m, true); if (rc) return rc; }      // (after vertex updates: the bounds of the current vertices)
        if (nm) *nm = (uint32_t)m.ms.meshlets.size();
        if (nmv) *nmv = m.ms.mverts.size();
        if (nmt) *nmt = m.ms.mtris.size();
        if (ml) { memcpy(ml, m.ms.meshlets.data(), m.ms.meshlets.size() * sizeof(XkMeshlet));
                  for (size_t i = 0; i < m.ms.meshlets.size(); ++i) ml[i].BindlessContext = 0; }
        if (mv) memcpy(mv, m.ms.mverts.data(), m.ms.mverts.size() * 4);
        if (mt) memcpy(mt, m.ms.mtris.data(), m.ms.mtris.size());
        return ZR_OK;
    });
}

int zr_material_prepare(zr_ctx* c, const zr_material* mat, ZrMaterialHost* out)
{
    for (int t = 0; t < 7; ++t) {
        const uint8_t* px = kDefaultTexel[t];
        out->image[t].clear(); out->w[t] = out->h[t] = 1;
        if (mat && mat->tex[t].rgba8) {
            const zr_image& im = mat->tex[t];
            if (im.width == 0 || im.height == 0 || im.width > 16384 || im.height > 16384) return zr_fail(c, ZR_ERR_ARG, "bad material image size");
            const size_t n = (size_t)im.width * im.height * 4;
            bool constant = true;
            for (size_t i = 4; i < n; ++i) if (im.rgba8[i] != im.rgba8[i & 3]) { constant = false; break; }
            px = im.rgba8;
            if (!constant) { out->image[t].assign(im.rgba8, im.rgba8 + n); out->w[t] = im.width; out->h[t] = im.height; }
        }
        out->texel[t] = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16 | (uint32_t)px[3] << 24;
    }
    for (int k = 0; k < 3; ++k) out->bc_linear[k] = zr_srgb_decode8((out->texel[0] >> (8 * k)) & 255u);
    return ZR_OK;
}

static int idx_clamp_h(float f, int hi) { f = fminf(fmaxf(f, 0.0f), (float)hi); return (int)f; }

// RHIGenerateMipmaps (ZE:6348-6433): level l+1 = vkCmdBlitImage(LINEAR) of level l at half size; mipLevels =
// floor(log2(max(w, h))) + 1 (ZE:6887).  Filtered on decoded values (sRGB for the base-colour slot, ZE:5878), re-encoded.
static void build_mip_chain(const zr_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h, bool srgb, std::vector<uint8_t>* chain, uint32_t* levels)
{
    uint32_t m = w > h ? w : h;
    uint32_t nl = 1; while (m > 1) { m >>= 1; nl++; }
    *levels = nl;
    chain->assign(rgba8, rgba8 + (size_t)w * h * 4);
    size_t src_off = 0;
    uint32_t sw = w, sh = h;
    for (uint32_t l = 1; l < nl; ++l) {
        const uint32_t dw = sw > 1 ? sw >> 1 : 1, dh = sh > 1 ? sh >> 1 : 1;
        const size_t dst_off = chain->size();
        chain->resize(dst_off + (size_t)dw * dh * 4);
        const uint8_t* src = chain->data() + src_off;
        uint8_t* dst = chain->data() + dst_off;
        const float kx = (float)sw / (float)dw, ky = (float)sh / (float)dh;
        for (uint32_t y = 0; y < dh; ++y) for (uint32_t x = 0; x < dw; ++x) {
            const float fu = fmaf((float)x + 0.5f, kx, -0.5f), fv = fmaf((float)y + 0.5f, ky, -0.5f);
            const float fx = floorf(fu), fy = floorf(fv), a = fu - fx, b = fv - fy;
            const int x0 = idx_clamp_h(fx, (int)sw - 1), x1 = idx_clamp_h(fx + 1.0f, (int)sw - 1);
            const int y0 = idx_clamp_h(fy, (int)sh - 1), y1 = idx_clamp_h(fy + 1.0f, (int)sh - 1);
            const uint8_t* p00 = src + ((size_t)y0 * sw + x0) * 4; const uint8_t* p10 = src + ((size_t)y0 * sw + x1) * 4;
            const uint8_t* p01 = src + ((size_t)y1 * sw + x0) * 4; const uint8_t* p11 = src + ((size_t)y1 * sw + x1) * 4;
            for (int ch = 0; ch < 4; ++ch) {
                const bool sr = srgb && ch < 3;
                const float t00 = sr ? c->lut[p00[ch]] : (float)p00[ch] / 255.0f, t10 = sr ? c->lut[p10[ch]] : (float)p10[ch] / 255.0f;
                const float t01 = sr ? c->lut[p01[ch]] : (float)p01[ch] / 255.0f, t11 = sr ? c->lut[p11[ch]] : (float)p11[ch] / 255.0f;
                const float top = fmaf(a, t10 - t00, t00), bot = fmaf(a, t11 - t01, t01);
                const float v = fmaf(b, bot - top, top);
                dst[((size_t)y * dw + x) * 4 + ch] = sr ? srgb_encode8(v) : (uint8_t)zr_unorm(v, 255.0f);
            }
        }
        src_off = dst_off; sw = dw; sh = dh;
    }
}

// An image for the kernels to sample: `bytes` into device memory of `own` (ZrOwn::alloc_image)
static int upload_bytes(zr_ctx* c, ZrOwn& own, const std::vector<uint8_t>& bytes, uint8_t** d)
{
    HIPCHK(c, own.alloc_image(d, bytes.size()));
    HIPCHK(c, hipMemcpy(*d, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    return ZR_OK;
}
// ... an RGBA8 image with its mip chain; `chain` (optional) keeps the chain on the host, for the packed material
static int upload_image(zr_ctx* c, ZrOwn& own, const uint8_t* rgba8, uint32_t iw, uint32_t ih, bool srgb, uint8_t** d, uint32_t* w, uint32_t* h,
                        uint32_t* levels, std::vector<uint8_t>* chain = nullptr)
{
    if (iw == 0 || ih == 0 || iw > 16384 || ih > 16384) return zr_fail(c, ZR_ERR_ARG, "bad image size");
    std::vector<uint8_t> mine;
    if (!chain) chain = &mine;
    build_mip_chain(c, rgba8, iw, ih, srgb, chain, levels);
    *w = iw; *h = ih;
    return upload_bytes(c, own, *chain, d);
}

// The material's images of `o`: mip chains and the packed form, into o.tex_mem (released first: a world update rebuilds a material here)
int zr_object_remake_material(zr_ctx* c, ZrSceneObject& o, const ZrMaterialHost& mat)
{
    o.tex_mem.release();
    for (int t = 0; t < 8; ++t) { o.d_tex[t] = nullptr; o.tex_w[t] = o.tex_h[t] = o.tex_levels[t] = 0; }
    o.mixed_sizes = false;
    memcpy(o.texel, mat.texel, sizeof o.texel); memcpy(o.bc_linear, mat.bc_linear, sizeof o.bc_linear);
    std::vector<uint8_t> chains[7];
    int lead = -1;                                          // first slot that holds an image
    for (int t = 0; t < 7; ++t) {
        if (mat.image[t].empty()) continue;
        int rc = upload_image(c, o.tex_mem, mat.image[t].data(), mat.w[t], mat.h[t], t == 0, &o.d_tex[t], &o.tex_w[t], &o.tex_h[t], &o.tex_levels[t], &chains[t]);
        if (rc) return rc;
        if (lead < 0) lead = t;
        else if (mat.w[t] != mat.w[lead] || mat.h[t] != mat.h[lead]) o.mixed_sizes = true;
    }
    if (lead >= 0 && !o.mixed_sizes) {
        // The packed material: per texel of the (common) mip chain the 13 channels BaseScene.frag reads, 16 B (ZR_PK_*); constant slots
        // put their constant there (the resolve takes those from the draw record, not from here).
        static const struct { int slot, ch, n; } kPack[7] = { {0, ZR_PK_BC, 3}, {1, ZR_PK_ME, 1}, {2, ZR_PK_RO, 1}, {3, ZR_PK_NO, 3}, {4, ZR_PK_AO, 1}, {5, ZR_PK_EM, 3}, {6, ZR_PK_MS, 1} };
        const size_t n_texels = chains[lead].size() / 4;
        std::vector<uint8_t> pk(n_texels * 16, 0);
        for (const auto& k : kPack) {
            const bool image = !chains[k.slot].empty();
            const uint8_t* src = image ? chains[k.slot].data() : nullptr;
            for (size_t i = 0; i < n_texels; ++i)
                for (int ch = 0; ch < k.n; ++ch)
                    pk[i * 16 + (size_t)k.ch + (size_t)ch] = image ? src[i * 4 + (size_t)ch] : (uint8_t)(mat.texel[k.slot] >> (8 * ch));
        }
        int rc = upload_bytes(c, o.tex_mem, pk, &o.d_tex[7]);
        if (rc) return rc;
        o.tex_w[7] = mat.w[lead]; o.tex_h[7] = mat.h[lead]; o.tex_levels[7] = o.tex_levels[lead];
    }
    return ZR_OK;
}

// The instance buffers of `o` from n_inst values (0: one identity record, not instanced), into o.mem (released first, and with it the
// update and visibility state: a world update re-makes an object of another instance count here).  Enqueued on the host's stream.
int zr_object_remake_instances(zr_ctx* c, ZrSceneObject& o, const XkInstanceData* inst, uint32_t n_inst)
{
    o.mem.release();
    o.d_inst = nullptr; o.d_raw = nullptr; o.upd = {}; o.pending[0] = o.pending[1] = 0; o.tab1 = false; o.host_stale = false;
    o.flag_pending[0] = o.flag_pending[1] = false; o.vis_stale = false; o.vis.clear();
    o.instanced = n_inst > 0; o.n_inst = n_inst ? n_inst : 1;
    o.inst.clear();
    if (n_inst) o.inst.assign(inst, inst + n_inst);
    HIPCHK(c, o.mem.alloc(&o.d_inst, o.n_inst));
    if (n_inst) {                       // (kept: the authoritative values of zr_object_set_instances / zr_object_update_instances_async)
        HIPCHK(c, o.mem.alloc(&o.d_raw, n_inst));
        HIPCHK(c, hipMemcpyAsync(o.d_raw, inst, sizeof(XkInstanceData) * n_inst, hipMemcpyHostToDevice, c->stream));
    }
    zr_launch_instance_prep(o.d_raw, o.d_inst, o.n_inst, o.instanced ? 1u : 0u, c->stream);
    return ZR_OK;
}

int zr_object_add_internal(zr_ctx* c, uint32_t mesh_id, const ZrMaterialHost& mat, const XkInstanceData* inst, uint32_t n_inst)
{
    ZrSceneObject o;
    o.mesh = mesh_id;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = zr_object_remake_material(c, o, mat);         // (a failure below drops `o`, and with it what it has made)
    if (rc == ZR_OK) rc = zr_object_remake_instances(c, o, inst, n_inst);
    if (rc) return rc;
    HIPCHK(c, zr_sync_all(c));
    c->objects.push_back(std::move(o));
    c->scene_dirty = true; c->scene_gen++; zr_casters_changed(c);
    return ZR_OK;
}

extern "C" int zr_object_add(zr_ctx* c, uint32_t mesh_id, const zr_material* mat, const XkInstanceData* inst, uint32_t n_inst)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size() && (n_inst == 0 || inst));
        ZrMaterialHost m;
        int rc = zr_material_prepare(c, mat, &m);
        if (rc) return rc;
        return zr_object_add_internal(c, mesh_id, m, inst, n_inst);
    });
}

// Capacities of the triangle-record arrays (chunks of 256 records) and of the clipped-triangle list, for hosts that size them themselves
// (0 = the default: 16 records per meshlet-instance, at least 32 Mi; 2^18 triangles).  Takes effect at the next frame.  The arrays hold at
// most 2^30 - 1 records (the kernels index them with 32-bit words): record_chunks beyond ZR_MAX_RECORD_CHUNKS is refused.
static constexpr uint32_t ZR_MAX_RECORD_CHUNKS = 0x3FFFFFFFu / 256u;
extern "C" int zr_set_limits(zr_ctx* c, uint32_t record_chunks, uint32_t slow_triangles)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (record_chunks > ZR_MAX_RECORD_CHUNKS) return zr_fail(c, ZR_ERR_ARG, "zr_set_limits: record_chunks above (2^30 - 1) / 256");
        c->limit_record_chunks = record_chunks; c->limit_slow_triangles = slow_triangles;
        c->work_capacity = 0; c->scene_dirty = true;          // the pools are re-made by the next frame
        zr_casters_changed(c);                                // (the shadow bins and the slow list with them)
        return ZR_OK;
    });
}

extern "C" int zr_set_bucket_share(zr_ctx* c, uint32_t percent)
{
    if (!c || percent < 1u || percent > 100u) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->bucket_pct = percent;          // (k_plan's argument from the next plan on; a frame that overflows its buckets is the same frame.
                                          // The camera pass's record buckets only: the shadow bins know nothing of it, the map is kept)
        return ZR_OK;
    });
}

static void drop_draw_tables(zr_ctx* c) { c->tables.release(); c->d_objs_b[0] = c->d_objs_b[1] = c->d_objs = nullptr; c->inst_dual = false; }

// (every object and mesh releases its device memory as it goes)
static void free_scene(zr_ctx* c)
{
    c->objects.clear(); c->scene_gen++; zr_casters_changed(c);
    c->meshes.clear();
    c->profabs.clear();
    drop_draw_tables(c);
    c->n_objs = 0; c->n_work = 0; c->scene_dirty = true;
}

extern "C" int zr_scene_clear(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        free_scene(c);
        return ZR_OK;
    });
}

static int upload_mesh(zr_ctx* c, ZrMesh& m)
{
    if (m.uploaded) return ZR_OK;
    m.mem.release();                    // (what an upload that failed part-way made)
    if (!m.has_meshlets) {
        zr_build_meshlets(m.v.data(), (uint32_t)m.v.size(), m.idx.data(), (uint32_t)m.idx.size(), 64, 124, 0.2f, &m.ms);
        m.has_meshlets = true;
    }
    // whole-mesh bounding sphere (centroid + max distance)
    double cx = 0, cy = 0, cz = 0;
    for (auto& v : m.v) { cx += v.Position[0]; cy += v.Position[1]; cz += v.Position[2]; }
    cx /= (double)m.v.size(); cy /= (double)m.v.size(); cz /= (double)m.v.size();
    double r = 0;
    for (auto& v : m.v) { double dx = v.Position[0] - cx, dy = v.Position[1] - cy, dz = v.Position[2] - cz; r = std::max(r, std::sqrt(dx * dx + dy * dy + dz * dz)); }
    m.center[0] = (float)cx; m.center[1] = (float)cy; m.center[2] = (float)cz; m.radius = (float)(r * 1.0001) + 1e-30f;
    // flatten for the kernels: one coalesced 16 B load per meshlet vertex, one 8 B load per meshlet triangle
    std::vector<float4> mpos(m.ms.mverts.size());
    for (size_t i = 0; i < mpos.size(); ++i) {
        const float* p = m.v[m.ms.mverts[i]].Position;
        mpos[i] = make_float4(p[0], p[1], p[2], 1.0f);
    }
    std::vector<uint2> mtri(m.ms.tri_order.size());
    for (const XkMeshlet& ml : m.ms.meshlets)
        for (uint32_t t = 0; t < ml.TriangleCount; ++t) {
            const uint8_t* tp = m.ms.mtris.data() + ml.TriangleOffset + 3u * t;
            mtri[ml.BindlessContext + t] = make_uint2((uint32_t)tp[0] | (uint32_t)tp[1] << 8 | (uint32_t)tp[2] << 16,
                                                      m.ms.tri_order[ml.BindlessContext + t]);
        }
    std::vector<ZrRVertex> rv(m.v.size());             // the resolve's vertex record: position + uv + the normalised normal
    for (size_t i = 0; i < rv.size(); ++i) {
        const XkVertex& x = m.v[i];
        const zf3 n = zr_normalize(zr3(x.Normal[0], x.Normal[1], x.Normal[2]));
        rv[i] = ZrRVertex{ x.Position[0], x.Position[1], x.Position[2], x.TexCoord[0], n.x, n.y, n.z, x.TexCoord[1] };
    }
    // ... and the same records per TRIANGLE CORNER in draw order (96 bytes a triangle): the resolve reaches a pixel's three corners from the
    // primitive id in one round trip instead of two (index, then vertex) - the kernel waits for its chain of dependent loads, not for arithmetic
    std::vector<ZrRVertex> rt(std::max<size_t>(1, m.idx.size()));
    for (size_t i = 0; i < m.idx.size(); ++i) rt[i] = rv[m.idx[i]];
    HIPCHK(c, upload(m.mem, &m.d_rt, rt));
    HIPCHK(c, upload(m.mem, &m.d_v, m.v)); HIPCHK(c, upload(m.mem, &m.d_rv, rv)); HIPCHK(c, upload(m.mem, &m.d_idx, m.idx)); HIPCHK(c, upload(m.mem, &m.d_meshlets, m.ms.meshlets));
    // draw-order triangle -> meshlet (the resolve marks the meshlet-instances that own a pixel)
    std::vector<uint32_t> tri_meshlet(std::max<size_t>(1, m.idx.size() / 3), 0u);
    for (size_t mi = 0; mi < m.ms.meshlets.size(); ++mi) {
        const XkMeshlet& ml = m.ms.meshlets[mi];
        for (uint32_t t = 0; t < ml.TriangleCount; ++t) {
            const uint32_t tri = m.ms.tri_order[ml.BindlessContext + t];
            if (tri < tri_meshlet.size()) tri_meshlet[tri] = (uint32_t)mi;
        }
    }
    std::vector<float4> mbox(2 * std::max<size_t>(1, m.ms.meshlets.size()), make_float4(0.0f, 0.0f, 0.0f, 0.0f));   // object-space box per meshlet
    for (size_t mi = 0; mi < m.ms.meshlets.size(); ++mi) {
        const XkMeshlet& ml = m.ms.meshlets[mi];
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t v = 0; v < ml.VertexCount; ++v) {
            const float4& q = mpos[ml.VertexOffset + v];
            const float e[3] = { q.x, q.y, q.z };
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], e[a]); hi[a] = std::max(hi[a], e[a]); }      // (a NaN coordinate drops out: k_geom sees it)
        }
        mbox[2 * mi] = make_float4(lo[0], lo[1], lo[2], 0.0f); mbox[2 * mi + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
    HIPCHK(c, upload(m.mem, &m.d_mpos, mpos)); HIPCHK(c, upload(m.mem, &m.d_mbox, mbox)); HIPCHK(c, upload(m.mem, &m.d_mtri, mtri)); HIPCHK(c, upload(m.mem, &m.d_tri_meshlet, tri_meshlet));
    m.uploaded = true;
    return ZR_OK;
}

// The work pools for cap_w meshlet-instances: the cull's lists, the shadow pass's bins, the camera pass's triangle records, the occlusion
// tests' boxes and flags.  A failed allocation returns with work_capacity 0 (and the caller's scene_dirty still set): the next frame
// tries again instead of launching on freed buffers.
static int make_work_pools(zr_ctx* c, uint32_t cap_w)
{
    ZrOwn& P = c->pools;
    P.release();
    c->work_capacity = 0; c->plan_valid = false;
    for (auto& o : c->objects) o.work_valid = false;      // (the history lived in the pools: finalize_scene reads it before it comes here)
    for (auto& sc : c->sc) sc = {};
    c->sb.bins = nullptr; c->sb.chunk_tab = nullptr; c->tb = {};
    c->d_pxrect = nullptr; c->d_zmin = nullptr; c->d_visflag[0] = c->d_visflag[1] = nullptr; c->d_spxrect = nullptr; c->d_szmin = nullptr; c->d_sflag = nullptr;
    const uint64_t cap = std::max<uint64_t>(1u << 20, 8ull * cap_w);
    c->bin_capacity = (uint32_t)std::min<uint64_t>(cap, 0x3FFFFFFFull);
    c->chunk_capacity = c->bin_capacity / ZR_CHUNK + std::max(c->n_tiles, c->sn_tiles) + 1u;
    for (auto& sc : c->sc) { HIPCHK(c, P.alloc(&sc.rects, cap_w)); HIPCHK(c, P.alloc(&sc.work, cap_w)); }
    HIPCHK(c, P.alloc(&c->sb.bins, c->bin_capacity)); HIPCHK(c, P.alloc(&c->sb.chunk_tab, c->chunk_capacity));
    // triangle-binned camera pass: triangle records (32 B) live in per-tile BUCKETS of two 16-byte planes, laid out every frame by
    // k_plan from the previous frame's per-tile counts; what lies behind the last bucket is the frame's overflow region (what a tile gets
    // beyond its bucket).  Sized from the scene: 16 records per meshlet-instance, at least 32 Mi - 1 GB of 288 reserved, touched as far as a frame
    // needs.  Planes that run full are reported like a bin overflow (zr_set_limits sizes them: 256 records per "chunk", at most 2^30 - 1 records).
    ZrTriBins& T = c->tb;
    T.n_waves = 8192; T.slow_cap = 1u << 18;
    // (16 per meshlet-instance: the frame after a camera cut at config 4 puts ~ 60 M records - 5 per meshlet-instance - into the 64
    // sections of the overflow region, unevenly; with 8 the fullest section ran over.  6 GB of 288 at 1 M instances.)
    uint64_t n_rec = std::min<uint64_t>(std::max<uint64_t>(32ull << 20, 16ull * cap_w), 0x3FFFFFFFull);
    if (c->limit_record_chunks) n_rec = 256ull * c->limit_record_chunks;      // zr_set_limits (a host sizing the planes; the overflow tests)
    if (c->limit_slow_triangles) T.slow_cap = std::max(2u, c->limit_slow_triangles);
    T.n_rec = (uint32_t)n_rec; T.bucket_max = (uint32_t)(n_rec - n_rec / 8u);
    T.n_tiles = c->n_tiles;
    T.unit_cap = T.bucket_max / (ZR_TCHUNK * ZR_TBATCHES) + 2u * c->n_tiles + 1u;
    HIPCHK(c, P.alloc(&T.sel, cap_w)); HIPCHK(c, P.alloc(&T.recA, (size_t)n_rec)); HIPCHK(c, P.alloc(&T.recB, (size_t)n_rec));
    HIPCHK(c, P.alloc(&T.over_tile, (size_t)n_rec)); HIPCHK(c, P.alloc(&T.plan, 2));
    HIPCHK(c, P.alloc(&T.tile_base, c->n_tiles)); HIPCHK(c, P.alloc(&T.tile_cap, c->n_tiles));
    HIPCHK(c, P.alloc(&T.cursor, (size_t)2 * c->n_tiles * ZR_TSTRIDE));
    HIPCHK(c, P.alloc(&T.over_cursor, 2 * ZR_OVER_SECTIONS)); HIPCHK(c, P.alloc(&T.n_units, 1));
    HIPCHK(c, P.alloc(&T.unit_tab, T.unit_cap)); HIPCHK(c, P.alloc(&T.wave_culled, T.n_waves)); HIPCHK(c, P.alloc(&T.slow, 4ull * T.slow_cap));
    HIPCHK(c, P.alloc(&c->d_pxrect, cap_w)); HIPCHK(c, P.alloc(&c->d_zmin, cap_w));
    HIPCHK(c, P.alloc(&c->d_visflag[0], cap_w)); HIPCHK(c, P.alloc(&c->d_visflag[1], cap_w));
    HIPCHK(c, P.alloc(&c->d_spxrect, cap_w)); HIPCHK(c, P.alloc(&c->d_szmin, cap_w)); HIPCHK(c, P.alloc(&c->d_sflag, cap_w));
    // (no plan yet: every bucket is empty - the first frame counts before it draws, see gbuffer_pass.  A fill that landed after the next
    // frame's k_plan would wipe the plan - every record then overflows into sections of capacity 0)
    HIPCHK(c, zr_fill_sync({ { T.tile_base, 0, (size_t)c->n_tiles * 4 }, { T.tile_cap, 0, (size_t)c->n_tiles * 4 },
                             { T.cursor, 0, (size_t)2 * c->n_tiles * ZR_TSTRIDE * 4 }, { T.over_cursor, 0, 2 * ZR_OVER_SECTIONS * 4 },
                             { T.n_units, 0, 4 }, { T.plan, 0, 8 },
                             { c->d_visflag[0], 0, cap_w }, { c->d_visflag[1], 0, cap_w } }));      // (no frame's stamp is 0)
    c->work_capacity = cap_w;              // every buffer is there
    return ZR_OK;
}

// CreateEngineScene's GPU half (ZE:4140-4284): meshlets, buffers, draw table in the reference's draw order
static int finalize_scene(zr_ctx* c)
{
    if (!c->scene_dirty) return ZR_OK;
    HIPCHK(c, zr_sync_all(c));
    for (auto& o : c->objects) { int rc = upload_mesh(c, c->meshes[o.mesh]); if (rc) return rc; }
    const bool sky = c->sky_set && c->sky_enabled;
    if (sky) { int rc = upload_mesh(c, c->sky_mesh); if (rc) return rc; }
    std::vector<ZrObject> tab;
    uint64_t work = 0, prim = 0, inst_total = 0;
    const uint32_t old_work = c->n_work;      // (the numbering the history on the device was written in)
    auto emit = [&](ZrSceneObject& o, const ZrMesh& m, uint32_t flags) {
        ZrObject d; memset(&d, 0, sizeof d);
        o.draw = (uint32_t)tab.size();
        d.verts = m.d_v; d.rverts = m.d_rv; d.rtris = m.d_rt; d.indices = m.d_idx; d.meshlets = m.d_meshlets; d.mpos = m.d_mpos; d.mbox = m.d_mbox; d.mtri = m.d_mtri; d.tri_meshlet = m.d_tri_meshlet;
        d.inst = o.d_inst;
        d.n_meshlets = (uint32_t)m.ms.meshlets.size(); d.n_tris = (uint32_t)(m.idx.size() / 3);
        d.n_inst = o.n_inst; d.instanced = o.instanced; d.flags = flags;
        d.work_base = (uint32_t)work; d.prim_base = (uint32_t)prim; d.inst_base = (uint32_t)inst_total;
        inst_total += d.n_inst;
        memcpy(d.texel, o.texel, sizeof d.texel); memcpy(d.bc_linear, o.bc_linear, sizeof d.bc_linear);
        for (int t = 0; t < 7; ++t)
            for (int ch = 0; ch < 4; ++ch) {
                const uint32_t v8 = (o.texel[t] >> (8 * ch)) & 255u;
                d.texc[t][ch] = (t == 0 && ch < 3) ? c->lut[v8] : (float)v8 / 255.0f;
            }
        for (int t = 0; t < 7; ++t) { d.tex[t].data = o.d_tex[t]; d.tex[t].w = o.tex_w[t]; d.tex[t].h = o.tex_h[t]; d.tex[t].levels = o.tex_levels[t]; d.tex[t]._pad = 0; }
        d.packed.data = o.d_tex[7]; d.packed.w = o.tex_w[7]; d.packed.h = o.tex_h[7]; d.packed.levels = o.tex_levels[7]; d.packed._pad = 0;
        memcpy(d.mesh_center, m.center, sizeof d.mesh_center); d.mesh_radius = m.radius;
        // BaseScene.frag on constant slots, once per draw instead of once per pixel (the kernels' own arithmetic: zr_math.h)
        for (int t = 0; t < 7; ++t) if (!o.d_tex[t]) d.const_slots |= 1u << t;
        const zf3 ts = zr_tangent_space_normal(zr3(d.texc[3][0], d.texc[3][1], d.texc[3][2]));
        d.ts_const[0] = ts.x; d.ts_const[1] = ts.y; d.ts_const[2] = ts.z;
        d.c_scene_color = zr_unorm(d.texc[5][0], 255.0f) | zr_unorm(d.texc[5][1], 255.0f) << 8 | zr_unorm(d.texc[5][2], 255.0f) << 16 | zr_unorm(d.texc[6][0], 255.0f) << 24;
        d.c_gB = zr_unorm(d.texc[1][0], 255.0f) | zr_unorm(1.0f, 255.0f) << 8 | zr_unorm(fmaxf(0.01f, d.texc[2][0]), 255.0f) << 16 | 255u << 24;
        d.c_gC = zr_unorm(d.texc[0][0], 255.0f) | zr_unorm(d.texc[0][1], 255.0f) << 8 | zr_unorm(d.texc[0][2], 255.0f) << 16 | zr_unorm(d.texc[4][0], 255.0f) << 24;
        work += (uint64_t)d.n_meshlets * d.n_inst; prim += (uint64_t)d.n_tris * d.n_inst;
        tab.push_back(d);
    };
    for (int pass = 0; pass < 2; ++pass)                 // non-instanced draws, then instanced draws (ZE:3445-3476)
        for (auto& o : c->objects)
            if ((int)o.instanced == pass) emit(o, c->meshes[o.mesh], o.hidden ? ZR_OBJ_HIDDEN : 0u);
    // The skydome is the table's last record but no work item of the shadow or the deferred-scene pass: it is drawn after the lighting
    // quad (ZE:3681-3691), depth-tested against the scene and colour only - k_sky_tiles + the resolve.
    const uint64_t scene_work = work, scene_inst = inst_total;
    if (sky) emit(c->sky_obj, c->sky_mesh, ZR_OBJ_SKY);
    if (work >= 0xFFFFFFFFull || prim >= 0xFFFFFFFFull) return zr_fail(c, ZR_ERR_OVERFLOW, "scene exceeds 2^32 meshlet-instances or primitives");
    drop_draw_tables(c);                // (zr_instances_table: table 1)
    HIPCHK(c, upload(c->tables, &c->d_objs_b[0], tab));
    c->d_objs = c->d_objs_b[0];
    c->n_objs = (uint32_t)tab.size(); c->n_work = (uint32_t)scene_work; c->n_inst_total = (uint32_t)scene_inst;
    { int rc = zr_instances_table(c); if (rc) return rc; }      // (objects with updated instances: the parity-1 table, n_objs records)
    c->sky_object = sky ? (uint32_t)tab.size() - 1u : 0u;
    if (sky && !c->d_sky_keys) HIPCHK(c, c->own.alloc(&c->d_sky_keys, (size_t)c->W * c->H));
    // A world update asked for the history to be carried (zr_ctx::history_remap): per kept draw the old work range and the new base; where
    // the instance count changed, the common prefix of instances.  The old planes are copied out first: ranges overlap when a base shifts
    // by less than a draw's length, in either direction, and make_work_pools releases the planes themselves.
    std::vector<ZrHistoryRange> ranges;
    uint64_t carried = 0;
    if (c->history_remap && old_work && c->d_visflag[0] && c->d_visflag[1] && c->d_sflag)
        for (const auto& o : c->objects) {
            const ZrObject& d = tab[o.draw];
            if (!o.work_valid || o.work_meshlets != d.n_meshlets) continue;
            const uint64_t count = (uint64_t)std::min(o.work_inst, d.n_inst) * d.n_meshlets;
            if (count == 0 || (uint64_t)o.work_base + count > old_work || (uint64_t)d.work_base + count > scene_work) continue;
            ranges.push_back({ d.work_base, o.work_base, (uint32_t)count, 0u });
            carried += count;
        }
    c->history_remap = false;
    std::sort(ranges.begin(), ranges.end(), [](const ZrHistoryRange& a, const ZrHistoryRange& b) { return a.new_base < b.new_base; });
    ZrOwn scratch;                      // (released when this returns, after the stream has drained)
    ZrHistoryCarry H = {};
    if (!ranges.empty()) {
        const size_t plane = ((size_t)old_work + 255u) & ~(size_t)255u;
        uint8_t* old = nullptr; ZrHistoryRange* d_ranges = nullptr;
        HIPCHK(c, scratch.alloc(&old, 3 * plane)); HIPCHK(c, upload(scratch, &d_ranges, ranges));
        const uint8_t* from[3] = { c->d_visflag[0], c->d_visflag[1], c->d_sflag };
        for (int k = 0; k < 3; ++k) { HIPCHK(c, hipMemcpyAsync(old + k * plane, from[k], old_work, hipMemcpyDeviceToDevice, c->stream)); H.src[k] = old + k * plane; }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        H.ranges = d_ranges; H.n_ranges = (uint32_t)ranges.size(); H.n_old = old_work; H.n_new = c->n_work;
    }
    if (c->n_work > c->work_capacity) { int rc = make_work_pools(c, c->n_work); if (rc) return rc; }
    c->any_images = c->mixed_images = false;
    for (const ZrObject& d : tab) for (int t = 0; t < 7; ++t) if (d.tex[t].data) c->any_images = true;
    for (const auto& o : c->objects) if (o.mixed_sizes) c->mixed_images = true;      // (the skydome's one image is sampled by itself)
    if (H.n_ranges) {
        // The marks and flags of the kept draws under their new numbers, stamp 0 and flag 1 everywhere else: vis_history, sflag_history,
        // vis_mark_prev, vis_cur and shadow_draws stay as they are, and so does the plan (per tile, not per work item) unless the pools
        // were re-made.  The camera lane reads the planes: the host waits for the carry.
        H.dst[0] = c->d_visflag[0]; H.dst[1] = c->d_visflag[1]; H.dst[2] = c->d_sflag;
        zr_launch_history_carry(H, c->stream);
        uint64_t moved[4] = { 0, 0, 0, 0 };      // the shadow flags' retest turn follows the items (zr_ctx::sflag_turn)
        for (const ZrHistoryRange& r : ranges) moved[(r.new_base - r.old_base) & 3u] += r.count;
        uint32_t d = 0;
        for (uint32_t k = 1; k < 4u; ++k) if (moved[k] > moved[d]) d = k;
        c->sflag_turn = (c->sflag_turn + 4u - d) & 3u;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        c->vis_history = false;         // work item numbering changed: last frame's visibility says nothing about this scene
        c->plan_valid = false;          // ... and neither do its per-tile record counts: the next frame counts before it draws (tri_raster)
        if (c->n_work) HIPCHK(c, hipMemsetAsync(c->d_sflag, 1, c->n_work, c->stream));      // shadow pass: everything is drawn in the first launch
        c->sflag_history = false;
    }
    c->history_items = carried;
    for (auto& o : c->objects) {        // the numbers the history knows the objects by from here on
        const ZrObject& d = tab[o.draw];
        o.work_base = d.work_base; o.work_inst = d.n_inst; o.work_meshlets = d.n_meshlets; o.work_valid = true;
    }
    c->list_valid[0] = c->list_valid[1] = false;      // ... and neither do the passes' work lists
    zr_casters_changed(c);                            // ... nor the kept shadow map: new draw table, maybe new pools
    c->scene_dirty = false;
    return ZR_OK;
}

int zr_scene_finalize(zr_ctx* c) { return finalize_scene(c); }

// ------------------------------------------------------------------------------------------------ skydome + background

extern "C" int zr_set_skydome(zr_ctx* c, const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, const zr_image* tex)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->sky_mesh = ZrMesh(); c->sky_obj = ZrSceneObject(); c->sky_set = false; c->scene_dirty = true;      // (releasing the old ones)
        c->world_named[1] = false;
        if (!tex || !tex->rgba8) return ZR_OK;
        ARGCHK(c, v && idx && nv > 0 && ni > 0 && ni % 3 == 0);
        for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) return zr_fail(c, ZR_ERR_ARG, "index out of range");
        c->sky_mesh.v.assign(v, v + nv); c->sky_mesh.idx.assign(idx, idx + ni);
        ZrSceneObject& o = c->sky_obj;
        o.mesh = 0; o.instanced = false; o.n_inst = 1;
        for (int t = 0; t < 7; ++t) o.texel[t] = 0xFFFFFFFFu;
        o.bc_linear[0] = o.bc_linear[1] = o.bc_linear[2] = 1.0f;
        int rc = upload_image(c, o.mem, tex->rgba8, tex->width, tex->height, true, &o.d_tex[0], &o.tex_w[0], &o.tex_h[0], &o.tex_levels[0]);   // sRGB by default, ZE:5860
        if (rc) return rc;
        HIPCHK(c, o.mem.alloc(&o.d_inst, 1));
        zr_launch_instance_prep(nullptr, o.d_inst, 1, 0u, c->stream);
        HIPCHK(c, zr_sync_all(c));
        c->sky_set = true;
        return ZR_OK;
    });
}

extern "C" int zr_set_background(zr_ctx* c, const zr_image* tex)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->bg_mem.release(); c->d_bg = nullptr; c->bg_set = false; c->world_named[2] = false;
        if (!tex || !tex->rgba8) return ZR_OK;
        int rc = upload_image(c, c->bg_mem, tex->rgba8, tex->width, tex->height, true, &c->d_bg, &c->bg_w, &c->bg_h, &c->bg_levels);
        if (rc) return rc;
        c->bg_set = true;
        return ZR_OK;
    });
}

extern "C" int zr_set_sky_flags(zr_ctx* c, int sky, int bg)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if ((sky != 0) != c->sky_enabled) c->scene_dirty = true;
        c->sky_enabled = sky != 0; c->bg_enabled = bg != 0;
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ cubemap

extern "C" int zr_set_cubemap(zr_ctx* c, const uint8_t* const faces[6], uint32_t dim)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        static const uint8_t grey[4] = { 127, 127, 127, 255 };
        if (!faces) dim = 1;
        ARGCHK(c, dim > 0 && dim <= 16384);
        if (faces) for (int f = 0; f < 6; ++f) ARGCHK(c, faces[f] != nullptr);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->cube_mem.release(); c->world_named[0] = false;
        memset(&c->cube, 0, sizeof c->cube);
        uint32_t levels = 1; for (uint32_t d = dim; d > 1; d >>= 1) levels++;      // floor(log2(dim)) + 1, ZE:6887
        if (levels > 16) return zr_fail(c, ZR_ERR_ARG, "cubemap too large");
        std::vector<std::vector<uint8_t>> lv(levels);
        const size_t fsz = (size_t)dim * dim * 4;
        lv[0].resize(fsz * 6);
        for (int f = 0; f < 6; ++f) { if (faces) memcpy(lv[0].data() + fsz * f, faces[f], fsz); else memcpy(lv[0].data() + fsz * f, grey, 4); }
        uint32_t d = dim;
        for (uint32_t l = 1; l < levels; ++l) {        // RHIGenerateMipmaps: vkCmdBlitImage LINEAR from level l-1 (2x2 box, linear light)
            const uint32_t nd = d > 1 ? d >> 1 : 1;
            lv[l].resize((size_t)nd * nd * 4 * 6);
            for (int f = 0; f < 6; ++f) {
                const uint8_t* src = lv[l - 1].data() + (size_t)d * d * 4 * f;
                uint8_t* dst = lv[l].data() + (size_t)nd * nd * 4 * f;
                for (uint32_t y = 0; y < nd; ++y) for (uint32_t x = 0; x < nd; ++x) {
                    const uint32_t x0 = 2 * x, x1 = (2 * x + 1 < d) ? 2 * x + 1 : d - 1, y0 = 2 * y, y1 = (2 * y + 1 < d) ? 2 * y + 1 : d - 1;
                    const uint8_t* p00 = src + ((size_t)y0 * d + x0) * 4; const uint8_t* p10 = src + ((size_t)y0 * d + x1) * 4;
                    const uint8_t* p01 = src + ((size_t)y1 * d + x0) * 4; const uint8_t* p11 = src + ((size_t)y1 * d + x1) * 4;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float a = (c->lut[p00[ch]] + c->lut[p10[ch]]) + (c->lut[p01[ch]] + c->lut[p11[ch]]);
                        dst[((size_t)y * nd + x) * 4 + ch] = srgb_encode8(a * 0.25f);
                    }
                    const uint32_t al = (uint32_t)p00[3] + p10[3] + p01[3] + p11[3];
                    dst[((size_t)y * nd + x) * 4 + 3] = (uint8_t)((al + 2) >> 2);
                }
            }
            d = nd;
        }
        for (uint32_t l = 0; l < levels; ++l) {
            uint8_t* p = nullptr;
            HIPCHK(c, upload(c->cube_mem, &p, lv[l]));
            c->cube.levels[l] = p;
        }
        c->cube_dim = dim; c->cube_levels = levels;
        c->view.LightsCount[3] = (int32_t)levels;       // CubemapMaxMips, ZE:4308
        c->view_dirty = true;
        return ZR_OK;
    });
}

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
        if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_update_uniforms between the stages of a frame (finish it with zr_render_lighting first)");
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
        if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_set_frame between the stages of a frame (finish it with zr_render_lighting first)");
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
static int set_winner_planes(zr_ctx* c, bool forward, bool id_capture, const char* what)
{
    const size_t n = (size_t)c->W * c->H;
    for (FrameCopy& F : c->fc) {
        if ((forward || id_capture) && !F.prim_plane) {
            if (c->own.alloc(&F.prim_plane, n) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, std::string(what) + ": out of device memory");
            HIPCHK(c, zr_fill_sync({ { F.prim_plane, 0xFF, n * 4 } }));
        }
        F.G.prim = (forward || id_capture) ? F.prim_plane : nullptr;
    }
    return ZR_OK;
}

// Forward variant (SH/Base.frag): the resolve additionally keeps each pixel's winning primitive id (set_winner_planes), and the lighting
// step runs k_forward on those instead of k_lighting on the GBuffer.
extern "C" int zr_set_shading(zr_ctx* c, uint32_t mode)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (mode != ZR_SHADING_DEFERRED && mode != ZR_SHADING_FORWARD) return zr_fail(c, ZR_ERR_ARG, "zr_set_shading: unknown mode");
        if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_set_shading between the stages of a frame");
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

// The current shadow map: during a drawn shadow pass the one being drawn, else the one the last drawn pass left (zr_ctx::smap).
static inline float* shadow_buf(zr_ctx* c) { return c->d_shadow_ext ? c->d_shadow_ext : c->fc[c->smap].shadow; }
// Contexts whose map is never kept (every frame draws it): the host reduces or gathers a partitioned or caller-owned map in place;
// ZR_FLAG_NO_LIST_REUSE asks to recompute what standing inputs would let the library keep; ZR_FLAG_SHADOW_OCCLUSION forces a variant of
// the pass for A/B, whose per-frame history statistics are what its callers read.
static inline bool shadow_keepable(const zr_ctx* c)
{
    return !c->d_shadow_ext && c->cfg.tile_world <= 1u && c->shadow_world <= 1u && c->stile_world <= 1u &&
           !(c->cfg.flags & (ZR_FLAG_NO_LIST_REUSE | ZR_FLAG_SHADOW_OCCLUSION));
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

// The frame in three stages so that a multi-GPU host can put collectives between them (zeldaengine_amd/dist.py):
//   zr_render_shadow    shadow pass (ZE:3239-3393) of this rank's share of the instances
//   zr_render_gbuffer   deferred-scene pass (ZE:3417-3480): cull + bin + raster + resolve of the owned tiles
//   zr_render_lighting  deferred-lighting pass (ZE:3531-3540) [+ skydome / background overlay]
// zr_render = all three.
// Object identity (zr_set_id_capture): the census's draw table - draw order, as finalize_scene numbers primitives, with each draw's add-order
// object index and first instance slot - and the per-slot arrays of the queries.  Built at the start of a captured frame, when the
// scene's objects changed since.
static int ids_prepare(zr_ctx* c)
{
    if (c->ids_table_gen == c->scene_gen && c->d_ids_draws) return ZR_OK;
    std::vector<uint32_t> slot_base(c->objects.size());
    uint32_t slots = 0;
    for (size_t i = 0; i < c->objects.size(); ++i) { slot_base[i] = slots; slots += c->objects[i].n_inst; }
    std::vector<ZrIdsDraw> tab;
    uint32_t prim = 0;
    for (int pass = 0; pass < 2; ++pass)                 // the draw order of finalize_scene (ZE:3445-3476)
        for (size_t i = 0; i < c->objects.size(); ++i) {
            const ZrSceneObject& o = c->objects[i];
            if ((int)o.instanced != pass) continue;
            const uint32_t nt = (uint32_t)(c->meshes[o.mesh].idx.size() / 3);
            tab.push_back({ prim, nt ? nt : 1u, (uint32_t)i, slot_base[i] });
            prim += nt * o.n_inst;
        }
    tab.push_back({ prim, 1u, 0xFFFFFFFFu, slots });     // sentinel: the end of the last draw
    HIPCHK(c, zr_sync_all(c));                           // (queries of an earlier scene may still read the old table)
    c->ids_table.release(); c->d_ids_draws = nullptr;
    HIPCHK(c, upload(c->ids_table, &c->d_ids_draws, tab));
    c->ids_n_draws = (uint32_t)tab.size() - 1u;
    c->ids_n_slots = slots;
    if (slots > c->ids_slot_cap || !c->d_ids_counts) {
        ZrOwn& P = c->ids_pool;
        P.release(); c->d_ids_counts = c->d_ids_cov = c->d_ids_list = c->d_ids_n = nullptr; c->d_ids_keys = nullptr; c->d_ids_hits = nullptr;
        c->ids_slot_cap = 0;
        const size_t cap = std::max<uint32_t>(slots, 1u);
        HIPCHK(c, P.alloc(&c->d_ids_counts, cap)); HIPCHK(c, P.alloc(&c->d_ids_cov, cap)); HIPCHK(c, P.alloc(&c->d_ids_list, cap));
        HIPCHK(c, P.alloc(&c->d_ids_n, 1)); HIPCHK(c, P.alloc(&c->d_ids_keys, cap)); HIPCHK(c, P.alloc(&c->d_ids_hits, cap));
        // between queries: counts 0, keys all ones, no listed slot (k_id_hits restores this after every pick)
        HIPCHK(c, zr_fill_sync({ { c->d_ids_counts, 0, cap * 4 }, { c->d_ids_keys, 0xFF, cap * 8 }, { c->d_ids_n, 0, 4 } }));
        c->ids_slot_cap = (uint32_t)cap;
    }
    c->ids_table_gen = c->scene_gen;
    return ZR_OK;
}

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
    int rc = finalize_scene(c);
    if (rc) return rc;
    if (c->view.LightsCount[3] != (int32_t)c->cube_levels) { c->view.LightsCount[3] = (int32_t)c->cube_levels; c->view_dirty = true; }
    c->ids_frame = false; c->ids_this = c->id_capture;      // (the frame enqueued last is about to be this one)
    if (c->id_capture) { rc = ids_prepare(c); if (rc) return rc; }
    c->fcur = (int)(c->frame_no & 1u);
    FrameCopy& F = c->fc[c->fcur];
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
    if (c->plan_behind_cam && s == c->stream && c->cam_s) { HIPCHK(c, hipEventRecord(c->ev_lane, c->cam_s)); HIPCHK(c, hipStreamWaitEvent(s, c->ev_lane, 0)); }
    c->plan_behind_cam = false;
    // ... and by an identity census enqueued against them since (zr_instance_coverage_async, on the host's stream)
    if (F.ids_wait) { if (s != c->stream) HIPCHK(c, hipStreamWaitEvent(s, F.ev_ids, 0)); F.ids_wait = false; }
    // this frame's draw table; instance updates since the last frame of this parity go into its planes (zr_instances_host.cpp)
    rc = zr_instances_frame(c, s, c->fcur);
    if (rc) return rc;
    rc = zr_texture_frame(c, s);          // ... and behind the last texture update (zr_texture_update_host.cpp)
    if (rc) return rc;
    c->timing_now = c->timing_interval != 0 && c->frame_no % c->timing_interval == 0;     // pass events cost ~6 us of stream bubble each
    hipEvent_t* ev = c->timing_now ? c->evr[c->sample_no % zr_ctx::EV_RING] : nullptr;
    if (ev) HIPCHK(c, hipEventRecord(ev[0], s));
    if (c->view_dirty) { c->view_version++; c->view_dirty = false; }
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
    // ... and the shadow pass's map as a whole while, beyond that, no caster changed and the map stays where it is (shadow_pass)
    c->shadow_keep = shadow_keepable(c) && c->smap_valid && c->smap_epoch == c->caster_epoch && memcmp(&c->smap_key, &c->pass[0], sizeof(ZrPass)) == 0;
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
    zr_launch_frame_begin(c->d_stats, src, F.view, rebuild & 2u, s);
    if (src) { HIPCHK(c, hipEventRecord(c->view_ev[k], s)); F.view_uploaded = c->view_version; }
    return ZR_OK;
}

// shadow pass (ZE:3239-3393) of this rank's share of the instances, on stream s
static int shadow_pass(zr_ctx* c, hipStream_t s)
{
    hipEvent_t* ev = c->timing_now ? c->evr[c->sample_no % zr_ctx::EV_RING] : nullptr;
    const ZrPass& P = c->pass[0];      // (built by frame_begin)
    if (ev) c->ev_kept[c->sample_no % zr_ctx::EV_RING] = c->shadow_keep;
    if (c->shadow_keep) {
        // The map of the last drawn pass is this frame's, bit for bit: nothing is launched.  Its statistics block, last_work[0] and the
        // occlusion flags stay as that pass left them; a timed frame records its two events all the same (no elapsed-time call meets an
        // unrecorded one), and the sample counts as 0 (zr_get_pass_times_avg).
        if (ev) { HIPCHK(c, hipEventRecord(ev[1], s)); HIPCHK(c, hipEventRecord(ev[2], s)); }
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
    if (ev) HIPCHK(c, hipEventRecord(ev[1], s));
    raster(c, P, s, occl ? 1 : 0);
    if (occl) {
        zr_launch_shadow_occlusion(P, c->d_objs, c->sc[0].work, c->sc[0].rects, c->d_spxrect, c->d_szmin, c->d_sflag, (const uint32_t*)shadow_buf(c),
                                   c->sb.bins, c->d_sstats, c->shadow_blocks * 8u, c->sflag_history ? (uint32_t)((c->shadow_draws + c->sflag_turn) & 3u) : 4u, s);      // (a turn per pass DRAWN: kept frames test nothing)
        c->sflag_history = true;
        raster(c, P, s, 2);
    }
    if (ev) HIPCHK(c, hipEventRecord(ev[2], s));
    HIPCHK(c, hipGetLastError());
    c->shadow_draws++;
    c->smap_key = P; c->smap_epoch = c->caster_epoch; c->smap_valid = true;
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
    hipEvent_t* ev = c->timing_now ? c->evr[c->sample_no % zr_ctx::EV_RING] : nullptr;
    if (ev) HIPCHK(c, hipEventRecord(ev[9], s));
    ZrPass P = c->pass[1];             // (built by frame_begin; the overlay fields are set below)
    c->gbuf_s = s;
    c->last_work[1] = P.n_work;
    // Two-pass occlusion culling: round 1 draws the meshlet-instances that owned a pixel last frame, a Hi-Z pyramid of the
    // result rejects what it hides, round 2 draws the rest.  The depth test decides every pixel either way, so the frame does
    // not depend on the history; without one (first frame of a scene) or with ZR_FLAG_NO_HIZ everything is drawn at once.
    const bool hiz_on = !(c->cfg.flags & ZR_FLAG_NO_HIZ) && P.n_work != 0;
    ZrHiz Z = c->hiz;
    Z.tiles_x = c->tiles_x; Z.tile_rank = c->cfg.tile_rank; Z.tile_world = c->cfg.tile_world;
    Z.pxrect = hiz_on ? c->d_pxrect : nullptr; Z.zmin = hiz_on ? c->d_zmin : nullptr;
    Z.vis_prev = c->d_visflag[c->vis_cur ^ 1]; Z.vis_now = hiz_on ? c->d_visflag[c->vis_cur] : nullptr;
    // visibility marks are frame stamps (1 .. 255): the resolve writes this frame's, the culls compare with last frame's - nothing is cleared
    const uint32_t vis_mark = 1u + (uint32_t)(c->frame_no % 255u);
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
    if (two) {
        Z.phase = 1;
        if (ev) HIPCHK(c, hipEventRecord(ev[3], s));
        tri_raster(c, P, Z, 1, s, false, count_first);
        if (ev) HIPCHK(c, hipEventRecord(ev[4], s));
        zr_launch_hiz_build(c->d_vis[c->fcur], c->W, c->H, Z, c->d_hiz_regions, c->n_hiz_regions, s);
        Z.phase = 2;
        tri_select(c, P, Z, 2, s);
        if (ev) HIPCHK(c, hipEventRecord(ev[5], s));
        tri_raster(c, P, Z, 2, s, true, false);
    } else {
        if (ev) HIPCHK(c, hipEventRecord(ev[3], s));
        tri_raster(c, P, Z, 1, s, true, count_first);
        if (ev) { HIPCHK(c, hipEventRecord(ev[4], s)); HIPCHK(c, hipEventRecord(ev[5], s)); }
    }
    {   // the overlay plane (skydome pixels) is written only when a skydome is drawn, or once more to wipe one that was
        const bool sky = c->sky_set && c->sky_enabled;
        P.write_overlay = (sky || c->fc[c->fcur].overlay_dirty) ? 1u : 0u;
        c->fc[c->fcur].overlay_dirty = sky;
        P.sky_keys = nullptr; P.sky_object = c->sky_object;
        if (sky && c->d_sky_keys) { zr_launch_sky_tiles(P, c->d_objs, c->d_owned, c->n_owned, c->d_sky_keys, s); P.sky_keys = c->d_sky_keys; }
    }
    if (ev) { HIPCHK(c, hipEventRecord(ev[6], s)); c->ev_moved[c->sample_no % zr_ctx::EV_RING] = defer_resolve; }
    c->resolve_deferred = defer_resolve;
    if (defer_resolve) {
        // the history now, the planes later: the host's stream waits for everything up to here and resolves from the same keys
        zr_launch_mark(P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], Z.vis_now, s, vis_mark);
        if (ev) HIPCHK(c, hipEventRecord(ev[10], s));
        c->resolve_P = P; c->resolve_mark = vis_mark;
        HIPCHK(c, hipEventRecord(c->ev_cam, s)); c->camera_on_lane = true; c->plan_behind_cam = true;
    } else {
        zr_launch_resolve_gbuffer(P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], c->fc[c->fcur].G, c->d_lut, c->d_unorm_lut, Z.vis_now, c->d_stats, s, vis_mark);
        c->cov_block = c->d_stats;
        if (ev) HIPCHK(c, hipEventRecord(ev[7], s));
        if (ZR_EV_CAM_AHEAD_OF_PLAN && c->in_render && s != c->stream) { HIPCHK(c, hipEventRecord(c->ev_cam, s)); c->camera_on_lane = true; c->plan_behind_cam = true; }
    }
    c->vis_mark_prev = vis_mark;
    if (P.n_work != 0) {     // the next frame's buckets, from this frame's counts: nothing of this frame waits for it
        zr_launch_plan(c->tb, c->d_owned, c->n_owned, c->d_stats, false, c->bucket_pct, s);
        c->plan_valid = true; c->plan_two_round = two;
    }
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
        if (rc == ZR_OK) rc = gbuffer_pass(c, c->cam_s, defer);
        // (a deferred resolve: ev_cam is already recorded, behind k_mark and ahead of k_plan - the lighting lane does not wait for the plan)
        if (rc == ZR_OK && !c->camera_on_lane) { HIPCHK(c, hipEventRecord(c->ev_cam, c->cam_s)); c->camera_on_lane = true; }
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
    hipEvent_t* ev = c->timing_now ? c->evr[c->sample_no % zr_ctx::EV_RING] : nullptr;
    ZrDevStats* const tally = c->d_rstats[c->fcur];
    zr_launch_fill32(tally->covered_part, 0u, 32, s);
    if (ev) HIPCHK(c, hipEventRecord(ev[11], s));
    zr_launch_resolve_gbuffer(c->resolve_P, c->d_objs, c->d_owned, c->n_owned, c->d_vis[c->fcur], c->fc[c->fcur].G, c->d_lut, c->d_unorm_lut, nullptr, tally, s, c->resolve_mark);
    if (ev) HIPCHK(c, hipEventRecord(ev[7], s));
    c->cov_block = tally; c->resolve_deferred = false;
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}

static int lighting_pass(zr_ctx* c, hipStream_t s)
{
    hipEvent_t* ev = c->timing_now ? c->evr[c->sample_no % zr_ctx::EV_RING] : nullptr;
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
    if (ev) HIPCHK(c, hipEventRecord(ev[8], s));
    HIPCHK(c, hipEventRecord(c->ev_end[c->frame_no % zr_ctx::END_RING], s));      // this frame's GBuffer / shadow map / uniforms copies are free again
    HIPCHK(c, hipGetLastError());
    if (c->timing_now) c->sample_no++;
    c->rendered = true; c->frame_no++; c->stage = 0;
    c->ids_frame = c->ids_this; c->ids_gen = c->scene_gen;
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
        if (rc == ZR_OK) rc = empty_pixel_pass(c, ls); // the shadow map (possibly reduced over ranks by the host) is final only now
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
        if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_set_shadow_tiles between the stages of a frame");
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

// The shadow pipeline's block: its slot-0 counters and its overflow latch belong to the frame's statistics
static void merge_shadow_stats(zr_ctx* c, const ZrDevStats& sh)
{
    ZrDevStats& h = c->h_stats;
    h.survivors[0] = sh.survivors[0]; h.bin_entries[0] = sh.bin_entries[0]; h.n_chunks[0] = sh.n_chunks[0];
    h.n_slow[0] = sh.n_slow[0]; h.n_vis_work[0] = sh.n_vis_work[0];
    // (k_shadow_occlusion tallies in 32 partial sums; survivors of the cull = drawn by the first launch + left out + drawn late)
    h.shadow_occluded = 0; for (uint32_t v : sh.covered_part) h.shadow_occluded += v;
    h.shadow_late = sh.shadow_late;
    h.survivors[0] += h.shadow_occluded + h.shadow_late;
    h.overflow |= sh.overflow;
    if (!h.overflow_sticky) h.overflow_sticky = sh.overflow_sticky;      // (a ZR_OVF_* code: the camera lane's, else the pipeline's)
}

extern "C" int zr_finish(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        if (c->rendered) {
            HIPCHK(c, hipMemcpy(&c->h_stats, c->d_stats, sizeof(ZrDevStats), hipMemcpyDeviceToHost));
            if (c->cov_block != c->d_stats)       // the newest frame's resolve ran on the host's stream and counted into its own block
                HIPCHK(c, hipMemcpy(c->h_stats.covered_part, c->cov_block->covered_part, sizeof c->h_stats.covered_part, hipMemcpyDeviceToHost));
            ZrDevStats sh;
            HIPCHK(c, hipMemcpy(&sh, c->d_sstats, sizeof(ZrDevStats), hipMemcpyDeviceToHost));
            merge_shadow_stats(c, sh);
            c->h_stats.covered_shadow = 0;
            if (c->h_stats.overflow_sticky) {     // latched by ANY frame since the last zr_finish, not only the newest one
                HIPCHK(c, zr_fill_sync({ { &c->d_stats->overflow_sticky, 0, sizeof(uint32_t) }, { &c->d_sstats->overflow_sticky, 0, sizeof(uint32_t) } }));
                c->h_stats.overflow = 1u;
                static const char* const what[] = { "?", "shadow bin entries", "slow-triangle list (zr_set_limits)", "camera work-unit table", "triangle-record arrays (zr_set_limits)",
                                                    "late shadow bin entries" };
                const uint32_t code = c->h_stats.overflow_sticky < 6u ? c->h_stats.overflow_sticky : 0u;
                char msg[160];
                snprintf(msg, sizeof msg, "tile bin list overflow (%s): a frame since the last zr_finish is incomplete", what[code]);
                return zr_fail(c, ZR_ERR_OVERFLOW, msg);
            }
        }
        return ZR_OK;
    });
}

// Mean per-pass GPU time over the last `last_n` frames (<= EV_RING), from hipEvents recorded on the render stream.
extern "C" int zr_get_pass_times_avg(zr_ctx* c, uint32_t last_n, float ms[ZR_PASS_COUNT])
{
    if (!c || !ms) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, "nothing rendered yet");
        int rc = zr_finish(c);
        if (rc && rc != ZR_ERR_OVERFLOW) return rc;
        if (last_n == 0) last_n = 1;
        if (last_n > (uint32_t)zr_ctx::EV_RING) last_n = zr_ctx::EV_RING;
        if (c->sample_no == 0) return zr_fail(c, ZR_ERR_STATE, "no timed frame yet (zr_set_timing_interval)");
        if ((uint64_t)last_n > c->sample_no) last_n = (uint32_t)c->sample_no;
        double acc[ZR_PASS_COUNT] = { 0 };
        for (uint32_t k = 0; k < last_n; ++k) {
            hipEvent_t* ev = c->evr[(c->sample_no - 1 - k) % zr_ctx::EV_RING];
            float t[ZR_PASS_COUNT] = { 0 };
            (void)hipEventElapsedTime(&t[ZR_PASS_CULL_SHADOW], ev[0], ev[1]);
            (void)hipEventElapsedTime(&t[ZR_PASS_SHADOW], ev[1], ev[2]);
            (void)hipEventElapsedTime(&t[ZR_PASS_CULL_CAMERA], ev[9], ev[3]);
            (void)hipEventElapsedTime(&t[ZR_PASS_GBUFFER], ev[3], ev[4]);
            (void)hipEventElapsedTime(&t[ZR_PASS_HIZ], ev[4], ev[5]);
            (void)hipEventElapsedTime(&t[ZR_PASS_GBUFFER2], ev[5], ev[6]);
            if (c->ev_moved[(c->sample_no - 1 - k) % zr_ctx::EV_RING]) {
                // the resolve on the host's stream: k_mark on the camera lane + the resolve itself, each between two records on the stream
                // it ran on (never across the wait between the lanes)
                float tm = 0.0f, tr = 0.0f;
                (void)hipEventElapsedTime(&tm, ev[6], ev[10]); (void)hipEventElapsedTime(&tr, ev[11], ev[7]);
                t[ZR_PASS_RESOLVE] = tm + tr;
            } else (void)hipEventElapsedTime(&t[ZR_PASS_RESOLVE], ev[6], ev[7]);
            (void)hipEventElapsedTime(&t[ZR_PASS_LIGHTING], ev[7], ev[8]);
            (void)hipEventElapsedTime(&t[ZR_PASS_TOTAL], ev[0], ev[8]);
            // (a frame that kept its shadow map ran no shadow pipeline: exactly 0, not the gap between two back-to-back records)
            if (c->ev_kept[(c->sample_no - 1 - k) % zr_ctx::EV_RING]) t[ZR_PASS_CULL_SHADOW] = t[ZR_PASS_SHADOW] = 0.0f;
            for (int i = 0; i < ZR_PASS_COUNT; ++i) acc[i] += t[i];
        }
        for (int i = 0; i < ZR_PASS_COUNT; ++i) ms[i] = (float)(acc[i] / last_n);
        return ZR_OK;
    });
}
extern "C" int zr_get_pass_times(zr_ctx* c, float ms[ZR_PASS_COUNT]) { return zr_guard(c, [&]() -> int { return zr_get_pass_times_avg(c, 1, ms); }); }

// Begin-to-end GPU time (first kernel of the camera lane to the end of the lighting pass) of each of the last `n` timed frames,
// newest first; returns how many were written.  With two frames in flight this latency is longer than the frame period.
extern "C" int zr_get_frame_latencies(zr_ctx* c, uint32_t n, float* ms)
{
    if (!c || !ms) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, "nothing rendered yet");
        int rc = zr_finish(c);
        if (rc && rc != ZR_ERR_OVERFLOW) return rc;
        if (n > (uint32_t)zr_ctx::EV_RING) n = zr_ctx::EV_RING;
        if ((uint64_t)n > c->sample_no) n = (uint32_t)c->sample_no;
        for (uint32_t k = 0; k < n; ++k) {
            hipEvent_t* ev = c->evr[(c->sample_no - 1 - k) % zr_ctx::EV_RING];
            ms[k] = 0.0f;
            (void)hipEventElapsedTime(&ms[k], ev[0], ev[8]);
        }
        return (int)n;
    });
}

// GPU time between the ends of consecutive frames (the frame period the GPU sustained) for the last `n` frames, newest first;
// returns how many were written (<= END_RING - 1).  Costs nothing extra: the end-of-frame event exists for the double buffering.
extern "C" int zr_get_frame_periods(zr_ctx* c, uint32_t n, float* ms)
{
    if (!c || !ms) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, "nothing rendered yet");
        int rc = zr_finish(c);
        if (rc && rc != ZR_ERR_OVERFLOW) return rc;
        const uint64_t have = c->frame_no > 0 ? c->frame_no - 1 : 0;
        if (n > (uint32_t)zr_ctx::END_RING - 1u) n = zr_ctx::END_RING - 1;
        if ((uint64_t)n > have) n = (uint32_t)have;
        for (uint32_t k = 0; k < n; ++k) {
            const uint64_t f = c->frame_no - 1 - k;
            ms[k] = 0.0f;
            (void)hipEventElapsedTime(&ms[k], c->ev_end[(f - 1) % zr_ctx::END_RING], c->ev_end[f % zr_ctx::END_RING]);
        }
        return (int)n;
    });
}

// Per-pass hipEvents are recorded on every interval-th frame (default 1 = every frame, 0 = never).  Each record is a small
// bubble on the render stream (~6 us on MI355X, six per frame), so a host that only wants throughput samples sparsely.
extern "C" int zr_set_timing_interval(zr_ctx* c, uint32_t interval)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->timing_interval = interval;
        return ZR_OK;
    });
}

extern "C" uint32_t zr_abi_version(void) { return ZR_ABI_VERSION; }

// `bytes` = sizeof(zr_stats) as the CALLER was compiled: the struct only ever grows at its end, so a host built against an older header
// gets the fields it knows and is never written past.
extern "C" int zr_get_stats(zr_ctx* c, zr_stats* out_user, size_t bytes)
{
    if (!c || !out_user) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes >= offsetof(zr_stats, round1_survivors) && bytes % 4 == 0);      // (the first release's struct ended there)
        zr_stats out_full; zr_stats* out = &out_full;
        int rc = zr_finish(c);
        if (c->rendered && (rc == ZR_OK || rc == ZR_ERR_OVERFLOW)) {      // shadow coverage is a statistic, counted on demand
            ZrDevStats z; (void)hipMemcpy(&z, c->d_stats, sizeof z, hipMemcpyDeviceToHost);
            uint32_t zero = 0;
            (void)hipMemcpy(&c->d_stats->covered_shadow, &zero, 4, hipMemcpyHostToDevice);
            zr_launch_count_shadow((const uint32_t*)shadow_buf(c), (size_t)c->SD * c->SD, c->d_stats, c->stream);
            (void)hipStreamSynchronize(c->stream);
            // (the count is the one word of the block that changed since zr_finish read it and merged the shadow pipeline's into it)
            (void)hipMemcpy(&c->h_stats.covered_shadow, &c->d_stats->covered_shadow, 4, hipMemcpyDeviceToHost);
        }
#ifdef ZR_DIAG
        if (getenv("ZR_DUMP_STATS")) {     // diagnostics: the raw device block
            const ZrDevStats& h = c->h_stats;
            fprintf(stderr, "zr stats: survivors %u %u %u  bin_entries %u %u %u  n_sel %u %u %u  n_slow %u %u %u  hiz_culled %u  n_chunks %u %u %u  overflow records %u %u\n",
                    h.survivors[0], h.survivors[1], h.survivors[2], h.bin_entries[0], h.bin_entries[1], h.bin_entries[2], h.n_sel[0], h.n_sel[1], h.n_sel[2],
                    h.n_slow[0], h.n_slow[1], h.n_slow[2], h.hiz_culled, h.n_chunks[0], h.n_chunks[1], h.n_chunks[2], h.pool_used[1], h.pool_used[2]);
        }
#endif
        memset(out, 0, sizeof *out);
        for (int i = 0; i < 2; ++i) {
            out->work_items[i] = c->last_work[i]; out->survivors[i] = c->h_stats.survivors[i]; out->bin_entries[i] = c->h_stats.bin_entries[i];
        }
        out->survivors[1] += c->h_stats.survivors[2]; out->bin_entries[1] += c->h_stats.bin_entries[2];    // both rounds of the camera pass
        out->hiz_culled = c->h_stats.hiz_culled; out->round1_survivors = c->last_two_round ? c->h_stats.survivors[1] : 0;
        out->covered_pixels = 0; for (uint32_t v : c->h_stats.covered_part) out->covered_pixels += v;
        out->covered_shadow_texels = c->h_stats.covered_shadow; out->overflow = c->h_stats.overflow;
        out->shadow_occluded = c->h_stats.shadow_occluded; out->shadow_late = c->h_stats.shadow_late;
        out->hiz_culled_geom = c->h_stats.hiz_culled_geom; out->struct_bytes = (uint32_t)sizeof(zr_stats);
        memcpy(out_user, out, std::min(bytes, sizeof(zr_stats)));
        return rc;
    });
}

// ------------------------------------------------------------------------------------------------ read-back

extern "C" int zr_read_color(zr_ctx* c, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && bytes == (size_t)c->W * c->H * 4);
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, c->d_color, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
extern "C" int zr_read_gbuffer(zr_ctx* c, int target, void* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const GBufferPtrs& G = c->fc[c->fcur].G;
        const void* src[6] = { G.depth, G.scene_color, G.gA, G.gB, G.gC, G.gD };
        ARGCHK(c, dst && target >= 0 && target < 6);
        ARGCHK(c, bytes == (size_t)c->W * c->H * (target == 5 ? 8 : 4));
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, src[target], bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
extern "C" int zr_read_shadowmap(zr_ctx* c, float* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && bytes == (size_t)c->SD * c->SD * 4);
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, shadow_buf(c), bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}

// The frame enqueued last, copied into caller-owned DEVICE buffers in stream order (no host synchronisation): what a host with two frames
// in flight uses instead of zr_read_color - the copies are ordered behind that frame's lighting pass and ahead of whatever the next
// zr_render enqueues on the render stream.  Either pointer may be NULL.  (The shadow map is double-buffered inside: the NEXT frame's
// shadow pipeline draws into the other copy, so the map copied here is this frame's whatever runs beside it.)
extern "C" int zr_copy_frame_async(zr_ctx* c, void* color_dev, void* shadow_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered || c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_copy_frame_async: no finished frame enqueued");
        HIPCHK(c, hipSetDevice(c->device));
        if (color_dev) HIPCHK(c, hipMemcpyAsync(color_dev, c->d_color, (size_t)c->W * c->H * 4, hipMemcpyDeviceToDevice, c->stream));
        if (shadow_dev) HIPCHK(c, hipMemcpyAsync(shadow_dev, shadow_buf(c), (size_t)c->SD * c->SD * 4, hipMemcpyDeviceToDevice, c->stream));
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ object identity (zelda_render.h)

extern "C" int zr_set_id_capture(zr_ctx* c, int enable)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_set_id_capture between the stages of a frame");
        const bool on = enable != 0;
        if (on == c->id_capture) return ZR_OK;
        HIPCHK(c, hipSetDevice(c->device));
        const int rc = set_winner_planes(c, c->shading == ZR_SHADING_FORWARD, on, "zr_set_id_capture");      // (no drain: frames in flight keep what they were enqueued with)
        if (rc) return rc;
        c->id_capture = on;
        return ZR_OK;
    });
}

// The frame enqueued last kept its winners and still describes the scene; `sync`: finish it first (its overflow is the query's error).
static int ids_ready(zr_ctx* c, const char* what, bool sync)
{
    if (!c->rendered || c->stage != 0) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": no finished frame enqueued");
    if (!c->ids_frame) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": the last frame was rendered without id capture (zr_set_id_capture)");
    if (c->ids_gen != c->scene_gen) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": the scene changed after the last frame");
    HIPCHK(c, hipSetDevice(c->device));
    return sync ? zr_finish(c) : ZR_OK;
}
static ZrIdsArgs ids_args(zr_ctx* c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
    const FrameCopy& F = c->fc[c->fcur];                      // (stage 0: the copy the frame enqueued last wrote)
    ZrIdsArgs A; memset(&A, 0, sizeof A);
    A.prim = F.prim_plane; A.depth = F.G.depth;
    A.draws = c->d_ids_draws; A.n_draws = c->ids_n_draws;
    A.W = c->W; A.x0 = x0; A.y0 = y0; A.w = w; A.h = h;
    A.counts = c->d_ids_counts; A.keys = c->d_ids_keys; A.hit_list = c->d_ids_list; A.n_hits = c->d_ids_n;
    return A;
}

extern "C" int zr_read_ids(zr_ctx* c, int kind, void* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && (kind == ZR_IDS_PRIMITIVE || kind == ZR_IDS_OBJECT));
        ARGCHK(c, bytes == (size_t)c->W * c->H * (kind == ZR_IDS_OBJECT ? 8 : 4));
        int rc = ids_ready(c, "zr_read_ids", true);
        if (rc) return rc;
        const ZrIdsArgs A0 = ids_args(c, 0, 0, c->W, c->H);
        if (kind == ZR_IDS_PRIMITIVE) { HIPCHK(c, hipMemcpy(dst, A0.prim, bytes, hipMemcpyDeviceToHost)); return ZR_OK; }
        if (!c->d_ids_obj) HIPCHK(c, c->own.alloc(&c->d_ids_obj, (size_t)c->W * c->H));
        ZrIdsArgs A = A0; A.obj_plane = c->d_ids_obj;
        zr_launch_id_census(A, ZR_IDS_OBJECTS, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(dst, c->d_ids_obj, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ZR_OK;
    });
}

extern "C" int zr_pick(zr_ctx* c, uint32_t x, uint32_t y, uint32_t w, uint32_t h, zr_hit* hits, uint32_t cap, uint32_t* n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, n && w > 0 && h > 0 && (hits || cap == 0));
        *n = 0;
        int rc = ids_ready(c, "zr_pick", true);
        if (rc) return rc;
        if (x >= c->W || y >= c->H) return ZR_OK;                  // wholly outside the frame
        ZrIdsArgs A = ids_args(c, x, y, std::min(w, c->W - x), std::min(h, c->H - y));
        zr_launch_id_census(A, ZR_IDS_PICK, c->stream);
        HIPCHK(c, hipGetLastError());
        uint32_t total = 0;
        HIPCHK(c, hipMemcpyAsync(&total, c->d_ids_n, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (total > c->ids_n_slots) return zr_fail(c, ZR_ERR_DEVICE, "zr_pick: hit list longer than the slot count");
        std::vector<zr_hit> all(total);
        zr_launch_id_hits(A, total, c->d_ids_hits, c->stream);       // (also clears the listed slots)
        HIPCHK(c, hipGetLastError());
        if (total) HIPCHK(c, hipMemcpyAsync(all.data(), c->d_ids_hits, sizeof(zr_hit) * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ids_n, 0, 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::sort(all.begin(), all.end(), [](const zr_hit& a, const zr_hit& b) {
            if (a.depth != b.depth) return a.depth < b.depth;
            if (a.object != b.object) return a.object < b.object;
            return a.instance < b.instance;
        });
        if (total) memcpy(hits, all.data(), sizeof(zr_hit) * std::min(total, cap));
        *n = total;
        return ZR_OK;
    });
}

static size_t ids_slot_bytes(const zr_ctx* c)
{
    size_t slots = 0;
    for (const auto& o : c->objects) slots += o.n_inst;      // (n_inst = max(1, instances))
    return 4 * slots;
}
// The whole-frame census into a count array on the device (cleared first), on the host's stream.
static int ids_coverage(zr_ctx* c, uint32_t* counts_dev, size_t bytes)
{
    if (bytes) HIPCHK(c, hipMemsetAsync(counts_dev, 0, bytes, c->stream));
    ZrIdsArgs A = ids_args(c, 0, 0, c->W, c->H);
    A.counts = counts_dev;
    if (bytes) zr_launch_id_census(A, ZR_IDS_COVERAGE, c->stream);
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}
extern "C" int zr_instance_coverage(zr_ctx* c, uint32_t* counts, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (counts || bytes == 0) && bytes == ids_slot_bytes(c));
        int rc = ids_ready(c, "zr_instance_coverage", true);
        if (rc == ZR_OK) rc = ids_coverage(c, c->d_ids_cov, bytes);
        if (rc) return rc;
        if (bytes) HIPCHK(c, hipMemcpyAsync(counts, c->d_ids_cov, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ZR_OK;
    });
}
extern "C" int zr_instance_coverage_async(zr_ctx* c, void* counts_dev, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (counts_dev || bytes == 0) && bytes == ids_slot_bytes(c));
        int rc = ids_ready(c, "zr_instance_coverage_async", false);
        if (rc == ZR_OK) rc = ids_coverage(c, (uint32_t*)counts_dev, bytes);
        if (rc) return rc;
        // the census reads the last frame's winner plane: the frame that writes that copy next (the one after next) waits for it
        HIPCHK(c, hipEventRecord(c->fc[c->fcur].ev_ids, c->stream));
        c->fc[c->fcur].ids_wait = true;
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ multi-GPU tiles

extern "C" int zr_tiles_device_buffer(zr_ctx* c, void** p, size_t* bytes)
{
    if (!c || !p || !bytes) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        *p = c->d_tiles; *bytes = (size_t)c->slots_per_rank * ZR_TILE * ZR_TILE * 4;
        return ZR_OK;
    });
}
// Lets the caller own the packed tile buffer (e.g. a torch tensor handed to RCCL; two of them alternate so that frame k's
// all-gather overlaps frame k+1's rendering).  ptr must hold zr_tiles_device_buffer's byte count; NULL = internal buffer.
extern "C" int zr_set_tiles_buffer(zr_ctx* c, void* ptr)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->d_tiles_ext = (uint32_t*)ptr;
        return ZR_OK;
    });
}

extern "C" int zr_read_tiles(zr_ctx* c, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && bytes == (size_t)c->slots_per_rank * ZR_TILE * ZR_TILE * 4);
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, c->d_tiles_ext ? c->d_tiles_ext : c->d_tiles, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
extern "C" int zr_composite(zr_ctx* c, const void* gathered)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, gathered != nullptr);
        HIPCHK(c, hipSetDevice(c->device));
        zr_launch_untile((const uint32_t*)gathered, c->d_tile_map, c->d_color, c->W, c->H, c->tiles_x, c->n_tiles, c->stream);
        HIPCHK(c, hipGetLastError());
        return ZR_OK;
    });
}
extern "C" int zr_color_device_ptr(zr_ctx* c, void** p) { if (!c || !p) return ZR_ERR_ARG; return zr_guard(c, [&]() -> int { *p = c->d_color; return ZR_OK; }); }
