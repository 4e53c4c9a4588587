// zr_resize.cpp — the frame's extent behind the C-ABI (zelda_render.h, "lifetime"): everything of a context that is sized by W, H or a
// tile count, made as one set (make_extent_state) by zr_create and again by zr_resize, and zr_get_extent.
//
// Host counterpart of RecreateSwapChain (ZE:2311-2330): the per-extent images are re-made, the scene stays where it is.  A resize builds
// the new set beside the old one, through an owner of its own, and swaps the two only when everything is there: a resize that runs out of
// memory leaves the context rendering at its old extent ("Resizing", has the peak this costs and the list of every
// pointer the swap replaces).  No kernel is launched here but the fill of the new key buffers.
#include "zr_ctx.h"

#include <cstring>

namespace {

// One extent's set.  The fields are the context's of the same names; `mem` owns the device memory behind the pointers, `pool_mem` the work
// pools' per-tile parts (made only where the context has work pools; else make_work_pools makes them for the extent it then finds).
struct ZrExtentState {
    ZrOwn mem, pool_mem;
    uint32_t W = 0, H = 0, tiles_x = 0, tiles_y = 0, n_tiles = 0, n_owned = 0, slots_per_rank = 0;
    GBufferPtrs G[2] = {}; uint32_t* prim_plane[2] = { nullptr, nullptr };
    uint32_t *d_color = nullptr, *d_tiles = nullptr, *d_tile_map = nullptr, *d_owned = nullptr;
    unsigned long long* d_vis[2] = { nullptr, nullptr }; unsigned long long* d_sky_keys = nullptr;
    float* d_hiz = nullptr; ZrHiz hiz = {}; uint32_t* d_hiz_regions = nullptr; uint32_t n_hiz_regions = 0;
    uint32_t *tile_count = nullptr, *tile_offset = nullptr, *tile_cursor = nullptr, *chunk_offset = nullptr;      // zr_ctx::ShadowBins
    bool pools = false; ZrTriBins tb = {}; uint4* chunk_tab = nullptr; uint32_t chunk_capacity = 0;
};

bool extent_ok(uint32_t W, uint32_t H)
{
    if (W == 0 || H == 0 || W > 255u * ZR_TILE || H > 255u * ZR_TILE) return false;
    // binning histograms (4 B per tile, dynamic) + a few static words must fit the default 64 KB of LDS per workgroup
    return ((W + ZR_TILE - 1) / ZR_TILE) * ((H + ZR_TILE - 1) / ZR_TILE) <= 16000u;
}

// Reads the context (its partition, its map's tile count, which of the planes made at first use it has now), writes E only.
int make_extent_state(zr_ctx* c, uint32_t W, uint32_t H, ZrExtentState* Ep)
{
    ZrExtentState& E = *Ep;
    ZrOwn& A = E.mem;
    if (!extent_ok(W, H)) return zr_fail(c, ZR_ERR_ARG, "too many tiles");
    E.W = W; E.H = H;
    const size_t n = (size_t)W * H;
    for (int i = 0; i < 2; ++i) {       // two frames in flight: see zr_ctx.h
        GBufferPtrs& G = E.G[i];
        HIPCHK(c, A.alloc(&G.depth, n)); HIPCHK(c, A.alloc(&G.scene_color, n)); HIPCHK(c, A.alloc(&G.gA, n)); HIPCHK(c, A.alloc(&G.gB, n));
        HIPCHK(c, A.alloc(&G.gC, n)); HIPCHK(c, A.alloc(&G.gD, n)); HIPCHK(c, A.alloc(&G.overlay, n));
        // the winner planes while the resolve keeps them (set_winner_planes: every pixel "none"); else made at their next first use
        if (c->fc[i].G.prim) { HIPCHK(c, A.alloc(&E.prim_plane[i], n)); G.prim = E.prim_plane[i]; }
    }
    HIPCHK(c, A.alloc(&E.d_color, n));
    for (auto& v : E.d_vis) HIPCHK(c, A.alloc(&v, n));
    if (c->d_sky_keys) HIPCHK(c, A.alloc(&E.d_sky_keys, n));      // (k_sky_tiles writes every owned pixel before the resolve reads it)

    // screen tiles: camera target partitioned t % world == rank
    E.tiles_x = (W + ZR_TILE - 1) / ZR_TILE; E.tiles_y = (H + ZR_TILE - 1) / ZR_TILE; E.n_tiles = E.tiles_x * E.tiles_y;
    const ZrTilePartition tp = zr_partition(E.tiles_x, E.tiles_y, c->cfg.tile_world, c->cfg.tile_rank);
    E.slots_per_rank = tp.slots_per_rank; E.n_owned = (uint32_t)tp.owned.size();
    HIPCHK(c, upload(A, &E.d_tile_map, tp.map)); HIPCHK(c, upload(A, &E.d_owned, tp.owned));
    const size_t tile_words = (size_t)E.slots_per_rank * ZR_TILE * ZR_TILE;
    HIPCHK(c, A.alloc(&E.d_tiles, tile_words));
    const uint32_t mt = (E.n_tiles > c->sn_tiles ? E.n_tiles : c->sn_tiles) * ZR_TSTRIDE + 1;     // (the bins use the first sn_tiles + 1 words)
    HIPCHK(c, A.alloc(&E.tile_count, mt)); HIPCHK(c, A.alloc(&E.tile_offset, mt));
    HIPCHK(c, A.alloc(&E.tile_cursor, mt)); HIPCHK(c, A.alloc(&E.chunk_offset, mt));

    size_t hiz_texels = 0;
    {   // Hi-Z pyramid: level l = max depth per (8 << l)^2 pixel block
        for (int l = 0; l < 4; ++l) { E.hiz.hw[l] = (W + (8u << l) - 1) / (8u << l); E.hiz.hh[l] = (H + (8u << l) - 1) / (8u << l); hiz_texels += (size_t)E.hiz.hw[l] * E.hiz.hh[l]; }
        E.hiz.fw = (W + 3u) / 4u; E.hiz.fh = (H + 3u) / 4u;
        hiz_texels += (size_t)E.hiz.fw * E.hiz.fh;
        HIPCHK(c, A.alloc(&E.d_hiz, hiz_texels));
        static_assert(ZR_TILE == 32 && ZR_SUPERTILE_SHIFT >= 1, "a 64 x 64 region of the pyramid must lie inside one super-tile");
        std::vector<uint32_t> regions;
        for (uint32_t ry = 0; ry < (H + 63u) / 64u; ++ry)
            for (uint32_t rx = 0; rx < (W + 63u) / 64u; ++rx)
                if (zr_tile_owner(rx * 2u, ry * 2u, c->cfg.tile_world) == c->cfg.tile_rank) regions.push_back(rx | ry << 16);
        E.n_hiz_regions = (uint32_t)regions.size();
        HIPCHK(c, upload(A, &E.d_hiz_regions, regions));
        float* p = E.d_hiz;
        for (int l = 0; l < 4; ++l) { E.hiz.lvl[l] = p; p += (size_t)E.hiz.hw[l] * E.hiz.hh[l]; }
        E.hiz.fine = p;
    }
    HIPCHK(c, zr_fill_sync({ { E.G[0].overlay, 0, n * 4 }, { E.G[1].overlay, 0, n * 4 }, { E.d_color, 0, n * 4 },
                             { E.d_tiles, 0, tile_words * 4 },
                             { E.tile_count, 0, (size_t)mt * 4 },       // k_bin_count counts into zeroes (k_scan zeroes the counts
                             { E.tile_cursor, 0, (size_t)mt * 4 },      // and the cursors again for the fill and the next frame)
                             { E.d_hiz, 0, hiz_texels * sizeof(float) } }));      // texels over other ranks' regions stay 0 ("hidden")
    for (uint32_t* p : E.prim_plane) if (p) HIPCHK(c, zr_fill_sync({ { p, 0xFF, n * 4 } }));
    // both key buffers hold the empty key between frames (the resolve resets what it reads)
    for (auto& v : E.d_vis) zr_launch_fill64(v, ZR_EMPTY_KEY, n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));

    if (c->work_capacity != 0) {        // the work pools' per-tile parts, beside the pools themselves
        E.tb = c->tb;
        if (int rc = zr_make_pool_tiles(c, E.pool_mem, E.n_tiles, &E.tb, &E.chunk_tab, &E.chunk_capacity)) return rc;
        E.pools = true;
    }
    return ZR_OK;
}

// The swap.  Nothing here can fail.  Every pointer into the old set is replaced or dropped to "made at first use" before the old owner
// releases it; the kernel-argument blocks that hold such pointers are c->tb, c->hiz and FrameCopy::G (assigned here), c->pass[] (built by
// every frame_begin) and c->resolve_P (written by the gbuffer_pass of the frame whose lighting call reads it) - both cleared here all the
// same; c->Gclear points at the context's one clear pixel and stays.
void commit_extent_state(zr_ctx* c, ZrExtentState& E)
{
    c->W = c->cfg.width = E.W; c->H = c->cfg.height = E.H;
    c->tiles_x = E.tiles_x; c->tiles_y = E.tiles_y; c->n_tiles = E.n_tiles; c->n_owned = E.n_owned; c->slots_per_rank = E.slots_per_rank;
    for (int i = 0; i < 2; ++i) { c->fc[i].G = E.G[i]; c->fc[i].prim_plane = E.prim_plane[i]; c->d_vis[i] = E.d_vis[i]; }
    c->d_color = E.d_color; c->d_tiles = E.d_tiles; c->d_tile_map = E.d_tile_map; c->d_owned = E.d_owned; c->d_sky_keys = E.d_sky_keys;
    c->d_hiz = E.d_hiz; c->hiz = E.hiz; c->d_hiz_regions = E.d_hiz_regions; c->n_hiz_regions = E.n_hiz_regions;
    c->sb.tile_count = E.tile_count; c->sb.tile_offset = E.tile_offset; c->sb.tile_cursor = E.tile_cursor; c->sb.chunk_offset = E.chunk_offset;
    // made at first use, through c->ext: the next use makes them for the new extent
    c->lk.plane = nullptr; c->lk.rest = nullptr; c->lk.alloc_failed = false;
    c->lk.marks = nullptr; c->lk.handed_out = false; zr_settle_forget(&c->lk.settle);      // (the frame's address is void with the old set)
    c->d_scaled = nullptr; c->ids.obj = nullptr; c->hl.plane = nullptr; c->hl.frame = nullptr; c->ov.frame = nullptr; c->wire.frame = nullptr;
    c->d_tiles_ext = nullptr;            // (sized by the old slots_per_rank: back to the internal buffer)
    memset(&c->resolve_P, 0, sizeof c->resolve_P); memset(c->pass, 0, sizeof c->pass); c->pass_live[0] = c->pass_live[1] = false;
    if (E.pools) {
        c->tb = E.tb; c->sb.chunk_tab = E.chunk_tab; c->chunk_capacity = E.chunk_capacity;
        c->pool_tiles = std::move(E.pool_mem);
    }
    c->ext = std::move(E.mem);           // (releases the old set)
}

}  // namespace

int zr_extent_create(zr_ctx* c)
{
    ZrExtentState E;
    if (int rc = make_extent_state(c, c->W, c->H, &E)) return rc;
    commit_extent_state(c, E);
    return ZR_OK;
}

// Replaces RecreateSwapChain (ZE:2311-2330, reached from ZE:1973-1976).
extern "C" int zr_resize(zr_ctx* c, uint32_t width, uint32_t height)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!extent_ok(width, height)) return zr_fail(c, ZR_ERR_ARG, "zr_resize: a zero extent, one beyond 255 tiles a side, or more than 16000 tiles");
        if (int rc = zr_stage_idle(c, "zr_resize")) return rc;
        if (c->dist) return zr_fail(c, ZR_ERR_UNSUPPORTED, "zr_resize: the native multi-GPU host is attached (its buffers are sized at zr_dist_prepare)");
        if (width == c->W && height == c->H) return ZR_OK;      // nothing happens: no synchronisation, no rest ends
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));       // as the reference waits for the device: nothing in flight reads the old set after this
        // the new set first, beside the old one; a failure from here to the swap leaves the context as it was
        ZrExtentState E;
        ZrDeltaBuffers D;
        int rc = make_extent_state(c, width, height, &E);
        if (rc == ZR_OK && c->delta.on) rc = zr_delta_make(c, width, height, c->delta.b.codec.on, &D);
        if (rc) { (void)hipGetLastError(); return rc; }
        commit_extent_state(c, E);
        if (c->delta.on) { c->delta.b = std::move(D); c->delta.full = true; }      // (the old buffers are released; serial goes on counting)
        // Every per-pixel history is forgotten: both GBuffer copies, the camera pass of the frame before and its round-2 keep, the record
        // plan, the camera's work list (a rank's is cut to its tiles), the visibility marks (the next frame draws in one round, as a
        // scene's first frame does), the lighting pass's plane - its key does not hold the extent.  The shadow map, its work list and its
        // occlusion flags stand: a resize is a camera change, not a caster change.
        for (FrameCopy& F : c->fc) { F.g_gen = 0; F.overlay_dirty = false; F.ids_wait = false; }
        zr_history_forgotten(c, ZR_HIST_CAMERA_LIST | ZR_HIST_PLAN | ZR_HIST_VISIBILITY | ZR_HIST_LIGHT_PLANE);
        c->carry.cam_prev_valid = c->carry.r2_settled = c->carry.plan_two_round = c->carry.plan_behind_cam = false;
        memset(&c->cam_prev_key, 0, sizeof c->cam_prev_key); memset(&c->list_key[1], 0, sizeof c->list_key[1]);
        zr_camera_changed(c);
        // until the next frame the read-backs, the identity queries and the deliveries answer as on a context that has rendered no frame
        c->rendered = false; c->ids_frame = false; c->last_two_round = false; c->empty_ready = false;
        c->cov_block = c->d_stats; c->last_work[1] = 0; c->h_stats = ZrDevStats{};
        if (c->lens.valid) zr_uniforms_reproject(c);      // uniforms of zr_set_frame stay as given; uniforms never set stay unset
        // the pools' few words of plan state that are no tile's, as a scene's first frame finds them (the per-tile ones are new and zeroed)
        if (E.pools) HIPCHK(c, zr_pool_plan_reset(c));
        return ZR_OK;
    });
}

extern "C" int zr_get_extent(zr_ctx* c, uint32_t* width, uint32_t* height)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (width) *width = c->W;
        if (height) *height = c->H;
        return ZR_OK;
    });
}
