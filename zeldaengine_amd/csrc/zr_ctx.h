// zr_ctx.h — the internal context and the helpers that the host's translation units share ("Where the host code lives").
#pragma once

#include <atomic>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "zr_frame_end.h"
#include "zr_frame_plan.h"
#include "zr_ids.h"
#include "zr_meshlet.h"
#include "zr_overlay.h"
#include "zr_scale.h"
#include "zr_settle.h"
#include "zr_timed.h"
#include "zr_types.h"
#include "zr_world_doc.h"

// The owner of one lifetime's HIP resources: device memory, pinned host memory, events and streams are made through it, and it frees
// what it made, newest first, on release() and when it is destroyed.  The kernel-argument structs keep their raw pointers: views into
// owned memory.  (Hidden: no exported symbol.)
class __attribute__((visibility("hidden"))) ZrOwn {
public:
    ZrOwn() = default;
    ZrOwn(ZrOwn&& o) noexcept : items_(std::move(o.items_)) { o.items_.clear(); }
    ZrOwn& operator=(ZrOwn&& o) noexcept { if (this != &o) { release(); items_.swap(o.items_); } return *this; }
    ~ZrOwn() { release(); }

    template <typename T> hipError_t alloc(T** p, size_t n) { return keep(Dev, p, room() ? hipMalloc((void**)p, (n ? n : 1) * sizeof(T)) : hipErrorOutOfMemory); }
    // Images that kernels gather from at random (material textures, skydome, background): allocated in whole 2 MiB units, so that the
    // driver maps them with large page fragments whatever the allocator's pools look like at the time - a 1.4 MiB texture that lands
    // in 4 KiB-mapped memory costs the sampled resolve a third of its speed (seen as two modes of `value_textured`, run to run).
    hipError_t alloc_image(uint8_t** p, size_t bytes) { return alloc(p, (bytes + (2u << 20) - 1) / (2u << 20) * (2u << 20)); }
    template <typename T> hipError_t host(T** p, size_t n) { return keep(Host, p, room() ? hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault) : hipErrorOutOfMemory); }
    hipError_t event(hipEvent_t* e, unsigned flags = hipEventDefault) { return keep(Event, e, room() ? hipEventCreateWithFlags(e, flags) : hipErrorOutOfMemory); }
    hipError_t stream(hipStream_t* s) { return keep(Stream, s, room() ? hipStreamCreateWithFlags(s, hipStreamNonBlocking) : hipErrorOutOfMemory); }
    hipError_t stream(hipStream_t* s, int priority) { return keep(Stream, s, room() ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority) : hipErrorOutOfMemory); }
    void adopt(ZrOwn&& o) { items_.insert(items_.end(), o.items_.begin(), o.items_.end()); o.items_.clear(); }      // o's, released before ours
    void release() noexcept
    {
        for (auto it = items_.rbegin(); it != items_.rend(); ++it)
            switch (it->kind) {
            case Dev: (void)hipFree(it->p); break;
            case Host: (void)hipHostFree(it->p); break;
            case Event: (void)hipEventDestroy((hipEvent_t)it->p); break;
            case Stream: (void)hipStreamDestroy((hipStream_t)it->p); break;
            }
        items_.clear();
    }

private:
    enum Kind : uint8_t { Dev, Host, Event, Stream };
    struct Item { Kind kind; void* p; };
    std::vector<Item> items_;
    bool room() noexcept             // a place for the next record, made before the resource: keeping it cannot throw
    {
        if (items_.size() < items_.capacity()) return true;
        try { items_.reserve(2 * items_.size() + 16); return true; } catch (...) { return false; }
    }
    template <typename H> hipError_t keep(Kind k, H* h, hipError_t e) noexcept { if (e == hipSuccess && *h) items_.push_back({ k, (void*)*h }); return e; }
};

// hipMemset of device memory is ordered on the NULL stream and need not be complete when it returns; the library's streams are
// non-blocking ones (no implicit ordering with the null stream): the fills are through before this returns, so before anything that
// follows is enqueued on them.
struct ZrFill { void* p; int value; size_t bytes; };
static inline hipError_t zr_fill_sync(std::initializer_list<ZrFill> fills)
{
    for (const ZrFill& f : fills) {
        const hipError_t e = hipMemset(f.p, f.value, f.bytes);
        if (e != hipSuccess) return e;
    }
    return hipDeviceSynchronize();
}

template <typename T> static hipError_t upload(ZrOwn& own, T** d, const std::vector<T>& h)
{
    hipError_t e = own.alloc(d, h.size());
    if (e != hipSuccess) return e;
    return h.empty() ? hipSuccess : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

struct ZrMesh {
    ZrOwn mem;                           // the device buffers below (made by upload_mesh)
    std::vector<XkVertex> v;
    std::vector<uint32_t> idx;           // draw-order index buffer
    ZrMeshletSet ms;
    bool has_meshlets = false, uploaded = false;
    float center[3] = { 0, 0, 0 }; float radius = 0;
    XkVertex* d_v = nullptr; ZrRVertex* d_rv = nullptr; ZrRVertex* d_rt = nullptr; uint32_t* d_idx = nullptr; XkMeshlet* d_meshlets = nullptr;
    float4* d_mpos = nullptr; float4* d_mbox = nullptr; uint2* d_mtri = nullptr; uint32_t* d_tri_meshlet = nullptr;
    // Vertex updates (zr_mesh_update_host.cpp), set up at the mesh's first update: upd.set[0] = the buffers above, set[1] their parity-1
    // twins, upd.raw what the update calls write.  stale[p]: set p is older than raw (the next frame of parity p refits it);
    // v_stale = a device-form update came after `v`; ml_stale = ms.meshlets' bounds are not yet the device's of the current vertices.
    ZrMeshState upd = {}; bool stale[2] = { false, false }, v_stale = false, ml_stale = false;
};

// Host form of one material: per slot either a constant texel or an RGBA8 image (mips are built at zr_object_add).
struct ZrMaterialHost {
    uint32_t texel[7]; float bc_linear[3];
    std::vector<uint8_t> image[7];       // empty: the slot is constant
    uint32_t w[7], h[7];
};

struct ZrSceneObject {
    ZrOwn mem;                           // the device memory below: instance records, raw values, update state
    ZrOwn tex_mem;                       // ... and the material's images (d_tex[]): an owner of their own, so that a world update can
                                         // re-make an object's instance buffers and keep its material where it is
    uint32_t mesh = 0, n_inst = 1; bool instanced = false;
    std::vector<XkInstanceData> inst;    // host copy (zr_object_get_instances)
    ZrInstance* d_inst = nullptr;        // the instance records: what every frame reads until an update, then the parity-0 plane
    XkInstanceData* d_raw = nullptr;     // instanced objects: the raw values on the device (written only by the update calls)
    // Instance updates (zr_instances_host.cpp), set up at the object's first update: upd.plane[0] = d_inst, plane[1] its parity-1 twin.
    // pending[p]: an upper bound of list p's length on the device; tab1 = the parity-1 draw table points at plane[1];
    // host_stale = a device-form update came after `inst` (zr_object_get_instances reads back); draw = the record in the draw table.
    ZrInstanceState upd = {}; uint32_t pending[2] = { 0, 0 }; bool tab1 = false, host_stale = false; uint32_t draw = 0;
    // Visibility (zr_instances_host.cpp): hidden = the whole object (ZR_OBJ_HIDDEN in the draw record), flag_pending[p] = the parity-p
    // table does not hold it yet; vis = the host copy of upd.vis (empty: never touched, every instance shown), vis_stale = a device-form
    // update came after it (zr_object_get_visibility reads back).
    bool hidden = false, flag_pending[2] = { false, false }, vis_stale = false;
    std::vector<uint8_t> vis;
    uint32_t texel[7]; float bc_linear[3];
    uint8_t* d_tex[8] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };   // [7]: the packed material (ZrObject::packed)
    uint32_t tex_w[8] = { 0 }, tex_h[8] = { 0 }, tex_levels[8] = { 0 };
    bool mixed_sizes = false;            // image slots of different sizes: no packed form
    // Where a world load or update made the object from (zr_world.cpp: the matching rules of zr_world_update_json): the Profab's name and
    // the model's index in its list; mat_pristine = the material is still as the Profab gave it (zr_object_set_texture and
    // zr_object_update_texture_async clear it).  Objects of zr_object_add have from_world = false.
    std::string profab; uint32_t profab_model = 0; bool from_world = false, mat_pristine = false;
    // The work-item numbers the frame loop's history (d_visflag, d_sflag) knows the object's meshlet-instances by: written by
    // zr_scene_finalize, read by the next one that carries the history (work_valid: there are some).
    uint32_t work_base = 0, work_inst = 0, work_meshlets = 0; bool work_valid = false;
};

// First byte and channel count of each material slot in the packed texel (ZR_PK_*): the scene upload packs by it, a texture update rewrites by it.
static const struct { uint32_t ch, n; } kSlotPack[7] = { { ZR_PK_BC, 3 }, { ZR_PK_ME, 1 }, { ZR_PK_RO, 1 }, { ZR_PK_NO, 3 }, { ZR_PK_AO, 1 }, { ZR_PK_EM, 3 }, { ZR_PK_MS, 1 } };
// A mip chain (RHIGenerateMipmaps, ZE:6348-6433): every level half the one before, never below 1; level `level` of a w x h chain and the
// texels ahead of it (the levels lie one behind the other).
static inline uint32_t zr_mip_next(uint32_t d) { return d > 1 ? d >> 1 : 1; }
struct ZrMipLevel { uint32_t w, h; size_t off; };
static inline ZrMipLevel zr_mip_level(uint32_t w, uint32_t h, uint32_t level)
{
    ZrMipLevel L = { w, h, 0 };
    for (uint32_t l = 0; l < level; ++l) { L.off += (size_t)L.w * L.h; L.w = zr_mip_next(L.w); L.h = zr_mip_next(L.h); }
    return L;
}

struct ZrProfab { uint32_t mesh; ZrMaterialHost mat; };

// Two frames in flight (the reference does: MAX_FRAMES_IN_FLIGHT, ZE:77): what a lighting pass reads is double-buffered, and this is one
// copy of it.  Frame N uses copy N & 1 (zr_ctx::fcur, set at frame begin, so the read-back entry points see the frame rendered last) -
// of everything but the shadow map: which copy holds the current map is zr_ctx::smap, and it changes only when a shadow pass is drawn.
struct FrameCopy {
    GBufferPtrs G = {};                  // G.prim: the winner plane below, while the resolve keeps it (forward variant, id capture), else null
    float* shadow = nullptr; XkView* view = nullptr;
    uint32_t* empty_rgba = nullptr;      // the colour the lighting shader gives a pixel that holds every target's clear value, this frame
    uint32_t* prim_plane = nullptr;      // winner ids (zr_set_shading, zr_set_id_capture), made on first use
    bool overlay_dirty = false;          // G.overlay may hold skydome pixels of an earlier frame
    bool shadow_cleared = false;         // `shadow` already holds depth 1.0 (cleared by a lighting pass since it was last drawn into)
    uint64_t view_uploaded = 0;          // which version of the uniforms `view` holds
    uint64_t g_gen = 0;                  // the run of equal inputs (ZrFramePlan::g_gen) G was last resolved in (0: never)
    // a reader of this copy enqueued on the render stream - a census or a highlight's mask (the winner plane), an overlay (G.depth): the
    // frame that writes it next waits for it
    hipEvent_t ev_ids = nullptr; bool ids_wait = false;
};

// The buffers of the deliveries of changes, through owners of their own.  delivered = what the client holds; flags = a byte per tile,
// rewritten by every delivery (nothing to clear on the stream); packed / list / header = the host form's device buffers, h_header its
// pinned landing place; scaled = the filtered frame (delta scale above 1).  codec: what ZR_FRAME_DELTA_PACKED adds, through codec_mem -
// lens = a listed tile's record length, rewritten by every packed delivery; header / offsets / stream / h_header = the packed host
// form's buffers (it shares `list`).  Going between the raw and the packed forms makes or releases these alone.
struct ZrDeltaBuffers {
    ZrOwn mem, codec_mem;
    uint32_t *delivered = nullptr, *list = nullptr, *header = nullptr, *scaled = nullptr; uint8_t *packed = nullptr, *flags = nullptr;
    zr_frame_delta* h_header = nullptr;
    struct Codec {
        bool on = false; uint16_t* lens = nullptr; uint32_t *header = nullptr, *offsets = nullptr; uint8_t* stream = nullptr;
        zr_frame_delta_packed* h_header = nullptr;
    } codec;
};

// Every HIP resource of the context is made through the owner of its lifetime: `own` (the context: what zr_create makes, its streams
// first, and what later calls add for good), then one owner per group that is re-made or dropped as a whole (work pools, draw tables,
// ids, skydome, background, cubemap, shadow tiles; the scene's in its meshes and objects; each staging slot).  `own` is declared first,
// so zr_destroy's `delete` releases it last, after every other owner - and its streams last of all.
// `ext` owns what is sized by the frame's extent (W, H, a tile count) - what make_extent_state makes (zr_resize.cpp: the GBuffer copies,
// the key buffers, d_color, the Hi-Z pyramid, the tile tables, d_tiles, the shadow bins' per-tile arrays) and what later calls make at
// first use (winner planes, the skydome's key plane, the light-keep plane and its records, d_scaled, ids.obj, the highlight's plane and
// frame, the overlay's frame).  zr_resize builds a new set beside it and swaps the two.  `pool_tiles` owns the work pools' per-tile parts (make_pool_tiles).
struct zr_ctx {
    ZrOwn own, ext, pool_tiles;
    zr_config cfg;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;

    std::vector<ZrMesh> meshes;
    std::vector<ZrSceneObject> objects;
    bool scene_dirty = true;
    ZrObject* d_objs = nullptr; uint32_t n_objs = 0, n_work = 0;     // d_objs: the draw table of the frame enqueued last (an alias)
    // Draw tables: [0] made by zr_scene_finalize (every object's d_inst), [1] the parity-1 table, once an instance has been updated: it
    // differs only where an updated object points at its parity-1 plane.  A frame reads the table and the planes of its parity.
    ZrObject* d_objs_b[2] = { nullptr, nullptr }; ZrOwn tables;
    // What orders the between-frames updates against the frames in flight (zr_update.cpp; DESIGN.md §5, "Moving instances").
    struct Update {
        // Instance, visibility and vertex updates: reader[p] = 1 + the last frame that read the table / planes of parity p (0: none);
        // ev_scatter follows the last update (on scatter_s), ev_apply the last frame-head apply (on apply_s); a pinned staging ring for the
        // host form.  Made at the first update: a scene that never moves an instance has none of it.
        uint64_t reader[2] = { 0, 0 };
        hipEvent_t ev_scatter = nullptr, ev_apply = nullptr; hipStream_t scatter_s = nullptr, apply_s = nullptr;
        bool scatter_wait[2] = { false, false }, apply_done = false, dual = false;      // scatter_wait[p]: the next frame of parity p waits for ev_scatter; dual: two draw tables exist
        static constexpr int RING = 4;
        struct Stage { ZrOwn mem; uint8_t* h = nullptr; uint8_t* d = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; } ring[RING];      // cap: bytes
        uint32_t slot = 0;
        // Texture updates (zr_texture_update_host.cpp) rewrite a slot's mip chain and the packed material IN PLACE: ev_tex follows the last
        // one (on tex_s); an update waits for the end of the frame enqueued last, the next frame's first stream waits for ev_tex (tex_wait).
        // d_srgb_thr: the 256 sRGB encode thresholds (zr_srgb.h).  Made at the first update.
        hipEvent_t ev_tex = nullptr; hipStream_t tex_s = nullptr; bool tex_wait = false; float* d_srgb_thr = nullptr;
    } upd;
    // The frame schedule (zr_frame_plan.h): what the frame being enqueued does - decided once, at frame begin, from `facts`; the staged
    // entry points span three calls - and what the frames enqueued so far left behind.  The pass blocks the carry's validity bits speak
    // of live here: list_key[] = the block each pass's work list on the device was built from, smap_key = the block the current shadow
    // map was drawn from, cam_prev_key = the camera block of the frame enqueued last.
    ZrFrameFacts facts; ZrFramePlan plan; ZrFrameCarry carry;
    ZrPass list_key[2] = {}, smap_key = {}, cam_prev_key = {};
    // this frame's two geometry passes (0 shadow, 1 camera), built at frame begin
    ZrPass pass[2]; bool pass_live[2] = { false, false };
    // The epochs the keeps go by.  caster_epoch: bumped (zr_casters_changed) by every call that can change what the shadow pass would draw
    // or where - objects, instances, vertices, meshlets, limits, the map's buffer or partition, the host's stream.  camera_epoch: bumped
    // (zr_camera_changed, and with every zr_casters_changed: a caster is drawn by the camera too) by every call that can change what the
    // camera pass draws, its work numbering or its record layout.  surface_epoch: bumped (zr_surface_changed) by what the resolve reads
    // beyond that - every texture update, the winner planes coming or going.
    uint64_t caster_epoch = 0, camera_epoch = 0, surface_epoch = 0;
    // smap: the copy (fc[smap].shadow) that holds the current shadow map; a drawn pass targets the other one and flips it.  shadow_draws /
    // cam_draws: passes drawn so far (k_shadow_occlusion's retest turn, the visibility stamp's turn).
    int smap = 0; uint64_t shadow_draws = 0, cam_draws = 0;

    XkUniformBufferMVP cam, shadow; XkView view; bool frame_valid = false;
    // What of the last zr_update_uniforms depends on the extent - the camera's projection - as it was asked for (valid: no zr_set_frame
    // since): zr_resize evaluates it again for the new extent (zr_uniforms_reproject).
    struct Lens { bool valid = false; float fov = 0, zn = 0, zf = 0; } lens;
    uint32_t debug_view = 0;
    uint32_t shading = 0;                           // ZR_SHADING_*: which scene pipeline shades the frame (zr_set_shading)

    uint32_t W = 0, H = 0, SD = 0;
    uint32_t tiles_x = 0, tiles_y = 0, n_tiles = 0, n_owned = 0, slots_per_rank = 0;
    uint32_t stiles_x = 0, stiles_y = 0, sn_tiles = 0;
    uint32_t *d_owned = nullptr, *d_sowned = nullptr;
    uint32_t* d_tile_map = nullptr;      // tile -> owner * slots_per_rank + slot (k_untile)
    struct ZrDist* dist = nullptr;       // native multi-GPU host (zr_dist.cpp), or null
    uint32_t* d_color = nullptr; uint32_t* d_tiles = nullptr;
    float* d_shadow_ext = nullptr;       // caller-owned shadow map (zr_set_shadow_buffer), or null
    uint32_t shadow_rank = 0, shadow_world = 1; int stage = 0;   // stage: 0 idle, 1 shadow done, 2 gbuffer done
    // The shadow MAP owned by light-space super-tiles (zr_set_shadow_tiles): this context draws the casters that can reach a tile of the map
    // it owns; its owned tiles are exact, the others hold leftovers until zr_shadow_unpack scatters every rank's tiles in.
    uint32_t stile_rank = 0, stile_world = 1, s_slots_per_rank = 0, n_sowned_rank = 0;
    uint32_t *d_sowned_rank = nullptr, *d_stile_map = nullptr; ZrOwn stile_mem;
    uint32_t* d_tiles_ext = nullptr;     // caller-owned packed tile buffer for the next frames (zr_set_tiles_buffer), or null

    // The work pools, sized for work_capacity meshlet-instances by make_work_pools: sc, sb.bins, tb, d_pxrect, d_zmin, d_visflag,
    // d_spxrect, d_szmin, d_sflag - and through `pool_tiles` their per-tile parts: sb.chunk_tab, tb.tile_base / tile_cap / cursor /
    // r2_count / unit_tab
    ZrOwn pools;
    // the cull's output, one set per geometry pass (0 shadow, 1 camera) so that the two pipelines can run on two streams
    struct CullList { uint32_t *rects = nullptr, *work = nullptr; } sc[2];
    // the shadow pass's meshlet bins: per-tile counts, list offsets, fill cursors and work-unit offsets; the lists; the work units
    struct ShadowBins { uint32_t *tile_count = nullptr, *tile_offset = nullptr, *tile_cursor = nullptr, *chunk_offset = nullptr;
                        ZrBinEntry* bins = nullptr; uint4* chunk_tab = nullptr; } sb;
    uint32_t bucket_pct = 100;                              // zr_set_bucket_share: every planned bucket at that share of its size
    ZrTriBins tb = {};                    // triangle-binned camera pass: selection list, records (as emitted / in tile order), slow list
    uint32_t chunk_capacity = 0;         // raster work units the chunk table holds: bin_capacity / ZR_CHUNK + tiles
    uint32_t n_inst_total = 0;
    // one pixel holding the clear value of every GBuffer target; empty_ready: this frame's FrameCopy::empty_rgba has been computed
    uint8_t* d_clear_px = nullptr; GBufferPtrs Gclear = {}; bool empty_ready = false;
    // diagnostics read from the environment once, at zr_create, by -DZR_DIAG builds (never needed for a correct frame)
    uint32_t env_skip = 0, env_skip_light = 0; int32_t env_light_list_min = 4; bool env_no_empty_px = false;
    // XkView upload: a pageable-memory hipMemcpyAsync blocks the host until the stream has drained (~0.3 ms per frame here),
    // so the uniforms go through a small ring of pinned copies, and only when they changed
    static constexpr int VIEW_RING = kZrViewRing;
    XkView* h_view_ring = nullptr; hipEvent_t view_ev[VIEW_RING] = {}; uint32_t view_slot = 0; bool view_dirty = true;
    uint64_t view_version = 1;           // of the uniforms (FrameCopy::view_uploaded: the version a device copy holds)
    // Two frames in flight: the camera pipeline runs on `cam_s`, the shadow pipeline and the lighting pass on the host's `stream`;
    // frame N + 1's camera pipeline overlaps frame N's lighting.  What a lighting pass reads is therefore double-buffered: fc[fcur] is
    // the current frame's copy - at stage 0 the one the frame enqueued last wrote - and fc[fcur ^ 1] the next frame's.  (The shadow map's
    // two copies live in fc[] too, but are picked by `smap`, not by the frame's parity.)
    FrameCopy fc[2]; int fcur = 0;
    hipStream_t cam_s = nullptr;
    hipEvent_t ev_join = nullptr, ev_cam = nullptr;
    // A resolve left to the host's stream (ZrFramePlan::resolve_deferred): what it is launched with.  ev_lane: the lane's end, recorded
    // only where a frame waits for it (ZrFramePlan::wait_lane_end).
    ZrPass resolve_P; uint32_t resolve_mark = 0;
    hipEvent_t ev_lane = nullptr;
    unsigned long long* d_sky_keys = nullptr; uint32_t sky_object = 0;      // the skydome's key plane (k_sky_tiles) and its draw record
    // End of a frame's lighting pass, a ring of (timing-enabled) events: the next-but-one frame waits for it before it reuses the
    // double-buffered copies, and consecutive ones give the GPU's frame period (zr_get_frame_periods).  Recorded by every frame but those
    // inside a run of one-launch frames (zr_frame_end.h; `end`: which frame each slot holds, ZR_REST_END_EVERY): read through zr_frame_end().
    static constexpr int END_RING = kZrEndRing;
    hipEvent_t ev_end[END_RING] = {}; ZrEndState end;
    // The key buffer, one per frame parity like the FrameCopy resources (both hold the empty key between frames: the resolve resets what
    // it reads): frame N's rounds, Hi-Z build, k_mark and resolve use copy N & 1, so a resolve on the host's stream is not in the next
    // frame's way; the frame after that waits for ev_end[N] before it touches anything of this parity.
    unsigned long long* d_vis[2] = { nullptr, nullptr }; uint32_t raster_blocks = 2048, shadow_blocks = 2048;
    uint4* d_slow0 = nullptr; uint32_t slow0_cap = 1u << 18;      // shadow pass: triangles for the clipper (k_shadow_slow)
    uint32_t work_capacity = 0, bin_capacity = 0; bool any_images = false, mixed_images = false;
    uint32_t limit_record_chunks = 0, limit_slow_triangles = 0;      // zr_set_limits (0 = defaults)
    // two-pass Hi-Z occlusion culling of the camera pass: per work item pixel bbox + least depth (written by the cull),
    // visibility of the previous / current frame (one byte per meshlet-instance, marked by the resolve), the pyramid
    uint2* d_pxrect = nullptr; float* d_zmin = nullptr; uint8_t* d_visflag[2] = { nullptr, nullptr };
    // shadow pass occlusion culling (k_shadow_occlusion): the cull's box + least depth per work item, "not hidden last frame" per meshlet-instance
    uint2* d_spxrect = nullptr; float* d_szmin = nullptr; uint8_t* d_sflag = nullptr;
    // A world update (zr_world.cpp) that adds, removes, resizes or reorders objects asks the next zr_scene_finalize to carry the visibility
    // marks and the shadow flags of the kept draws to their new work-item numbers (k_history_carry) instead of forgetting them;
    // history_items: how many meshlet-instances the last zr_scene_finalize carried.
    bool history_remap = false; uint64_t history_items = 0;
    // k_shadow_occlusion tests a flagged item every fourth drawn pass, on the turn (work id + shadow_draws + sflag_turn) & 3.  A carry
    // that moves the items' work ids by d adds -d here, so that an item keeps its turn; where the kept draws move by different amounts
    // (mod 4), the amount most items move by.  shadow_draws itself stays what it counts.
    uint32_t sflag_turn = 0;
    float* d_hiz = nullptr; ZrHiz hiz = {}; int vis_cur = 0; bool last_two_round = false;
    uint32_t vis_mark_prev = 0;          // the stamp the resolve wrote into last frame's visibility marks (ZrHiz::vis_stamp)
    uint32_t* d_hiz_regions = nullptr; uint32_t n_hiz_regions = 0;      // the 64 x 64 pixel regions over owned tiles (k_hiz_build)
    ZrDevStats* d_stats = nullptr; ZrDevStats h_stats = {};
    // The shadow pipeline's statistics / work counters (slot 0) live in a block of their own: the pipeline resets what it counts itself
    // (k_scan), so it does not wait for the camera lane's k_frame_begin, and the camera lane does not wait for it.
    ZrDevStats* d_sstats = nullptr;
    // A resolve on the host's stream tallies its covered pixels into a block of its frame copy (only covered_part is used), zeroed on that
    // stream: the next frame's k_frame_begin zeroes d_stats on the camera lane while it may still be counting.  cov_block: where the
    // resolve of the frame enqueued last counted (d_stats, or one of these).
    ZrDevStats* d_rstats[2] = { nullptr, nullptr }; ZrDevStats* cov_block = nullptr;
    uint64_t last_work[2] = { 0, 0 };

    // object identity of the last frame (zr_set_id_capture, zr_ids.hip).  The winner planes are FrameCopy::prim_plane, shared with the forward variant.
    bool id_capture = false;             // the next frames keep their winner plane (FrameCopy::G.prim set)
    bool ids_frame = false, ids_this = false;      // the frame enqueued last kept it / the frame being enqueued does
    uint64_t scene_gen = 0;              // objects added or cleared
    // The queries' own state (zr_readback.cpp): gen / table_gen = the scene (scene_gen) of the last frame / of the table; table owns
    // draws, pool the slot arrays (counts ... hits)
    struct Ids {
        uint64_t gen = 0, table_gen = ~0ull;
        ZrOwn table, pool;
        ZrIdsDraw* draws = nullptr; uint32_t n_draws = 0, n_slots = 0, slot_cap = 0;
        uint32_t *counts = nullptr, *cov = nullptr, *list = nullptr, *n = nullptr;
        unsigned long long* keys = nullptr; zr_hit* hits = nullptr; uint2* obj = nullptr;
    } ids;

    // Delivering changes (zr_deliver_host.cpp, zr_delta.hip).  b: the buffers (ZrDeltaBuffers), made by zr_set_frame_delta(1), released by
    // zr_set_frame_delta(0), re-made beside the old ones by zr_resize.  full: the next delivery lists every tile; serial: deliveries since
    // enable.  scale: zr_set_frame_delta_scale's factor (1: the frame itself), a setting like hl.delta: set while delta is off and kept;
    // above 1 the buffers are sized for the scaled extent (zr_delta_extent) and b.scaled is the frame every delivery filters first.
    struct Delta { bool on = false, full = true; uint32_t serial = 0, scale = 1; ZrDeltaBuffers b; } delta;
    // Delivering a scaled frame (zr_deliver_host.cpp): where the host forms' filter writes, made at its first use through `ext` for
    // scale 2, the largest output (scale 1 is read from the frame itself)
    uint32_t* d_scaled = nullptr;
    // Highlighting a selection (zr_highlight_host.cpp, zr_highlight.hip).  set: a byte per slot, host state, cleared when scene_gen moves
    // (set_gen: the scene it was sized for); dirty: the device bitset `bits` (a bit per slot; bits_mem, re-made when the slot count
    // outgrows bits_words) is older than it - the next highlighted delivery stages it on the render stream first, so deliveries in
    // flight keep the set they were enqueued with.  plane (ceil(W / 64) * H words) and frame (W * H) are made at first use through `ext`.
    // delta: zr_set_frame_delta_highlight - the deliveries of changes deliver the highlighted frame.
    struct Highlight {
        std::vector<uint8_t> set; uint64_t set_gen = ~0ull; bool dirty = true, delta = false;
        zr_highlight_style style = { { 255, 160, 0, 255 }, { 255, 160, 0, 0 }, 2u, 0u };
        ZrOwn bits_mem; uint32_t* bits = nullptr; size_t bits_words = 0;
        unsigned long long* plane = nullptr; uint32_t* frame = nullptr;
    } hl;

    ZrOwn cube_mem; CubeDesc cube = {}; uint32_t cube_dim = 0, cube_levels = 0;
    uint64_t cube_gen = 0;               // of the cubemap's contents: bumped whenever they are replaced (zr_set_cubemap, which a world's override goes through)
    // The lighting pass's plane of standing terms (zr_lighting_host.cpp; ZrFramePlan::light_keep): 32 bytes per pixel, made at the first
    // fill through `ext` (alloc_failed: it could not be, and the context never keeps at this extent).  ONE plane: every lighting pass of the context is
    // enqueued on the host's stream, in frame order, so a fill is through before the next frame reads, and a read before the next fill.
    // now / key: the standing uniforms of the frame being enqueued / of the fill (ZrFrameFacts::light_uniforms_same).  last, count[]:
    // what the lighting pass enqueued last did with the plane (ZR_LIGHT_PLANE_*), and how often each happened (zr_get_light_keep).
    struct LightKey {
        float SB[16], cam[3]; uint32_t SD, n_dir, max_mips, cube_dim, cube_levels, debug_skip;
        XkLight dir[XK_MAX_DIRECTIONAL_LIGHTS_NUM];
    };
    // rest: the fill's slot and records (ZrRestRecord, zr_types.h), made with the plane in an allocation of their own (null: no room - the
    // context keeps, but never in one launch); by_arg: the passes that ran as the one launch (ZrFramePlan::light_args).
    // Settling (zr_settle.h; k_lighting_stand): marks = a word per part of the one launch, made with the records and zero-filled (null: no
    // room, or a build without the launch - the context rests through k_lighting_rest); settle / settle_key = the rule's state and the byte
    // image of the last stand launch's key; settle_off: ZR_NO_REST_SETTLE was set at zr_create; handed_out: zr_color_device_ptr gave the
    // frame's address to a caller who may write through it (until a resize voids it) - the library can no longer vouch for the target.
    struct SettleKey { ZrLightParams L; float cam[3]; uint32_t nDir, n_owned, _pad; const void *out, *plane, *rest, *owned, *marks; };
    struct LightKeep { float4* plane = nullptr; float4* rest = nullptr; bool alloc_failed = false; LightKey now = {}, key = {}; uint32_t last = 0;
                       uint64_t count[3] = { 0, 0, 0 }, by_arg = 0;
                       uint32_t* marks = nullptr; ZrSettleState settle; SettleKey settle_key = {}; bool settle_off = false, handed_out = false;
                       bool lead_off = false;      // ZR_NO_LEAD_WAVE was set at zr_create: a settling context rests through k_lighting_stand (k_lighting_lead's control)
                     } lk;
    float lut[256]; float* d_lut = nullptr;
    float* d_unorm_lut = nullptr;        // [0..255] = c / 255, [256..1279] = c / 1023 (IEEE quotients, computed on the host)

    static constexpr int EV_RING = 64;     // per-pass hipEvents of the last EV_RING timed frames (bench averages over them)
    // skydome + background passes (ZE:2657-2744, 3681-3699)
    ZrMesh sky_mesh; ZrSceneObject sky_obj; bool sky_set = false, sky_enabled = true;
    ZrOwn bg_mem; uint8_t* d_bg = nullptr; uint32_t bg_w = 0, bg_h = 0, bg_levels = 0; bool bg_set = false, bg_enabled = true;

    // One timed frame: its events (zr_timed.h has their order in the frame graph) and the rule's result for the frame's plan - which of
    // them this sample recorded, and what zr_get_pass_times_avg reads each figure from.
    struct TimedFrame {
        hipEvent_t ev[EV_COUNT] = {};
        ZrTimedRule rule;
    } timed[EV_RING];
    uint64_t frame_no = 0; bool rendered = false;
    uint32_t timing_interval = 1; bool timing_now = true; uint64_t sample_no = 0;    // pass events every interval-th frame
    TimedFrame* timed_frame() { return timing_now ? &timed[sample_no % EV_RING] : nullptr; }      // this frame's sample, or null

    // world + livelink + the content tree (zr_assets.cpp)
    std::string asset_root; bool assets_on = false;     // directory holding Profabs/ and Content/ (the engine's working directory)
    ZrWorld world;
    // the cubemap [0], the skydome [1] and the background [2] are the ones `world` names (set by a world load or update through the
    // content tree; cleared when the host replaces them with zr_set_cubemap / zr_set_skydome / zr_set_background)
    bool world_named[3] = { false, false, false };
    bool ll_incremental = false;         // zr_livelink_poll applies payloads with the update (zr_livelink_set_incremental)
    std::map<std::string, std::vector<ZrProfab>> profabs;
    std::mutex ll_mutex; std::thread ll_thread; std::atomic<bool> ll_run{ false };
    int ll_listen_fd = -1; bool ll_pending = false, ll_bind_any = false; ZrWorld ll_world; uint16_t ll_port = 0;

    // Overlaying lines (zr_overlay_host.cpp, zr_overlay.hip).  seg: the list, host state, tied to nothing of the scene; dirty: the device
    // copy d_seg (through `mem` with the records and rectangles the set-up kernel writes, all sized for `cap` segments and re-made when
    // the list outgrows them) is older than it - the next overlaid delivery stages it on the render stream first, so deliveries in
    // flight keep the list they were enqueued with.  frame (W * H) is made at first use through `ext`.  delta: zr_set_frame_delta_overlay.
    // (Last in the context: what the frame loop touches lies where it lay.)  A context that never sets a list has none of it.  The
    // camera is cam_prev_key's: the block of the frame enqueued last.
    struct Overlay {
        std::vector<zr_overlay_segment> seg; bool dirty = true, delta = false;
        zr_overlay_style style = { 0.0f, 0u, { 0u, 0u } };
        ZrOwn mem; zr_overlay_segment* d_seg = nullptr; ZrOvRecord* recs = nullptr; uint32_t* rects = nullptr; size_t cap = 0;
        uint32_t* frame = nullptr;
    } ov;
    // Casting rays (zr_raycast_host.cpp, zr_raycast.hip): the host form's staging on the device - cap rays in, cap records out - through
    // an owner of its own, grown on demand
    struct Rays { ZrOwn mem; zr_ray* rays = nullptr; zr_ray_hit* hits = nullptr; size_t cap = 0; } rays;
    // The wireframe (zr_wire_host.cpp, zr_wire.hip).  style: host state, kept like the highlight's; frame (W * H) is made at first use
    // through `ext`; delta: zr_set_frame_delta_wire.  A context that never asks for the stage has none of it.
    struct Wire { zr_wire_style style = { { 0, 0, 0, 255 }, 256u, 0u, 0u }; bool delta = false; uint32_t* frame = nullptr; } wire;
};

// What the deliveries of changes compare, list and size their buffers for: the frame at the delta scale (zr_ctx::Delta::scale), in tiles
struct ZrDeltaExtent { uint32_t W, H, tiles_x, n_tiles; };
static inline ZrDeltaExtent zr_delta_extent_of(uint32_t fw, uint32_t fh, uint32_t s)
{
    const uint32_t W = zr_scale_extent(fw, s), H = zr_scale_extent(fh, s), tx = (W + ZR_TILE - 1u) / ZR_TILE;
    return { W, H, tx, tx * ((H + ZR_TILE - 1u) / ZR_TILE) };
}
static inline ZrDeltaExtent zr_delta_extent(const zr_ctx* c) { return zr_delta_extent_of(c->W, c->H, c->delta.scale); }
int zr_fail(zr_ctx* c, int code, const std::string& msg);      // records the message (never throws), returns code
// ZR_OK at stage 0, else the refusal "<what> between the stages of a frame" (hint: "... (finish it with zr_render_lighting first)")
int zr_stage_idle(zr_ctx* c, const char* what, bool hint = true);
// What the shadow pass would draw, or where, may have changed: the next frame draws its map (see zr_ctx::caster_epoch, zr_frame_plan).  The device forms
// of the updates call it when they enqueue: their kernels are stream-ordered ahead of the next frame.
static inline void zr_casters_changed(zr_ctx* c) { c->caster_epoch++; c->camera_epoch++; }
// What the camera pass draws, how its work items are numbered or where its records go may have changed, the casters apart: the next
// frame draws round 2 (see zr_ctx::camera_epoch).
static inline void zr_camera_changed(zr_ctx* c) { c->camera_epoch++; }
// What the resolve reads beyond the camera pass's inputs may have changed: the next two frames resolve again (see zr_ctx::surface_epoch).
static inline void zr_surface_changed(zr_ctx* c) { c->surface_epoch++; }
// What the frames so far left on the device says nothing about the frames to come: the passes' work lists, the record buckets' plan, the
// visibility marks, the shadow pass's occlusion flags (ZrFrameCarry) - the next frame rebuilds, counts first, draws in one round.
enum : uint32_t { ZR_HIST_SHADOW_LIST = 1u, ZR_HIST_CAMERA_LIST = 2u, ZR_HIST_LISTS = 3u, ZR_HIST_PLAN = 4u, ZR_HIST_VISIBILITY = 8u, ZR_HIST_SHADOW_FLAGS = 16u,
                  ZR_HIST_LIGHT_PLANE = 32u };      // ... and the lighting pass's plane: the next resting frame fills it
static inline void zr_history_forgotten(zr_ctx* c, uint32_t what)
{
    ZrFrameCarry& k = c->carry;
    if (what & ZR_HIST_SHADOW_LIST) k.list_valid[0] = false;
    if (what & ZR_HIST_CAMERA_LIST) k.list_valid[1] = false;
    if (what & ZR_HIST_PLAN) k.plan_valid = false;
    if (what & ZR_HIST_VISIBILITY) k.vis_history = false;
    if (what & ZR_HIST_SHADOW_FLAGS) k.sflag_history = false;
    if (what & ZR_HIST_LIGHT_PLANE) k.light_valid = false;
}
#define HIPCHK(c, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) \
    return zr_fail((c), ZR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)
#define ARGCHK(c, cond) do { if (!(cond)) return zr_fail((c), ZR_ERR_ARG, "bad argument: " #cond); } while (0)
// zr_update.cpp: what orders the between-frames updates against the frames in flight (zr_ctx::upd)
int zr_update_begin(zr_ctx* c, hipStream_t x);                   // an update's scatter on x: behind the last apply / refit and the last update
int zr_update_end(zr_ctx* c, hipStream_t x);                     // ... and the frames of both parities behind it
int zr_update_tex_begin(zr_ctx* c, hipStream_t x);               // a texture update on x: behind the frame enqueued last and the last update
int zr_update_tex_end(zr_ctx* c, hipStream_t x);                 // ... and the next frame behind it
hipStream_t zr_update_lane(const zr_ctx* c);                     // the stream a host-form update is enqueued on
// the host form: `bytes` of src through the pinned staging ring, enqueue(staged, lane), the slot's event behind it
int zr_update_host_form(zr_ctx* c, const void* src, size_t bytes, const std::function<int(const void*, hipStream_t)>& enqueue);
// ... on stream x instead of the lane (the highlight set rides the render stream, between the deliveries that read it)
int zr_update_host_form_on(zr_ctx* c, hipStream_t x, const void* src, size_t bytes, const std::function<int(const void*, hipStream_t)>& enqueue);
int zr_update_frame(zr_ctx* c, hipStream_t s, int par);          // frame head: this frame's draw table, the updates that are due
int zr_update_table(zr_ctx* c);                                  // zr_scene_finalize: the parity-1 table of a new draw table
void zr_drop_draw_tables(zr_ctx* c);
hipError_t zr_update_sync(zr_ctx* c);                            // zr_sync_all: the last updates (on callers' streams)
// zr_instances_host.cpp
bool zr_instances_due(const zr_ctx* c, int par);                 // some object's table, flag or plane of this parity is behind
int zr_instances_apply(zr_ctx* c, hipStream_t s, int par);       // frame head (zr_update_frame): bring them up to date
int zr_instances_sync_host(zr_ctx* c, ZrSceneObject& o);         // zr_object_get_instances after a device-form update
// zr_mesh_update_host.cpp
bool zr_mesh_update_due(const zr_ctx* c, int par);               // some mesh's set of this parity is stale
int zr_mesh_update_frame(zr_ctx* c, hipStream_t s, int par);     // frame head (zr_update_frame): refit them, point the table at them
bool zr_mesh_update_table(zr_ctx* c);                            // zr_scene_finalize: new draw tables; true = the scene needs the parity-1 table
int zr_mesh_sync_host(zr_ctx* c, ZrMesh& m, bool meshlets);      // zr_mesh_get_vertices / _get_meshlets after an update
// No exception crosses the C-ABI: every exported function that returns a status runs its body through this, behind nothing but its
// bare argument checks (tests/test_abi_and_symbols.py holds the sources to it).
template <typename F> static inline int zr_guard(zr_ctx* c, F&& body) noexcept
{
    try { return body(); }
    catch (const std::bad_alloc&) { return zr_fail(c, ZR_ERR_OOM, "out of host memory"); }
    catch (const std::exception& e) { return zr_fail(c, ZR_ERR_IO, e.what()); }
    catch (...) { return zr_fail(c, ZR_ERR_IO, "unexpected exception"); }
}
// zr_context.cpp
hipError_t zr_sync_all(zr_ctx* c);     // every stream the library enqueues on
// zr_resize.cpp: everything of the context that is sized by the extent, made for W x H beside what the context has (which stays as it is
// and in use) and, by ZrExtentState::commit, put in its place.  zr_create makes the first set the same way.
int zr_extent_create(zr_ctx* c);
// zr_scene.cpp: the work pools' per-tile parts for n_tiles screen tiles, made through `into` and zeroed; *T and *chunk_tab / *chunk_capacity
// get the new pointers and sizes (T: a copy of c->tb; the rest of it stays).  zr_pool_plan_reset: the pools' few words of plan state zeroed.
int zr_make_pool_tiles(zr_ctx* c, ZrOwn& into, uint32_t n_tiles, ZrTriBins* T, uint4** chunk_tab, uint32_t* chunk_capacity);
hipError_t zr_pool_plan_reset(zr_ctx* c);
// zr_deliver_host.cpp: the buffers of the deliveries of changes for a W x H frame at the context's delta scale; moved into zr_ctx::Delta::b
// they become the context's (the old ones are released)
int zr_delta_make(zr_ctx* c, uint32_t W, uint32_t H, bool codec, ZrDeltaBuffers* out);
// zr_frame_host.cpp: the camera's projection, ViewProjSpace and ViewportInfo of the last zr_update_uniforms for the extent as it is now
void zr_uniforms_reproject(zr_ctx* c);
// Tile ownership (zr_tile_owner) of a grid of tiles among `world` ranks: the tiles `rank` owns, in increasing index = its slots in the
// packed buffer; map: tile -> owner * slots_per_rank + slot (k_untile); slots_per_rank: the most tiles any rank owns.
struct ZrTilePartition { std::vector<uint32_t> owned, map; uint32_t slots_per_rank = 0; };
ZrTilePartition zr_partition(uint32_t tiles_x, uint32_t tiles_y, uint32_t world, uint32_t rank);
// zr_update.cpp: the end of frame f < frame_no - f's own event, or where f recorded none a later one of the host's stream, recorded now if
// need be (zr_frame_end.h); and stream x made to wait for it.  Every reader of zr_ctx::ev_end but the one-launch frames' pacing goes through them.
int zr_frame_end(zr_ctx* c, uint64_t f, hipEvent_t* ev);
int zr_wait_frame_end(zr_ctx* c, hipStream_t x, uint64_t f);
// zr_frame_host.cpp
static inline hipStream_t lane_stream(const zr_ctx* c, ZrLane lane) { return lane == ZR_LANE_CAM ? c->cam_s : c->stream; }
// A timed frame's events `which`, in order, each on the stream the rule names - those of them the frame records (zr_timed.h: a stage the
// plan does not run records nothing); an untimed frame: nothing.  The passes call it where they always did and decide nothing themselves.
static inline int timed_events(zr_ctx* c, std::initializer_list<int> which)
{
    if (zr_ctx::TimedFrame* const T = c->timed_frame())
        for (int e : which)
            if (T->rule.records(e)) HIPCHK(c, hipEventRecord(T->ev[e], lane_stream(c, T->rule.lane[e])));
    return ZR_OK;
}
#define TIMED(c, ...) do { if (int _rc = timed_events((c), { __VA_ARGS__ })) return _rc; } while (0)
// The current shadow map: during a drawn shadow pass the one being drawn, else the one the last drawn pass left (zr_ctx::smap).
static inline float* shadow_buf(zr_ctx* c) { return c->d_shadow_ext ? c->d_shadow_ext : c->fc[c->smap].shadow; }
int set_winner_planes(zr_ctx* c, bool forward, bool id_capture, const char* what);      // zr_set_shading, zr_set_id_capture
// The frame's device copy of XkView brought up to date on s, and the camera lane's statistics zeroed where the plan says so (frame_begin;
// lighting_pass, for a frame planned as one launch that turns out to read XkView after all).
int zr_frame_uniforms(zr_ctx* c, hipStream_t s, bool reset_stats, bool reset_camera_list);
// zr_lighting_host.cpp: the lighting stage
void zr_light_facts(zr_ctx* c, ZrFrameFacts* f);       // frame_begin: what the plan reads about the plane
bool zr_light_plane_make(zr_ctx* c);                   // frame_begin, a frame planned to fill: the plane exists (false: it cannot, ever)
int empty_pixel_pass(zr_ctx* c);
int lighting_pass(zr_ctx* c);
// zr_readback.cpp
int ids_prepare(zr_ctx* c);            // frame_begin of a captured frame: the census's draw table
// The frame enqueued last kept its winners and still describes the scene (else the refusal, in `what`'s name); sync: finish it first
// (capture = false: a query that reads no winner plane - a ray cast - asks for the rest)
int ids_ready(zr_ctx* c, const char* what, bool sync, bool capture = true);
ZrIdsArgs ids_args(zr_ctx* c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);      // the census's arguments for a rectangle of that frame
size_t ids_slot_count(const zr_ctx* c);                                              // the slots of zr_instance_coverage
// A reader of that frame's copy - its winner plane (the census, the highlight's mask) or its GBuffer depth (the overlay) - was enqueued on
// the render stream: the frame that resolves into that copy next (the one after next, where it draws its camera pass) waits for it
// (both: the reader read what EITHER parity's next drawn frame may rewrite at its head - the instance planes and mesh sets of a scene that
// no update has split into parities yet, a ray cast - so both copies note it and the next frame waits as well)
int ids_reader_enqueued(zr_ctx* c, bool both = false);
// zr_highlight_host.cpp: the device bitset brought up to the host's set, on the render stream (a highlighted delivery, ahead of its launches)
int hl_upload(zr_ctx* c);
// zr_overlay_host.cpp: the overlay stage of a delivery on the render stream - the list brought up to date, set up for the camera of the
// frame enqueued last, drawn over `src` into `dst` (null: the context's scratch frame, made at first use); *out: where the result lies
int zr_overlay_stage(zr_ctx* c, const uint32_t* src, uint32_t* dst, const uint32_t** out);
// zr_overlay.hip: the n segments at seg set up for the camera (pvm, hw, hh) of a W x H frame into recs and rects (n each); `frame` (16-byte
// aligned) with the records drawn over it against `depth` into dst (4-byte aligned), all W x H
void zr_launch_overlay_setup(const zr_overlay_segment* seg, uint32_t n, const float* pvm, float hw, float hh, uint32_t W, uint32_t H, ZrOvRecord* recs, uint32_t* rects,
                             hipStream_t st);
void zr_launch_overlay_apply(const uint32_t* frame, const float* depth, const ZrOvRecord* recs, const uint32_t* rects, uint32_t n, uint32_t* dst, uint32_t W, uint32_t H,
                             const zr_overlay_style& style, hipStream_t st);
// zr_wire_host.cpp: the wire stage of a delivery on the render stream - the edges of the last frame's winners drawn over `src` into `dst`
// (null: the context's scratch frame, made at first use); *out: where the result lies
int zr_wire_stage(zr_ctx* c, const uint32_t* src, uint32_t* dst, const uint32_t** out);
// What is delivered: the frame enqueued last with the stages asked for applied in this order - the wire (zr_wire_stage), the highlight,
// the overlay's lines (zr_overlay_stage) - then filtered by `scale` (1: not filtered)
struct ZrDeliverWhat { bool wire, highlight, overlay; uint32_t scale; };
// zr_deliver_host.cpp: the two whole-frame forms of a delivery
int zr_deliver_to_host(zr_ctx* c, const char* what, ZrDeliverWhat w, uint8_t* dst, size_t bytes);
int zr_deliver_to_device(zr_ctx* c, const char* what, ZrDeliverWhat w, void* color_dev);
// zr_scene.cpp, also used by zr_world.cpp
float zr_srgb_decode8(uint32_t c);
int zr_material_prepare(zr_ctx* c, const zr_material* mat, ZrMaterialHost* out);
int zr_object_add_internal(zr_ctx* c, uint32_t mesh_id, const ZrMaterialHost& mat, const XkInstanceData* inst, uint32_t n_inst);
// zr_dist.cpp
void zr_dist_destroy(zr_ctx* c);
hipError_t zr_dist_sync(zr_ctx* c);
// zr_world.cpp, for zr_livelink_poll: a parsed world instantiated / applied as a difference, what either throws turned into the world
// path's own codes
int zr_apply_world_guarded(zr_ctx* c, const ZrWorld& w);
int zr_update_world_guarded(zr_ctx* c, const ZrWorld& w, zr_world_delta& D);
// zr_assets.cpp
std::string zr_asset_search(const zr_ctx* c, const std::string& name);
int zr_profab_from_disk(zr_ctx* c, const std::string& name, int* found);
int zr_world_apply_overrides(zr_ctx* c, const ZrWorld& w);
// ... in two steps, for zr_world_update_json: everything that can be refused (names, files) is read into the plan and nothing is
// changed; the commit sets what the plan holds.  which: bit k = re-read item k (0 cubemap, 1 skydome, 2 background), clear: bit k = the
// world no longer names item k, drop it (the state of a context that never had it).
struct ZrOverridePlan {
    unsigned which = 0, clear = 0;
    std::vector<uint8_t> cube_px[6]; uint32_t cube_dim = 0;
    std::vector<uint8_t> sky_px; uint32_t sky_w = 0, sky_h = 0; std::vector<XkVertex> sky_v; std::vector<uint32_t> sky_idx;
    std::vector<uint8_t> bg_px; uint32_t bg_w = 0, bg_h = 0;
};
int zr_world_plan_overrides(zr_ctx* c, const ZrWorld& w, ZrOverridePlan* plan);
int zr_world_commit_overrides(zr_ctx* c, ZrOverridePlan& plan);
// zr_scene.cpp, for zr_world_update_json: an object's instance buffers / material re-made in place (the caller has synchronised), and
// the scene finalised now instead of by the next frame
int zr_object_remake_instances(zr_ctx* c, ZrSceneObject& o, const XkInstanceData* inst, uint32_t n_inst);
int zr_object_remake_material(zr_ctx* c, ZrSceneObject& o, const ZrMaterialHost& mat);
int zr_scene_finalize(zr_ctx* c);
