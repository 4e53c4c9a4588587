/*
 * zelda_render.h — C-ABI of the MI355X-native deferred renderer (libzelda_render.so).
 *
 * The reference (iceprincefounder/ZeldaEngine) is a monolith with no plugin/FFI
 * boundary: its renderer is the private body of XkZeldaEngineApp.  The entry
 * points below are therefore the seam a maintainer would cut: each one replaces
 * the engine-internal function cited next to it and takes the engine's own byte
 * layouts (zelda_abi.h).  See INTEGRATION.md for the binding stubs.
 *
 * Conventions: 0 = OK, negative = error (message via zr_last_error); no C++
 * exception crosses the ABI; the caller owns every input pointer (contents are
 * copied before return); outputs are written into caller buffers.  A context is
 * bound to one HIP device and is NOT thread-safe, except zr_livelink_* which
 * hand a parsed world to the render thread under a mutex.
 *
 * There is no CPU fallback: every entry point that computes fails with
 * ZR_ERR_DEVICE when no HIP device is usable.
 */
#ifndef ZELDA_RENDER_H
#define ZELDA_RENDER_H

#include "zelda_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZR_OK            0
#define ZR_ERR_ARG      -1
#define ZR_ERR_DEVICE   -2
#define ZR_ERR_OOM      -3
#define ZR_ERR_PARSE    -4
#define ZR_ERR_IO       -5
#define ZR_ERR_STATE    -6
#define ZR_ERR_OVERFLOW -7
#define ZR_ERR_UNSUPPORTED -8

/* Version of this header's structs and entry points.  A host checks zr_abi_version() == ZR_ABI_VERSION after loading the library
 * (INTEGRATION.md); structs that may grow (zr_stats) are passed with their size as the caller knows it and only ever grow at the end. */
#define ZR_ABI_VERSION 7u

#ifndef ZR_TILE
#define ZR_TILE 32            /* screen tile edge in pixels (raster + multi-GPU partition unit); 32 or 64 */
#endif

/* Multi-GPU screen partition: tiles are owned in super-tiles of (1 << ZR_SUPERTILE_SHIFT)^2 tiles (128 x 128 pixels), dealt to the
 * ranks round-robin along x with a skew per super-tile row, so that a meshlet (tens of pixels) nearly always falls to ONE rank and
 * that rank alone transforms it, while neighbouring super-tiles still go to different ranks. */
#ifndef ZR_SUPERTILE_SHIFT
#define ZR_SUPERTILE_SHIFT 2
#endif
#define ZR_SUPERTILE_SKEW  3

typedef struct zr_ctx zr_ctx;

/* Flags for zr_config.flags */
#define ZR_FLAG_NO_FRUSTUM_CULL 1u  /* disable meshlet frustum culling (parity A/B) */
#define ZR_FLAG_NO_CONE_CULL    2u  /* disable meshlet cone culling   (parity A/B) */
#define ZR_FLAG_SKIP_COMPOSITE  4u  /* tile_world>1: caller gathers packed tiles itself */
#define ZR_FLAG_NO_HIZ          8u  /* disable two-pass Hi-Z occlusion culling of the camera pass (parity A/B) */
#define ZR_FLAG_SERIAL_PASSES   16u /* zr_render: shadow and camera pipelines on the one stream instead of side by side */
#define ZR_FLAG_PACKED_TILES    32u /* tile_world == 1: still light into the packed tile buffer (the multi-GPU data path on one GPU) */
#define ZR_FLAG_MESHLET_BINS   128u /* reserved: zr_create answers it with ZR_ERR_UNSUPPORTED */
#define ZR_FLAG_NO_RECT_CULL    64u /* tile_world > 1: do not reject meshlets by the rank's owned screen region before stage B (parity A/B) */
#define ZR_FLAG_NO_LIST_REUSE  256u /* rebuild the passes' instance-level work lists every frame instead of only when camera / light matrices or the
                                     * scene change (parity A/B; the lists are an acceleration structure, never pixels) - and draw the
                                     * shadow map every frame instead of keeping it while its light and casters stand still (zr_render) */
#define ZR_FLAG_NO_SHADOW_OCCLUSION 512u /* shadow pass: draw every survivor of the cull instead of leaving out what the map's own depths already hide
                                     * (parity A/B: the map is the same bit for bit either way) */
#define ZR_FLAG_SHADOW_OCCLUSION 1024u  /* ... and the opposite: occlusion-cull the shadow pass of a scene of any size (by default only from one
                                     * meshlet-instance per five texels of the map on, where it pays).  The flag forces a variant of the
                                     * PASS for A/B, so the pass runs: such a context draws its shadow map every frame, still light or
                                     * not (its shadow_occluded / shadow_late are every frame's own); automatic occlusion keeps the map */

typedef struct zr_config {
    uint32_t width, height;   /* swapchain extent, ZE:78-79 (default 1920x1080) */
    uint32_t shadow_dim;      /* SHADOWMAP_DIM, ZE:87 (0 -> 1024) */
    uint32_t debug_view;      /* GlobalConstants.SpecConstants 0..9, ZE:1803-1842 */
    int32_t  device;          /* HIP device ordinal */
    uint32_t tile_rank;       /* screen-tile partition: this context renders tiles t with */
    uint32_t tile_world;      /*   t % tile_world == tile_rank (0 -> 1) */
    uint32_t flags;
} zr_config;

/* One RGBA8 image; rgba8 == NULL selects the slot's engine default (ZE:4951-4978). */
typedef struct zr_image { const uint8_t* rgba8; uint32_t width, height; } zr_image;
/* Material = the 7 PBR samplers of BaseScene.frag:7-13 in order bc, m, r, n, ao, ev, ms. */
typedef struct zr_material { zr_image tex[XK_PBR_SAMPLER_NUMBER]; } zr_material;

/* XkCameraDesc (ZE:619-669) as plain floats; input of zr_update_uniforms. */
typedef struct zr_camera { float Position[3]; float Lookat[3]; float Speed, FOV, zNear, zFar; } zr_camera;

/* Per-pass GPU timings of the last zr_render, milliseconds (hipEvents on the render stream). */
enum { ZR_PASS_CULL_SHADOW = 0,   /* k_cull_box<SHADOW> + k_bin_count + k_scan + k_bin_fill (the map's clear rides in the previous lighting pass) */
       ZR_PASS_SHADOW,            /* k_raster_chunks + k_tile_slow<SHADOW> (clipped triangles) */
       ZR_PASS_CULL_CAMERA,       /* k_cull_box<GBUFFER> (also compacts round 1's list: last frame's visible set) */
       ZR_PASS_GBUFFER,           /* round 1 (the whole pass when the frame runs in one round): k_geom + k_tile */
       ZR_PASS_HIZ,               /* k_hiz_build + round 2's k_select (0 in a one-round frame) */
       ZR_PASS_GBUFFER2,          /* round 2: k_geom<Hi-Z> + k_tile (the last round also draws both rounds' clipped triangles) */
       ZR_PASS_RESOLVE,           /* k_resolve_gbuffer: the GBuffer write (+ k_mark where the resolve runs on the host's stream: the two durations, summed) */
       ZR_PASS_LIGHTING,          /* k_lighting */
       ZR_PASS_COMPOSITE, ZR_PASS_TOTAL, ZR_PASS_COUNT };

/* Frame statistics of the last zr_render (read back lazily by zr_get_stats). */
typedef struct zr_stats {
    uint64_t work_items[2];     /* meshlet-instances tested   [shadow, camera] */
    uint64_t survivors[2];      /* meshlet-instances binned   [shadow, camera] */
    uint64_t bin_entries[2];    /* (tile, meshlet-instance) pairs */
    uint64_t covered_pixels;    /* GBuffer pixels with geometry */
    uint64_t covered_shadow_texels; /* shadow-map texels with depth < 1 */
    uint32_t overflow;          /* nonzero: a bin list overflowed; frame invalid */
    uint32_t hiz_culled;        /* camera meshlet-instances rejected by the Hi-Z occlusion test (0 on a scene's first frame) */
    uint64_t round1_survivors;  /* of survivors[1]: drawn in round 1 (visible last frame); 0 when the frame ran in one round */
    uint32_t shadow_occluded;   /* of survivors[0]: not drawn - every texel their box reaches already held a nearer depth (the map is the same) */
    uint32_t shadow_late;       /* of survivors[0]: hidden last frame, not hidden now: drawn by the shadow pass's late launch */
    uint32_t hiz_culled_geom;   /* of hiz_culled: rejected only after a wave had transformed the meshlet's vertices (exact vertex box, every triangle
                                 * hidden); hiz_culled - hiz_culled_geom fell to the box bounds before any vertex work */
    uint32_t struct_bytes;      /* sizeof(zr_stats) as the LIBRARY knows it (ABI version 5: 96) */
} zr_stats;

/* --- lifetime (replaces InitVulkan/Cleanup, ZE:1714, 3747) --- */
int  zr_create(const zr_config* cfg, zr_ctx** out);
void zr_destroy(zr_ctx* ctx);
const char* zr_last_error(const zr_ctx* ctx);
/* Render on a caller-owned hipStream_t (NULL = the context's own stream). */
int  zr_set_stream(zr_ctx* ctx, void* hip_stream);
/* Replaces RecreateSwapChain (ZE:2311-2330, reached from ZE:1973-1976): a new extent, the same scene, nothing submitted again.
 * After zr_resize(ctx, W', H') everything observable - every later frame in every debug view and shading mode, the GBuffer targets, the
 * shadow map, the identity queries, covered_pixels / covered_shadow_texels, zr_world_save_json - is that of a new context with the same
 * zr_config but for the extent, given the same scene, the same calls and the same last uniforms.  Kept as they are, device memory and
 * all: meshes, objects (instances, visibility, materials - also what only a device-form update ever wrote), Profabs, the world, cubemap,
 * skydome, background, the shadow map, streams and staging, limits, bucket share, shading mode, debug view, id capture, timing
 * interval, livelink, the highlight set and style, the overlay list and style.  Re-made: whatever is sized by the extent.  Forgotten: every per-pixel history - the
 * next frame draws its camera pass as a scene's first frame does, while the shadow map stands or falls by its own key, as after a
 * camera move (a resize with light and casters still enqueues no shadow pipeline).  Until that frame the read-backs, the identity queries
 * and the deliveries answer as on a context that has rendered no frame.
 * Uniforms of zr_update_uniforms (and of the world forms, which go through it) are evaluated again for the new extent: Proj,
 * ViewProjSpace and ViewportInfo are bit-equal to a new context's.  Uniforms last set raw by zr_set_frame stay as given.
 * While delta is on its buffers are re-made for the new (scaled) extent; scale, highlight and overlay flags and packed mode stay, serial goes on
 * counting, the next delivery is a full one.  A caller-owned tile buffer (zr_set_tiles_buffer) goes back to the internal one, and
 * zr_color_device_ptr / zr_tiles_device_buffer answer anew.
 * The call synchronises everything the library has enqueued.  The new set is built beside the old one and swapped in on success: a
 * resize that cannot allocate reports what zr_create would have and leaves the context rendering at the old extent.
 * ZR_ERR_ARG (before anything is touched): a zero extent, an edge beyond 255 * ZR_TILE, more than 16 000 tiles.  ZR_ERR_STATE: between
 * the stages of a frame.  ZR_ERR_UNSUPPORTED: the native multi-GPU host is attached (zr_dist_prepare).  The extent the context already
 * has: ZR_OK, and nothing happens - no synchronisation, no rest ends. */
int  zr_resize(zr_ctx* ctx, uint32_t width, uint32_t height);
int  zr_get_extent(zr_ctx* ctx, uint32_t* width, uint32_t* height);      /* the extent as it is now (either pointer may be NULL) */
int  zr_tile_size(void);                            /* the ZR_TILE this library was built with */
uint32_t zr_abi_version(void);                      /* the ZR_ABI_VERSION this library was built with */

/* --- scene submission (replaces CreateRenderObjectsFromProfabs ZE:4922-5000, CreateMeshVertexBuffers
 *     ZE:4725-4770, CreateInstancedBuffer ZE:4795-4824) --- */
int  zr_mesh_create(zr_ctx* ctx, const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, uint32_t* mesh_id);
/* Attach caller-built meshlets (the `.meshlet` payload, ZE:7089-7127).  The mesh's draw order becomes
 * meshlet order exactly as CreateMeshVertexBuffers<XkMeshIndirect> flattens it (ZE:4733-4756). */
int  zr_mesh_set_meshlets(zr_ctx* ctx, uint32_t mesh_id, const XkMeshlet* m, uint32_t nm,
                          const uint32_t* meshlet_vertices, size_t nmv,
                          const uint8_t* meshlet_triangles, size_t nmt);
/* Build meshlets with the library's own clusteriser (BuildMeshlets, ZM:132-172: 64 v / 124 t / cone 0.2).
 * Called implicitly by zr_object_add for meshes that have none.  Draw order stays index order. */
int  zr_mesh_build_meshlets(zr_ctx* ctx, uint32_t mesh_id, uint32_t max_vertices, uint32_t max_triangles,
                            float cone_weight);
/* The clusteriser without a context (pure host code, no GPU needed): the ZeldaMeshlet tool's job.  NULL outputs = size query. */
int  zr_meshlets_build(const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, uint32_t max_vertices,
                       uint32_t max_triangles, float cone_weight, XkMeshlet* m, uint32_t* nm, uint32_t* meshlet_vertices,
                       size_t* nmv, uint8_t* meshlet_triangles, size_t* nmt, uint32_t* tri_order);
/* Copy the mesh's meshlets out (any pointer may be NULL; counts always returned). */
int  zr_mesh_get_meshlets(zr_ctx* ctx, uint32_t mesh_id, XkMeshlet* m, uint32_t* nm,
                          uint32_t* meshlet_vertices, size_t* nmv, uint8_t* meshlet_triangles, size_t* nmt);
/* n_inst == 0: non-instanced draw (Base.vert); n_inst >= 1: instanced draw (BaseInstanced.vert). */
int  zr_object_add(zr_ctx* ctx, uint32_t mesh_id, const zr_material* mat,
                   const XkInstanceData* inst, uint32_t n_inst);
/* Capacities of the camera pass's triangle-record arrays (record_chunks x 256 records of 32 bytes, + 4 bytes of tile id) and of its
 * clipped-triangle list; 0 = defaults (16 records per meshlet-instance of the scene, at least 32 Mi; 2^18 triangles).  A frame that
 * outgrows either reports ZR_ERR_OVERFLOW at zr_finish (zr_last_error names which).  Takes effect at the next frame (the arrays are re-made).
 * record_chunks is at most (2^30 - 1) / 256 = 4194303 (below 1 << 22): a larger value returns ZR_ERR_ARG and changes nothing. */
int  zr_set_limits(zr_ctx* ctx, uint32_t record_chunks, uint32_t slow_triangles);
/* The record arrays are laid out per frame as one bucket per screen tile, sized from the previous frame's count (+ 25 % + 128), and
 * an overflow region behind them for what a tile gets beyond its bucket.  percent (1..100, default 100) plans every bucket at that
 * share of its size: more of the arrays left to the overflow region, more records taking the slower route through it - same
 * frame, bit for bit (the overflow tests pin that).  Takes effect with the next plan (the next frame's end). */
int  zr_set_bucket_share(zr_ctx* ctx, uint32_t percent);
int  zr_scene_clear(zr_ctx* ctx);                   /* CleanupBasePass, ZE:4142 (also drops meshes and Profabs) */
int  zr_object_count(zr_ctx* ctx, uint32_t* n);
/* Copy out the instance array of object `index` (add order); *n = 0 for a non-instanced draw.  dst may be NULL. */
int  zr_object_get_instances(zr_ctx* ctx, uint32_t index, uint32_t* mesh_id, XkInstanceData* dst, uint32_t* n);
/* Moving instances.  Replace instances [first, first + n) of instanced object `index` (add order, as
 * zr_object_get_instances).  Takes effect with the next zr_render; frames already enqueued still draw the old values.  `data` may be
 * reused when the call returns.  The instance count is fixed at zr_object_add.  Neither call changes the scene (the identity queries
 * go on describing the last frame); a non-instanced object or a range beyond the instance count: ZR_ERR_ARG; between the stages of a
 * frame: ZR_ERR_STATE. */
int  zr_object_set_instances(zr_ctx* ctx, uint32_t index, uint32_t first, const XkInstanceData* data, uint32_t n);
/* The same from caller-owned DEVICE memory, in the order of hip_stream (NULL = the render stream): data_dev[i] replaces instance
 * idx_dev[i] (idx_dev NULL = instances first .. first + n - 1; with idx_dev the indices are the object's own and `first` only enters
 * the range check).  The library reads both buffers only inside hip_stream's order: a caller may overwrite them with work enqueued on
 * hip_stream after this call.  Device indices >= the object's instance count are ignored; an index listed twice in one call gets one
 * of its values.  Both buffers 4-byte aligned.  No host synchronisation (zr_object_get_instances reads back with one). */
int  zr_object_update_instances_async(zr_ctx* ctx, uint32_t index, uint32_t first, const uint32_t* idx_dev,
                                      const XkInstanceData* data_dev, uint32_t n, void* hip_stream);
/* Hiding and showing.  An instance is drawn iff its object is visible AND its own byte is nonzero; the two states are
 * independent (hiding an object and showing it again keeps its instance bytes), and zr_object_add starts everything visible.  A hidden
 * instance is absent from every pass and every entry point that draws - the shadow map, the camera pass, deferred and forward shading,
 * all debug views; zr_render, the staged calls, zr_render_geometry, rank contexts, zr_dist_frame - and the frame is, byte for byte, the
 * frame of a context built with only the shown objects and instances, in the same order.  Takes effect with the next zr_render; frames
 * already enqueued still draw the old state (two frames stay in flight, the host is never synchronised).  The scene does not change:
 * primitive ids, object and instance numbering and coverage slots are those of the full scene (a hidden instance keeps its slot,
 * zr_instance_coverage reads 0 there), the shadow partition by i % world keeps using the full scene's instance index, and the identity
 * queries go on describing the last frame until the next one is rendered.  zr_object_set_instances / zr_object_update_instances_async on
 * a hidden instance move it and leave it hidden; either order of a move and a hide between two frames gives the same result.
 * zr_object_get_instances returns hidden instances too.  zr_stats: covered_pixels, covered_shadow_texels, survivors and bin_entries
 * describe what was drawn; work_items still counts hidden meshlet-instances (they are tested, and rejected first).  zr_scene_clear and
 * world loads start over, with everything visible.
 * Between the stages of a frame: ZR_ERR_STATE.  A bad object index, the per-instance forms on a non-instanced object, a range beyond the
 * instance count, n > 0 with a null buffer, a misaligned idx_dev: ZR_ERR_ARG, and the context is unchanged.  n == 0, or a
 * zr_object_set_visible that flips nothing: ZR_OK, and nothing changes (the kept shadow map stays kept).
 * Whole object (any object, instanced or not); visible != 0 shows it: */
int  zr_object_set_visible(zr_ctx* ctx, uint32_t index, int visible);
/* Instances [first, first + n) of instanced object `index`: visible[i] == 0 hides, != 0 shows.  `visible` may be reused when the call
 * returns.  Works before the scene's first frame. */
int  zr_object_set_instance_visibility(zr_ctx* ctx, uint32_t index, uint32_t first, const uint8_t* visible, uint32_t n);
/* The same from caller-owned DEVICE memory, in the order of hip_stream (NULL = the render stream): visible_dev[i] applies to instance
 * idx_dev[i] (idx_dev NULL = instances first .. first + n - 1; with idx_dev the indices are the object's own and `first` only enters the
 * range check).  Both buffers are read only inside hip_stream's order: a caller may overwrite them with work enqueued on hip_stream
 * after this call.  Device indices >= the object's instance count are ignored; an index listed twice in one call gets one of its values.
 * idx_dev 4-byte aligned, visible_dev bytes.  No host synchronisation.  A scene no frame has used yet: ZR_ERR_STATE (use the host form). */
int  zr_object_update_instance_visibility_async(zr_ctx* ctx, uint32_t index, uint32_t first, const uint32_t* idx_dev,
                                                const uint8_t* visible_dev, uint32_t n, void* hip_stream);
/* Copy out: *object_visible, and one byte (0 / 1) per instance (any pointer may be NULL; *n = the instance count, 0 for a non-instanced
 * draw).  After a device-form update this reads back with one synchronisation. */
int  zr_object_get_visibility(zr_ctx* ctx, uint32_t index, int* object_visible, uint8_t* dst, uint32_t* n);
/* Deforming meshes.  Replace vertices [first, first + n) of mesh `mesh_id`, all 44 bytes of each XkVertex.  The
 * vertex count, the index buffer and the meshlet partition are fixed: only the values move; bounding spheres, normal cones and boxes are
 * refitted by the library.  Takes effect with the next zr_render; frames already enqueued still draw the old shape; every object that
 * uses the mesh sees it.  `v` may be reused when the call returns.  The scene does not change (the identity queries go on describing
 * the last frame).  A mesh no frame has used yet: the host copy is rewritten (and the bounds of meshlets already attached follow).
 * Between the stages of a frame: ZR_ERR_STATE; a bad mesh id, a range beyond the vertex count, n > 0 with v == NULL: ZR_ERR_ARG, and
 * the context is unchanged.  The skydome's mesh has no id: zr_set_skydome replaces it. */
int  zr_mesh_set_vertices(zr_ctx* ctx, uint32_t mesh_id, uint32_t first, const XkVertex* v, uint32_t n);
/* The same from caller-owned DEVICE memory, in the order of hip_stream (NULL = the render stream).  The library reads v_dev only inside
 * hip_stream's order: a caller may overwrite it with work enqueued on hip_stream after this call.  v_dev 4-byte aligned (else
 * ZR_ERR_ARG).  No host synchronisation.  A mesh no frame has used yet has no device copy: ZR_ERR_STATE (use zr_mesh_set_vertices). */
int  zr_mesh_update_vertices_async(zr_ctx* ctx, uint32_t mesh_id, uint32_t first, const XkVertex* v_dev, uint32_t n, void* hip_stream);
/* Copy out the mesh's current vertices (dst may be NULL; *n = the vertex count).  After a device-form update this and
 * zr_mesh_get_meshlets read back with one synchronisation. */
int  zr_mesh_get_vertices(zr_ctx* ctx, uint32_t mesh_id, XkVertex* dst, uint32_t* n);
/* Changing textures.  Replace the image of material slot `slot` (0..6: bc, m, r, n, ao, ev, ms) of object `index`
 * (add order).  Same width and height as the image the slot holds; all mip levels and the packed material follow, built on the GPU to
 * the bytes zr_object_add would have built.  Takes effect with the next zr_render; frames already enqueued still sample the old image.
 * `img->rgba8` may be reused when the call returns.  The scene does not change: work lists, plan, visibility history, the kept shadow
 * map and the identity queries all stand.  An image that happens to be constant stays an image (no collapse on update).
 * Between the stages of a frame: ZR_ERR_STATE; a bad object index, slot > 6, null or misaligned data, or a size other than the slot's:
 * ZR_ERR_ARG; a slot that holds no image - zr_object_add collapsed a constant image to its texel, or took the engine default -:
 * ZR_ERR_STATE (a slot meant to change must be added with a non-constant image of its final size).  The context is unchanged by a
 * refused call.  Out of scope: promoting a constant slot to an image, changing an image's size, updating a sub-rectangle; the
 * skydome, the background and the cubemap (zr_set_skydome / zr_set_background / zr_set_cubemap replace those). */
int  zr_object_set_texture(zr_ctx* ctx, uint32_t index, uint32_t slot, const zr_image* img);
/* The same from caller-owned DEVICE memory (width * height * 4 bytes RGBA8, row-major, 4-byte aligned) in the order of hip_stream
 * (NULL = the render stream); read only inside that order: a caller may overwrite it with work enqueued on hip_stream after this
 * call.  No host synchronisation. */
int  zr_object_update_texture_async(zr_ctx* ctx, uint32_t index, uint32_t slot, const void* rgba8_dev, uint32_t width, uint32_t height,
                                    void* hip_stream);
/* Copy out mip level `level` of the slot's current image (dst may be NULL; *w, *h = that level's size, *levels = the chain's length;
 * cap = the room at dst in bytes).  After an update this reads back with one synchronisation.  A slot without an image: ZR_ERR_STATE. */
int  zr_object_get_texture(zr_ctx* ctx, uint32_t index, uint32_t slot, uint32_t level, uint8_t* dst, size_t cap, uint32_t* w, uint32_t* h,
                           uint32_t* levels);
/* 6 RGBA8 sRGB faces in Vulkan layer order +X,-X,+Y,-Y,+Z,-Z (RHICreateTextureCubeResource ZE:5908-6150);
 * mips are generated like RHIGenerateMipmaps (ZE:6348-6433).  faces == NULL: built-in 1x1 grey. */
int  zr_set_cubemap(zr_ctx* ctx, const uint8_t* const faces[6], uint32_t dim);

/* Skydome pass (CreateSkydomePass ZE:2690-2744, draw ZE:3681-3691): the sky mesh (Content/Models/skydome.obj in the engine)
 * with its sRGB texture, drawn unlit after the lighting quad with depth LESS against the deferred depth.  tex == NULL removes it.
 * Background pass (ZE:2657-2688, 3693-3699): full-screen quad at z = 1, LESS_OR_EQUAL, sRGB texture.  Both only in debug view 0. */
int  zr_set_skydome(zr_ctx* ctx, const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, const zr_image* tex);
int  zr_set_background(zr_ctx* ctx, const zr_image* tex);
/* XkWorld::EnableSkydome / EnableBackground (zr_world_load_json sets them from the JSON). */
int  zr_set_sky_flags(zr_ctx* ctx, int enable_skydome, int enable_background);

/* --- per-frame uniforms (replaces UpdateWorld ZE:4294-4308 + UpdateUniformBuffer ZE:4585-4664) --- */
int  zr_update_uniforms(zr_ctx* ctx, const zr_camera* cam,
                        const XkLight* dir, uint32_t n_dir, const XkLight* point, uint32_t n_point,
                        const XkLight* spot, uint32_t n_spot, float roll_stage, float roll_light, float time);
/* Raw form: the three UBOs the engine memcpy's each frame (ZE:4626-4664). */
int  zr_set_frame(zr_ctx* ctx, const XkUniformBufferMVP* camera, const XkUniformBufferMVP* shadow, const XkView* view);
int  zr_get_frame(zr_ctx* ctx, XkUniformBufferMVP* camera, XkUniformBufferMVP* shadow, XkView* view);
int  zr_set_debug_view(zr_ctx* ctx, uint32_t spec_constants);
/* Which of the engine's two scene pipelines shades the frame (ZE:93 ENABLE_DEFERRED_SHADING picks one at compile time):
 *   ZR_SHADING_DEFERRED (default)  BaseScene.frag -> GBuffer -> BaseLighting.frag (ZE:2803-2997, 3417-3480, 3531-3540);
 *   ZR_SHADING_FORWARD             Base.frag:46-144 straight into the frame (pipelines ZE:2749-2801, draws ZE:3544-3680): unquantised
 *                                  inputs, no Mask, FinalColor * ShadowFactor, Base.frag's own debug table (:123-143; view 9 = view 0).
 * Takes effect with the next frame; between the stages of a frame: ZR_ERR_STATE.  The GBuffer targets are still written (zr_read_gbuffer). */
#define ZR_SHADING_DEFERRED 0u
#define ZR_SHADING_FORWARD  1u
int  zr_set_shading(zr_ctx* ctx, uint32_t mode);

/* --- the frame (replaces RecordCommandBuffer ZE:3160-3744 + vkQueueSubmit ZE:2014) ---
 * cull -> shadow -> cull -> gbuffer -> lighting [-> composite].  Asynchronous: the call only enqueues.  The shadow pipeline and
 * the lighting pass go to the render stream (zr_set_stream), the camera pipeline to a stream of the library's own that the
 * lighting pass waits for; so work the host enqueues on the render stream afterwards is ordered after the finished frame, and
 * up to two frames are in flight (the next frame's camera pipeline runs next to this frame's lighting), as in the reference
 * (MAX_FRAMES_IN_FLIGHT, ZE:77).  zr_finish and the read-back entry points wait for everything.
 * The shadow map is KEPT while the shadow pass's matrices (light, stage), the casters (objects, instances, vertices, meshlets, limits) and
 * the map's buffer stand still: such a frame enqueues no shadow pipeline at all and lights from the map of the last drawn pass - the same
 * map bit for bit.  The pass's statistics (zr_get_stats slot 0, shadow_occluded, shadow_late) then stay those of the last drawn pass, its
 * pass times read exactly 0, and zr_read_shadowmap / zr_copy_frame_async return the kept map.  Every entry point (zr_render, the staged
 * calls, zr_render_geometry) decides alike.  Drawn every frame: a tile- or instance-partitioned map, a caller-owned one
 * (zr_set_shadow_buffer), contexts with ZR_FLAG_NO_LIST_REUSE or ZR_FLAG_SHADOW_OCCLUSION.
 * Round 2 of the camera pass is kept likewise while the camera pass's matrices (camera, stage) and what it draws (objects, instances,
 * vertices, meshlets, visibility, limits, bucket share, skydome) stand still: from the third frame of such a rest on, a frame draws
 * round 1 - what owned a pixel of the frame before, which is all that can own one now - and enqueues no Hi-Z build and no second
 * round; the GBuffer is the same bit for bit.  Its statistics (survivors, hiz_culled, hiz_culled_geom, bin_entries) stay those of the last
 * drawn round 2, ZR_PASS_HIZ and ZR_PASS_GBUFFER2 read exactly 0.  Every entry point decides alike; never kept: contexts with
 * ZR_FLAG_NO_LIST_REUSE (and ZR_FLAG_NO_HIZ has no second round to keep).  A frame that ran out of record room (ZR_ERR_OVERFLOW from
 * zr_finish) is incomplete, and so is every frame of the rest that keeps round 2 behind it - each reports the overflow again - until
 * zr_finish has reported it: the frame after that draws both rounds again.
 * The WHOLE camera pass, and the GBuffer with it, is kept one step further: when, beyond the above, nothing the GBuffer write reads
 * changed (material textures: zr_object_set_texture / zr_object_update_texture_async; the winner plane of zr_set_shading and
 * zr_set_id_capture) and both internal GBuffer copies were written from these very inputs - from the third frame after the last such
 * change on - a frame enqueues, on the render stream alone: the uniform upload, the shadow pipeline if the map is drawn, and the
 * lighting pass (with its one-pixel pre-launch); where zr_render keeps the shadow map too (a map at least two frames old), the upload and the pre-launch go to the
 * library's own, otherwise idle stream beside the previous frame's lighting pass, and the render stream waits for them.  The GBuffer, the
 * visibility history, the record plan and every camera-pass statistic (covered_pixels included) stay those of the last drawn frame, so
 * zr_get_stats, zr_read_gbuffer, the identity queries and zr_copy_frame_async answer as on a drawn frame; ZR_PASS_CULL_CAMERA,
 * ZR_PASS_GBUFFER, ZR_PASS_HIZ, ZR_PASS_GBUFFER2 and ZR_PASS_RESOLVE read exactly 0.  Lights, debug view, background and cubemap are
 * inputs of the lighting pass and end nothing.  Never kept whole: a context that draws a skydome (its round 2 is still kept), and
 * whatever never keeps round 2.
 * The lighting pass of a frame that keeps BOTH its camera pass and its shadow map keeps, per pixel, what the point lights do not feed:
 * the shadow factor (the 25 PCF taps), the directional lights' share of the direct term and the reflection.  The first such frame
 * computes them as ever and stores them as exact fp32 in a plane of 32 bytes per pixel, made then (no room for it: the context never
 * keeps, and that is no error); every later one loads them and computes only the point lights, the indirect term and the compose - the
 * frame is the same bit for bit, in every debug view.  The plane stands while that GBuffer and that map stand and, compared byte for
 * byte, the shadow matrix, the camera position, the directional lights in use and their count, the cubemap (zr_set_cubemap and a
 * world's override replace it) and its mip count do; anything else - the point lights, the debug view, the background, the time -
 * ends nothing, except that a frame whose empty-pixel shortcut is off (debug view 6) needs a plane filled by such a frame.  When it no
 * longer stands, the next frame that rests fills it again.  Deferred shading only; never with ZR_FLAG_NO_LIST_REUSE, never on a context
 * whose map is never kept.  zr_get_light_keep tells what the last frame did.
 * A frame that loads them is ONE kernel launch when it has at most 64 point lights, its empty-pixel shortcut is on and its debug view
 * is not 9: what it reads of the uniforms travels as a kernel argument, the colour of the pixels nothing was drawn to - it moves with
 * the point lights - is computed inside the launch, and nothing is uploaded; the device copy of the uniforms is brought up to date by
 * the next frame that reads it (zr_light_keep::read_by_arg counts such frames).  The frame is the same bit for bit.
 * Such a launch also LEAVES AS THEY STAND the pixels no point light reaches.  It shades the frame in parts of half a tile (32 x 16
 * pixels); a part whose world-space box - widened to the origin, where a pixel nothing was drawn to is shaded, if it holds one - lies
 * outside every point light's radius would get, pixel for pixel, the colour the launch before wrote to the same addresses, and once a
 * launch has written that colour the part returns after its set-up: no GBuffer, plane or frame byte of it moves.  The frame is the
 * same bit for bit.  The library vouches for the bytes it leaves alone: whatever could change them or the colour they should hold -
 * any lighting pass that is not such a launch, any difference in the launch's parameters (debug view, background, camera, directional
 * lights, target, extent), zr_set_background, zr_resize - starts a new generation, in which every part is shaded once before it may
 * stand again.  Contexts that never leave a pixel alone, and write every pixel of every resting frame as before: those with a
 * caller-owned tiles buffer (zr_set_tiles_buffer) or the native multi-GPU host, every rank of a tile_world above 1, a context whose frame address zr_color_device_ptr has
 * handed out (the caller may write through it; until a zr_resize voids it), and every context created with ZR_NO_REST_SETTLE in the
 * environment.  zr_get_rest_settled counts the parts that stand. */
int  zr_render(zr_ctx* ctx);
/* The same frame in three stages (zr_render = all three, in this order), so that a multi-GPU host can place its
 * collectives between them: shadow pass | deferred-scene pass (cull, raster, GBuffer write) | deferred-lighting pass. */
int  zr_render_shadow(zr_ctx* ctx);
int  zr_render_gbuffer(zr_ctx* ctx);
int  zr_render_lighting(zr_ctx* ctx);
/* Both geometry passes at once, side by side as zr_render runs them: the shadow pass on the render stream, the deferred-scene
 * pass on the library's own high-priority stream (zr_render_lighting waits for it).  A host that post-processes the shadow map
 * on another stream (the min all-reduce over ranks) makes that stream wait with zr_stream_wait_shadow, and the render stream
 * wait for its result, before zr_render_lighting.  zr_render = zr_render_geometry + zr_render_lighting.  Replaces the pair
 * zr_render_shadow + zr_render_gbuffer. */
int  zr_render_geometry(zr_ctx* ctx);
int  zr_stream_wait_shadow(zr_ctx* ctx, void* hip_stream);   /* hip_stream waits for the last enqueued shadow pass */
int  zr_finish(zr_ctx* ctx);                        /* stream sync + overflow check */
int  zr_get_pass_times(zr_ctx* ctx, float ms[ZR_PASS_COUNT]);              /* last frame */
int  zr_get_pass_times_avg(zr_ctx* ctx, uint32_t last_n, float ms[ZR_PASS_COUNT]);  /* mean of the last n <= 64 timed frames */
int  zr_get_frame_latencies(zr_ctx* ctx, uint32_t n, float* ms);   /* begin-to-end GPU ms of the last n timed frames, newest first; returns the count */
/* GPU ms between the ends of consecutive frames, last n <= 511 frames, newest first; returns the count.  Inside a run of frames that
 * are one launch (see zr_render) only every ZR_REST_END_EVERY-th frame records its end: every frame between two recorded ends reports
 * the MEAN of its run - the time between the two records over the number of frames - and the sum over a window whose ends are
 * recorded is exact.  ZR_REST_END_EVERY is read from the environment at zr_create (1 .. 64, default 8; 1: every frame records its end
 * and reports its own period).  Such frames upload nothing, so nothing but these ends paces the host: it runs at most
 * 4 + ZR_REST_END_EVERY - 1 frames ahead of the device (11 by default) before zr_render waits. */
int  zr_get_frame_periods(zr_ctx* ctx, uint32_t n, float* ms);
/* Pass events on every interval-th frame (default 1, 0 = never).  A record is a small bubble (about 5 us) on the stream it sits on, and
 * a sampled frame records the events of the stages it runs, no others: 2 where the frame is one launch; 3 where it keeps camera pass and
 * shadow map otherwise; 5 where it keeps the camera pass and draws the map; 10 where it draws its camera pass (12 where that frame's
 * resolve runs on the host's stream).  The figures of a stage that did not run read exactly 0. */
int  zr_set_timing_interval(zr_ctx* ctx, uint32_t interval);
/* bytes = sizeof(zr_stats) of the caller's header: the library writes min(bytes, its own size), so an older host is never overrun. */
int  zr_get_stats(zr_ctx* ctx, zr_stats* out, size_t bytes);
/* What the lighting pass of the frame enqueued last did with the plane of standing terms (see zr_render), and how many frames of the
 * context did each so far.  bytes = sizeof(zr_light_keep) of the caller's header, as with zr_get_stats. */
#define ZR_LIGHT_PLANE_IGNORED 0u   /* computed everything, stored nothing: a drawn frame, forward shading, a context that never keeps */
#define ZR_LIGHT_PLANE_FILLED  1u   /* computed everything and stored the standing terms */
#define ZR_LIGHT_PLANE_READ    2u   /* loaded the standing terms */
typedef struct zr_light_keep {
    uint32_t last, _pad;         /* ZR_LIGHT_PLANE_* of the last frame */
    uint64_t ignored, filled, read;
    uint64_t plane_bytes;        /* device memory the plane takes (0: not made) */
    uint64_t read_by_arg;        /* of `read`: the passes that were the frame's ONE launch - their uniforms kernel arguments, no upload,
                                  * no one-pixel launch, no event wait (at most 64 point lights, the empty-pixel shortcut on, not view 9) */
} zr_light_keep;
int  zr_get_light_keep(zr_ctx* ctx, zr_light_keep* out, size_t bytes);
/* The parts of a resting frame's one launch (owned tiles x 2) and how many of them stand settled after the frame enqueued last (see
 * zr_render): 0 unless that frame was such a launch on a context that settles.  Waits for the frame and reads the marks back: for tests
 * and tools, nothing is counted per frame. */
int  zr_get_rest_settled(zr_ctx* ctx, uint32_t* parts, uint32_t* settled);
/* ... and which: standing[p] = 1 where part p (owned tile slot * 2 + the half of the tile, upper first) stands settled, else 0;
 * bytes = zr_get_rest_settled's parts. */
int  zr_get_rest_settled_parts(zr_ctx* ctx, uint8_t* standing, size_t bytes);

/* --- read-back (there is no swapchain; replaces vkQueuePresentKHR ZE:2030) --- */
int  zr_read_color(zr_ctx* ctx, uint8_t* rgba8, size_t bytes);         /* W*H*4 row-major, top-left origin */
/* target 0 depth D32F, 1 SceneColor RGBA8, 2 GBufferA A2R10G10B10, 3 GBufferB RGBA8, 4 GBufferC RGBA8,
 * 5 GBufferD RGBA16F (ZE:2807-2843); W*H*{4,4,4,4,4,8} bytes. */
int  zr_read_gbuffer(zr_ctx* ctx, int target, void* dst, size_t bytes);
int  zr_read_shadowmap(zr_ctx* ctx, float* dst, size_t bytes);        /* dim*dim*4 */
/* The frame enqueued last, copied into caller-owned DEVICE buffers (W*H*4 bytes of RGBA8; dim*dim*4 of depth; either may be NULL) in
 * stream order, without synchronising the host: the copies run behind that frame's lighting pass and ahead of anything the next
 * zr_render puts on the render stream - what a presenting host with two frames in flight uses instead of zr_read_color. */
int  zr_copy_frame_async(zr_ctx* ctx, void* color_dev, void* shadow_dev);

/* --- delivering changes ("Delivering to a remote client"; DESIGN.md §5, "Delivering changes") ---
 * The frame as the 32 x 32 tiles that differ from what was delivered last: what a host that ships frames to a remote client sends instead
 * of W*H*4 bytes.  The context keeps ONE delivered copy of the frame - what the client holds.  A delivery compares the frame enqueued last
 * with that copy tile by tile, lists every tile in which any byte of any pixel inside the frame differs, in increasing tile index
 * t = ty * ceil(W/32) + tx (the numbering of zr_tile_partition), and makes the delivered copy the frame.  The k-th listed tile's pixels
 * are at pixels + k * 4096: 32 rows of 32 RGBA8 pixels, tile pixel (x, y) = frame pixel (tx*32 + x, ty*32 + y), pixels outside the frame
 * 0.  Applying a delivery to the client's copy gives exactly zr_read_color's bytes.  The comparison is against the last DELIVERY, not the
 * previous frame: frames rendered without a delivery in between are skipped over.  The first delivery after zr_set_frame_delta(ctx, 1)
 * and after zr_frame_delta_reset (a new client) lists every tile and sets full.
 * Buffers are always full-sized (no truncation case): total_tiles uint32 and total_tiles * 4096 bytes; only the first n_tiles entries
 * and slots are written, what lies behind them is left untouched. */
typedef struct zr_frame_delta {   /* 16 bytes */
    uint32_t n_tiles;      /* tiles listed by this delivery */
    uint32_t total_tiles;  /* ceil(W/32) * ceil(H/32) */
    uint32_t full;         /* 1: first delivery after enable / reset - every tile is listed */
    uint32_t serial;       /* deliveries since enable, this one included (a client notices a lost one) */
} zr_frame_delta;
/* enable != 0 allocates the delivered copy, the host form's packed buffer and list, and the marks; 0 releases them
 * (enable == ZR_FRAME_DELTA_PACKED: the compressed forms below as well; every other value behaves as 1).  A context that
 * never enables it allocates nothing and its frames enqueue what they always did.  ZR_ERR_UNSUPPORTED where the lighting pass does not
 * write the row-major frame itself (tile_world > 1, ZR_FLAG_PACKED_TILES); between the stages of a frame: ZR_ERR_STATE. */
int  zr_set_frame_delta(zr_ctx* ctx, int enable);
int  zr_frame_delta_reset(zr_ctx* ctx);             /* the next delivery is a full one again (serial goes on counting) */
/* Host form: zr_finish first (its error is passed on, as by zr_read_color), then the header, then n_tiles * 4 and n_tiles * 4096 bytes -
 * a frame at rest costs a 16-byte copy.  cap_tiles == total_tiles and bytes == total_tiles * 4096, else ZR_ERR_ARG; out_bytes = the
 * caller's sizeof(zr_frame_delta) (passed like zr_stats). */
int  zr_read_frame_delta(zr_ctx* ctx, uint32_t* tiles, uint32_t cap_tiles, uint8_t* pixels, size_t bytes, zr_frame_delta* out, size_t out_bytes);
/* Device form, into caller-owned DEVICE buffers (16 bytes of header; total_tiles uint32; total_tiles * 4096 bytes, 16-byte aligned):
 * synchronises nothing, ordered on the render stream exactly as zr_copy_frame_async's colour copy - behind the lighting pass of the
 * frame enqueued last, ahead of whatever the next zr_render enqueues.  The two forms may be mixed: they share the delivered copy in
 * stream order.
 * Both: ZR_ERR_STATE while delta is off, before the first finished frame, and between the stages of a frame. */
int  zr_copy_frame_delta_async(zr_ctx* ctx, void* header_dev, void* tiles_dev, void* pixels_dev);

/* --- delivering changes, compressed ("Delivering changes": the record format) ---
 * zr_set_frame_delta(ctx, ZR_FRAME_DELTA_PACKED) enables the raw forms above and two packed ones beside them, which list the same tiles
 * but deliver each as a losslessly compressed RECORD instead of 4 096 bytes, encoded on the GPU behind the lighting pass: only the
 * compressed bytes cross a link.  Going between 1 and ZR_FRAME_DELTA_PACKED while on synchronises and makes or releases the packed forms'
 * buffers alone: the delivered copy, full and serial stand.  All four forms share them in stream order and may be mixed freely.
 * A record is a multiple of 8 bytes and at most 4 104:
 *   bytes 0..3  tile pixel (0, 0), RGBA     4..5  u16: the record's length in 8-byte words     6..7  u16 mode: 0 coded, 1 raw
 *   mode 0:  8..39  64 width nibbles, group g in byte g / 2, even g in the low nibble;  40..  the groups' payloads, in group order
 *   mode 1:  8..4103  the tile's 4 096 bytes as a raw slot has them - taken exactly when the coded record would be longer than 4 104
 * Per channel a value is predicted by the one to its left, in column 0 by the one above; pixel (0, 0) is the header's.  The residual
 * r = (p - pred) mod 256 is zigzagged: z = 2r for r < 128, else 2 (255 - r) + 1.  The tile is 16 blocks of 8 x 8 pixels (block = by * 4 + bx);
 * group g = block * 4 + channel has 64 values, value i = block pixel (i & 7, i >> 3), and a width b (0..8) = the bit length of its largest
 * z.  Its payload is b little-endian 64-bit words, bit i of word k = bit k of value i: a coded record is 40 + 8 * sum(b) bytes, a tile of one
 * colour 40.  The stream is the records of the listed tiles in list order, back to back; record k is stream[offsets[k] .. offsets[k + 1]),
 * offsets[0] = 0 and offsets[n_tiles] = bytes.  List, offsets and stream are the same from run to run. */
#define ZR_FRAME_DELTA_PACKED 3
#define ZR_FRAME_DELTA_RECORD_MAX 4104u   /* bytes of the longest record */
typedef struct zr_frame_delta_packed {   /* 32 bytes */
    uint32_t n_tiles, total_tiles, full, serial;   /* as zr_frame_delta */
    uint32_t bytes;        /* length of the stream */
    uint32_t raw_tiles;    /* records in mode 1 */
    uint32_t reserved[2];  /* 0 */
} zr_frame_delta_packed;
/* Host form: zr_finish first, then the header, then n_tiles * 4, (n_tiles + 1) * 4 and `bytes` bytes (at rest: the 32-byte header, and
 * offsets[0] = 0).  Capacities are always full: cap_tiles == total_tiles, cap_offsets == total_tiles + 1, cap_bytes == total_tiles * 4104,
 * else ZR_ERR_ARG; what lies behind the written part is left untouched.  out_bytes = the caller's sizeof(zr_frame_delta_packed). */
int  zr_read_frame_delta_packed(zr_ctx* ctx, uint32_t* tiles, uint32_t cap_tiles, uint32_t* offsets, uint32_t cap_offsets, uint8_t* stream, size_t cap_bytes,
                                zr_frame_delta_packed* out, size_t out_bytes);
/* Device form, into caller-owned DEVICE buffers of those capacities (32 bytes of header; stream_dev 16-byte aligned, the others 4-byte):
 * ordered and unsynchronised exactly as zr_copy_frame_delta_async.
 * Both: ZR_ERR_STATE while packed delivery is not enabled, whatever the arguments; the other refusals are those of the raw forms, in
 * their order (arguments first). */
int  zr_copy_frame_delta_packed_async(zr_ctx* ctx, void* header_dev, void* tiles_dev, void* offsets_dev, void* stream_dev);
/* The client's side, context-free host code: a packed delivery (n listed tiles, n + 1 offsets, `bytes` of stream) applied to the client's
 * width * height * 4 copy of the frame; only pixels inside the frame are touched.  The input is taken as hostile and checked as a whole
 * before anything is written - ZR_ERR_PARSE for: a tile index >= the frame's tiles or not ascending; offsets that do not start at 0, do
 * not ascend or run past `bytes`; a record whose length word disagrees with its offsets or with 40 + 8 * sum(b), or that is longer than
 * 4 104 bytes; a width nibble above 8; an unknown mode.  Never reads beyond tiles[n), offsets[n] and stream[bytes). */
int  zr_frame_delta_decode(const uint32_t* tiles, const uint32_t* offsets, uint32_t n, const uint8_t* stream, size_t bytes, uint32_t width, uint32_t height,
                           uint8_t* client_rgba8);

/* --- delivering a scaled frame ("Delivering a scaled frame"; DESIGN.md §5, "Delivering a scaled frame") ---
 * The frame box-filtered by an integer factor `scale` (1 .. 8) in linear light, on the GPU behind the lighting pass, before any byte
 * crosses a link: what a host sends a client whose window is smaller than the frame, a thumbnail - and, from a context created at twice
 * the extent and delivered at scale 2, an anti-aliased picture.  The scaled extent is Wd = ceil(W/scale), Hd = ceil(H/scale).  Output
 * pixel (X, Y) covers the frame pixels X*scale <= x < min(W, (X+1)*scale), Y*scale <= y < min(H, (Y+1)*scale): n of them, fewer than
 * scale*scale in the last column and row - edge blocks average the pixels that exist.  Integer arithmetic throughout, so the kernel, the
 * host statement below and a client's own code agree byte for byte:
 *   T[c] = floor(65535 * L(c/255) + 1/2), L the sRGB EOTF (v/12.92 for v <= 0.04045, else ((v + 0.055)/1.055)^2.4) in float64
 *   R, G, B each:  S = the block's sum of T[p]; the result is the number of k in 1..255 with 2*S >= (T[k-1] + T[k]) * n - the byte whose
 *                  T is nearest the block's mean, ties upward
 *   A:             floor((2 * sum + n) / (2 * n))
 * A block of one colour yields that colour, and scale 1 is the identity.  Picking and the identity queries stay in the context's own
 * pixels: (x, y) of a scaled frame is the rectangle (x*scale, y*scale, scale, scale) of zr_pick.
 * Refusals, the context unchanged: ZR_ERR_ARG for scale 0 or above 8, a null pointer, a wrong byte count, a color_dev that is not
 * 4-byte aligned; ZR_ERR_UNSUPPORTED where the lighting pass does not write the row-major frame itself (tile_world > 1,
 * ZR_FLAG_PACKED_TILES: the cases of zr_set_frame_delta); ZR_ERR_STATE before the first finished frame and between the stages of one. */
int  zr_frame_scaled_extent(uint32_t width, uint32_t height, uint32_t scale, uint32_t* w, uint32_t* h);      /* context-free */
/* The host statement of the filter, context-free host code: what a client or a test compares with.  bytes == Wd*Hd*4. */
int  zr_frame_downscale(const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t scale, uint8_t* dst, size_t bytes);
/* Host form: zr_finish first (its error is passed on, as by zr_read_color), one launch into a buffer the context makes at first use
 * (for scale 2, the largest output; released by zr_destroy or a zr_resize), then Wd*Hd*4 bytes to the host - row-major, top-left origin. */
int  zr_read_color_scaled(zr_ctx* ctx, uint32_t scale, uint8_t* rgba8, size_t bytes);
/* Device form, straight into a caller-owned DEVICE buffer of Wd*Hd*4 bytes (4-byte aligned): synchronises nothing, ordered on the render
 * stream exactly as zr_copy_frame_async's colour copy - behind the lighting pass of the frame enqueued last, ahead of whatever the next
 * zr_render enqueues.  Two frames stay in flight. */
int  zr_copy_frame_scaled_async(zr_ctx* ctx, uint32_t scale, void* color_dev);
/* Deltas of the scaled frame.  zr_set_frame_delta_scale sets the scale the deliveries of changes work at (default 1: the frame itself);
 * callable only while delta is off (ZR_ERR_STATE while it is on), kept across zr_set_frame_delta(ctx, 0).  Above 1, zr_set_frame_delta
 * sizes everything for (Wd, Hd) and makes one scaled-frame buffer; every delivery, in all four forms, first filters the frame into it
 * and then compares, lists and encodes the SCALED frame: total_tiles = ceil(Wd/32) * ceil(Hd/32), the capacities, the list order, the
 * record format and zr_frame_delta_decode (the caller passes Wd, Hd) all follow from the scaled extent, and applying a delivery gives
 * exactly zr_read_color_scaled's bytes.  At scale 1 nothing differs in buffers, launches or bytes.
 * zr_get_frame_delta_extent answers for the current scale whether delta is on or off. */
int  zr_set_frame_delta_scale(zr_ctx* ctx, uint32_t scale);
int  zr_get_frame_delta_extent(zr_ctx* ctx, uint32_t* width, uint32_t* height, uint32_t* total_tiles, uint32_t* scale);

/* --- highlighting a selection ("Highlighting a selection"; DESIGN.md §5, "Highlighting a selection") ---
 * The frame delivered with a set of instances marked: an outer outline round them and, optionally, a fill over them, drawn on the GPU
 * behind the lighting pass from the winner plane of the identity queries below (zr_set_id_capture), before any byte crosses a link.
 * The frame itself is never marked: zr_read_color, zr_copy_frame_async, zr_color_device_ptr, the scaled forms and the deltas of a context
 * with highlight delivery off deliver what they always did.
 * The set is one flag per slot of zr_instance_coverage (objects in add order, then their instances in order; a non-instanced object has
 * one slot: first = 0, n = 1).  It is host state: changing it draws nothing, ends no rest and touches no frame; a delivery enqueued
 * before a change delivers the old set, even while still in flight.  It is cleared whenever the object list changes (zr_object_add,
 * zr_scene_clear, a world load, a world update that adds, removes, resizes or reorders objects).
 * The rule, integer arithmetic throughout, so the kernels, the host statement below and a client's own code agree byte for byte:
 *   M(x, y) = 1 iff the frame's winner at (x, y) - what zr_read_ids reports - is a scene primitive whose slot is in the set; the
 *             skydome, the background, empty pixels and pixels outside the frame have M = 0
 *   M = 1:                                                  R, G, B blended with `fill`
 *   M = 0 and some M = 1 within |dx| <= radius, |dy| <= radius:  R, G, B blended with `outline` (an outer outline, over whatever is there)
 *   otherwise the pixel, and A always, stays
 *   blend(p, q, a) = floor((p*(255 - a) + q*a + 127) / 255) per channel, on the frame's gamma-encoded bytes
 * An empty set, and radius 0 with fill opacity 0, are the identity.  At a scale above 1 the highlighted frame is filtered afterwards
 * (zr_frame_downscale of it): the radius is in the context's own pixels.
 * Refusals, the context unchanged, arguments first: ZR_ERR_ARG for a null pointer, a wrong count, a scale outside 1..8, a misaligned
 * destination, an object or range out of bounds, a radius above 8, a non-zero reserved; ZR_ERR_UNSUPPORTED where the lighting pass does
 * not write the row-major frame (tile_world > 1, ZR_FLAG_PACKED_TILES); ZR_ERR_STATE for the cases of zr_pick - no finished frame,
 * between the stages of one, the last frame rendered without id capture, the scene changed after it.  A highlighted delivery needs a
 * captured frame whatever the set holds. */
typedef struct zr_highlight_style {   /* 16 bytes */
    uint8_t  outline[4];   /* R, G, B, opacity 0..255 */
    uint8_t  fill[4];      /* R, G, B, opacity 0..255 (0: selected pixels stay as they are) */
    uint32_t radius;       /* outline width in frame pixels, 0..8 (0: no outline) */
    uint32_t reserved;     /* 0, else ZR_ERR_ARG */
} zr_highlight_style;      /* default: outline {255, 160, 0, 255}, fill {255, 160, 0, 0}, radius 2 */
/* Arguments as for zr_object_set_instance_visibility: on[i] != 0 puts instance first + i of `object` into the set, 0 takes it out. */
int  zr_highlight_set(zr_ctx* ctx, uint32_t object, uint32_t first, const uint8_t* on, uint32_t n);
int  zr_highlight_clear(zr_ctx* ctx);
/* One byte per slot; bytes = the slot count = zr_instance_coverage's byte count / 4. */
int  zr_highlight_get(zr_ctx* ctx, uint8_t* dst, size_t bytes);
/* bytes = the caller's sizeof(zr_highlight_style) (passed like zr_stats) */
int  zr_set_highlight_style(zr_ctx* ctx, const zr_highlight_style* style, size_t bytes);
int  zr_get_highlight_style(zr_ctx* ctx, zr_highlight_style* style, size_t bytes);
/* Host form: zr_finish first (its error is passed on), two launches (and the filter at a scale above 1) into buffers the context makes
 * at first use, then Wd*Hd*4 bytes to the host. */
int  zr_read_color_highlighted(zr_ctx* ctx, uint32_t scale, uint8_t* rgba8, size_t bytes);
/* Device form, into a caller-owned DEVICE buffer of Wd*Hd*4 bytes (4-byte aligned): synchronises nothing, ordered on the render stream
 * exactly as zr_copy_frame_scaled_async.  It reads the last frame's winner plane: the frame after next waits for it before it rewrites
 * that plane (as for zr_instance_coverage_async). */
int  zr_copy_frame_highlighted_async(zr_ctx* ctx, uint32_t scale, void* color_dev);
/* Deltas of the highlighted frame: callable only while delta is off (ZR_ERR_STATE while it is on), kept across zr_set_frame_delta(ctx, 0).
 * While on, every delivery of changes, in all four forms and at any delta scale, highlights, then filters, then compares and lists:
 * extents, capacities, list order and record format stay, applying a delivery gives exactly zr_read_color_highlighted(ctx, delta scale)'s
 * bytes, a frame at rest with an unchanged set lists 0 tiles, and changing the set lists the tiles whose highlighted bytes differ.
 * Every delivery then has the refusals above. */
int  zr_set_frame_delta_highlight(zr_ctx* ctx, int on);
/* The host statement of the rule over a byte-per-pixel mask (non-zero = highlighted), context-free host code: what a client or a test
 * compares with.  style_bytes = the caller's sizeof(zr_highlight_style); bytes == width*height*4. */
int  zr_frame_highlight(const uint8_t* rgba8, const uint8_t* mask, uint32_t width, uint32_t height, const zr_highlight_style* style, size_t style_bytes,
                        uint8_t* dst, size_t bytes);

/* --- overlaying lines ("Overlaying lines"; DESIGN.md §5, "Overlaying lines") ---
 * The frame delivered with a list of line segments drawn over it, depth-tested against the frame's own depth plane, on the GPU behind
 * the lighting pass and before any byte crosses a link: a selection's bounding box, a gizmo's axes, a grid, a light's radius, another
 * camera's frustum.  The frame itself is never drawn into: zr_read_color, zr_copy_frame_async, the scaled and highlighted forms and the
 * deltas of a context with overlay delivery off deliver what they always did.  A context that never calls these allocates nothing.
 * End points are in the space of a non-instanced vertex: they go through the proj * view * model of the frame enqueued LAST (a
 * zr_set_frame / zr_update_uniforms after that frame does not move the lines), so a box computed from zr_object_get_instances lands on
 * its instance.  The list is host state and no instance set: it survives zr_object_add, world updates and zr_resize; setting it draws
 * nothing, ends no rest and touches no frame; a delivery enqueued before a change delivers the old list, even while still in flight.
 * The rule, segment by segment in list order (csrc/zr_overlay.h states it in full; the kernels, zr_frame_overlay and a client's own
 * code agree byte for byte):
 *   clip = PVM * (p, 1) in fp32, every fma explicit; a non-finite component draws nothing
 *   the segment is clipped against z >= 0, 4w +- x >= 0, 4w +- y >= 0, w - z >= 0 and needs w > 0 at both ends
 *   both ends are projected and snapped to 1/256 pixel as a triangle's corners are; z = clip.z / clip.w
 *   X-major iff |dX| >= |dY|: every column whose centre cx = 256x + 128 lies in [Xa, Xb) gets the one row that holds
 *   Ya + floor((2 (cx - Xa) dY + dX) / (2 dX)) - the line's crossing of the column centre rounded to 1/256 pixel; Y-major alike.  A
 *   chain a-b, b-c covers the joint once; lines are one context pixel wide
 *   depth d = za + t (zb - za), t = (cx - Xa) / dX, clamped between za and zb
 *   visible iff ZR_OVERLAY_XRAY or d - depth_bias <= the frame's depth there (what zr_read_gbuffer(ctx, 0, ..) returns; NaN: hidden)
 *   visible: R, G, B blended with rgba at opacity rgba[3] (the highlight's blend); hidden: at opacity round(rgba[3] * hidden_opacity / 255)
 *   A is never changed; a pixel crossed by several segments takes them in list order
 * At a scale above 1 the overlaid frame is filtered afterwards; with a highlight the order is highlight, overlay, filter.
 * Refusals, the context unchanged, arguments first: ZR_ERR_ARG for a null pointer, n above ZR_OVERLAY_MAX_SEGMENTS, an unknown flag
 * bit, a wrong byte count, a scale outside 1..8, a misaligned destination, a negative or non-finite depth_bias, hidden_opacity above 255,
 * a non-zero reserved; ZR_ERR_UNSUPPORTED where the lighting pass does not write the row-major frame (tile_world > 1,
 * ZR_FLAG_PACKED_TILES); ZR_ERR_STATE before the first finished frame and between the stages of one - and, with highlight != 0, the
 * cases of zr_read_color_highlighted. */
typedef struct zr_overlay_segment {   /* 32 bytes */
    float    a[3], b[3];   /* the two end points */
    uint8_t  rgba[4];      /* R, G, B, opacity 0..255 */
    uint32_t flags;        /* ZR_OVERLAY_XRAY, every other bit 0 */
} zr_overlay_segment;
#define ZR_OVERLAY_XRAY 1u             /* not depth-tested */
#define ZR_OVERLAY_MAX_SEGMENTS 16384u
typedef struct zr_overlay_style {     /* 16 bytes */
    float    depth_bias;       /* >= 0, finite: taken off a line's depth before the test */
    uint32_t hidden_opacity;   /* 0..255: what is left of a segment's opacity where it is hidden (0: hidden parts are not drawn) */
    uint32_t reserved[2];      /* 0, else ZR_ERR_ARG */
} zr_overlay_style;        /* default: 0.0f, 0 */
/* Replaces the list; n = 0 clears it (seg may then be null). */
int  zr_overlay_set(zr_ctx* ctx, const zr_overlay_segment* seg, uint32_t n);
/* *n in: the room at dst in segments, out: the list's length; ZR_ERR_ARG when the room is too small (*n is still set).  dst null: the length alone. */
int  zr_overlay_get(zr_ctx* ctx, zr_overlay_segment* dst, uint32_t* n);
/* bytes = the caller's sizeof(zr_overlay_style) (passed like zr_stats) */
int  zr_set_overlay_style(zr_ctx* ctx, const zr_overlay_style* style, size_t bytes);
int  zr_get_overlay_style(zr_ctx* ctx, zr_overlay_style* style, size_t bytes);
/* Host form: zr_finish first (its error is passed on), the launches into buffers the context makes at first use, then Wd*Hd*4 bytes to
 * the host.  highlight != 0: the highlighted frame underneath (it needs a captured frame); 0: no id capture is needed. */
int  zr_read_color_overlaid(zr_ctx* ctx, uint32_t scale, int highlight, uint8_t* rgba8, size_t bytes);
/* Device form, into a caller-owned DEVICE buffer of Wd*Hd*4 bytes (4-byte aligned): synchronises nothing, ordered on the render stream
 * exactly as zr_copy_frame_scaled_async.  It reads the last frame's depth plane: the frame after next waits for it before it rewrites
 * that plane (as for zr_copy_frame_highlighted_async and the winner plane). */
int  zr_copy_frame_overlaid_async(zr_ctx* ctx, uint32_t scale, int highlight, void* color_dev);
/* Deltas of the overlaid frame: callable only while delta is off (ZR_ERR_STATE while it is on), kept across zr_set_frame_delta(ctx, 0).
 * While on, every delivery of changes, in all four forms and at any delta scale, highlights (where zr_set_frame_delta_highlight is on),
 * overlays, filters, then compares and lists: applying a delivery gives exactly zr_read_color_overlaid(ctx, delta scale, ..)'s bytes, a
 * frame at rest with an unchanged list lists 0 tiles, and a changed list lists the tiles whose overlaid bytes differ. */
int  zr_set_frame_delta_overlay(zr_ctx* ctx, int on);
/* The host statement of the rule, context-free host code: depth = width*height floats (zr_read_gbuffer's plane 0), pvm = the frame's
 * proj * view * model, 16 floats column-major; seg may be null when n = 0.  style_bytes = the caller's sizeof(zr_overlay_style);
 * bytes == width*height*4. */
int  zr_frame_overlay(const uint8_t* rgba8, const float* depth, uint32_t width, uint32_t height, const float* pvm, const zr_overlay_segment* seg, uint32_t n,
                      const zr_overlay_style* style, size_t style_bytes, uint8_t* dst, size_t bytes);

/* --- wireframe: the visible triangles' edges drawn over the delivered frame ("Wireframe"; DESIGN.md §5, "Wireframe") ---
 * "Shaded + wire": the lit frame with the edges of the triangle that won each pixel drawn over it - hidden lines are removed by
 * construction - on all of the scene or on the highlight set only, on the GPU behind the lighting pass from what the frame enqueued
 * last left on the device: its winner plane (zr_set_id_capture), draw table, instance records, vertex sets and camera block.  Meshes
 * deformed and instances moved on the device are followed with no host copy.  The frame itself is never drawn into, and a context that
 * never asks for the stage enqueues and allocates what it always did.
 * The rule (csrc/zr_wire.h states it in full; the kernel, zr_frame_wire and a client's own code agree byte for byte).  For a pixel
 * (x, y) whose winner is a scene primitive with the clip-space corners c0, c1, c2 (the camera pass's own float32 values), in float64:
 *   Hk = (hw (xk + wk), hh (yk + wk), wk), hw = W / 2, hh = H / 2        homogeneous screen coordinates, pixels
 *   for the edges (0,1), (1,2), (2,0):  l = Ha x Hb;  s = (lx (x + 0.5) + ly (y + 0.5)) + lz;  n2 = lx lx + ly ly
 *   on the wire iff for some edge n2 > 0 and s s <= (r r) n2, r = width_256 / 512 (a NaN compares false)
 * i.e. the pixel centre lies within half the width of an edge's line; the rule holds for corners behind the eye.  A pixel on the wire
 * has R, G, B blended with rgba at opacity rgba[3] (the highlight's blend), A stays.  With ZR_WIRE_SELECTED only pixels whose instance
 * is in the highlight set are candidates (an empty set: no wire).  The skydome, the background and empty pixels never get a wire.
 * Stages of a delivery, in this fixed order: wire, highlight, overlay, then the filter by `scale`.
 * Refusals, the context unchanged, arguments first: ZR_ERR_ARG for an unknown stage bit, a scale outside 1..8, a null or misaligned
 * pointer, a wrong byte count, a bad style; ZR_ERR_UNSUPPORTED where the lighting pass does not write the row-major frame
 * (tile_world > 1, ZR_FLAG_PACKED_TILES); ZR_ERR_STATE before the first finished frame, between the stages of one and - with
 * ZR_STAGE_WIRE as with ZR_STAGE_HIGHLIGHT - for the cases of zr_pick. */
typedef struct zr_wire_style {        /* 16 bytes */
    uint8_t  rgba[4];      /* R, G, B, opacity 0..255 */
    uint32_t width_256;    /* full line width in 1/256 pixel, 1..4096 */
    uint32_t flags;        /* ZR_WIRE_SELECTED or 0 */
    uint32_t reserved;     /* 0, else ZR_ERR_ARG */
} zr_wire_style;           /* default: {0, 0, 0, 255}, 256, 0 */
#define ZR_WIRE_SELECTED 1u            /* only the instances of the highlight set (zr_highlight_set) */
#define ZR_WIRE_WIDTH_MAX 4096u
#define ZR_STAGE_WIRE      1u
#define ZR_STAGE_HIGHLIGHT 2u
#define ZR_STAGE_OVERLAY   4u
/* bytes = the caller's sizeof(zr_wire_style) (passed like zr_stats).  Kept across zr_resize, zr_scene_clear and world loads. */
int  zr_set_wire_style(zr_ctx* ctx, const zr_wire_style* style, size_t bytes);
int  zr_get_wire_style(zr_ctx* ctx, zr_wire_style* style, size_t bytes);
/* One delivery for every combination of stages (a mask of ZR_STAGE_*): the host form (zr_finish first, Wd*Hd*4 bytes to the host) and
 * the device form (a caller-owned DEVICE buffer of Wd*Hd*4 bytes, 4-byte aligned, ordered on the render stream as
 * zr_copy_frame_scaled_async; the frame after next waits before it rewrites what the stages read).  stages = 0, ZR_STAGE_HIGHLIGHT and
 * ZR_STAGE_HIGHLIGHT | ZR_STAGE_OVERLAY deliver the bytes of zr_read_color_scaled, _highlighted and _overlaid(.., 1, ..). */
int  zr_read_color_staged(zr_ctx* ctx, uint32_t stages, uint32_t scale, uint8_t* rgba8, size_t bytes);
int  zr_copy_frame_staged_async(zr_ctx* ctx, uint32_t stages, uint32_t scale, void* color_dev);
/* Deltas of the wired frame: callable only while delta is off (ZR_ERR_STATE while it is on), kept across zr_set_frame_delta(ctx, 0).
 * While on, every delivery of changes draws the wire first: applying one gives zr_read_color_staged(ctx, ZR_STAGE_WIRE | .., delta scale). */
int  zr_set_frame_delta_wire(zr_ctx* ctx, int on);
/* The host statement of the rule, context-free host code.  prim = width*height winners (zr_read_ids, ZR_IDS_PRIMITIVE); corners = 9
 * floats per primitive: x, y, w of its three clip-space corners; a winner at or above n_prims is no triangle; selected = n_prims bytes
 * (non-zero = in the set, read only with ZR_WIRE_SELECTED) or null: every primitive.  style_bytes = the caller's
 * sizeof(zr_wire_style); bytes == width*height*4; corners may be null when n_prims = 0. */
int  zr_frame_wire(const uint8_t* rgba8, const uint32_t* prim, uint32_t width, uint32_t height, const float* corners, uint32_t n_prims, const uint8_t* selected,
                   const zr_wire_style* style, size_t style_bytes, uint8_t* dst, size_t bytes);

/* --- object identity of the last frame (which object won each pixel: picking, box selection, per-instance coverage) ---
 * What is reported is the deferred-scene pass's depth-test winner, i.e. what the GBuffer holds: the same in deferred and forward
 * shading and in every debug view.  The skydome and the background are not objects: they never appear and never hide a scene winner.
 * Every query describes the frame enqueued last (as zr_read_gbuffer).  The synchronous ones call zr_finish first and pass its error on
 * (an overflowed frame: ZR_ERR_OVERFLOW).  ZR_ERR_STATE when no frame has been rendered, when the last frame was rendered without
 * capture, when the scene changed after it (zr_object_add, zr_scene_clear, a world load) with no frame since, or between the stages of
 * a frame.  A rank context (tile_world > 1) reports its owned tiles only: pixels of other ranks' tiles read as none.
 * Summed over all slots, zr_instance_coverage equals zr_stats.covered_pixels. */
/* Keep the deferred-scene pass's per-pixel winner, from the next frame on; default off (one 4-byte store per pixel and frame).
 * Between the stages of a frame: ZR_ERR_STATE (as zr_set_shading). */
int  zr_set_id_capture(zr_ctx* ctx, int enable);

#define ZR_IDS_PRIMITIVE 0  /* W*H*4: global draw-order primitive id (non-instanced draws first, then instanced; per draw
                               instance * triangles + triangle), 0xFFFFFFFF = none */
#define ZR_IDS_OBJECT    1  /* W*H*8: {object, instance} per pixel; object = add order (as zr_object_get_instances),
                               instance = 0 for a non-instanced draw; {0xFFFFFFFF, 0xFFFFFFFF} = none */
int  zr_read_ids(zr_ctx* ctx, int kind, void* dst, size_t bytes);

typedef struct zr_hit {          /* 32 bytes */
    uint32_t object, instance;   /* as ZR_IDS_OBJECT */
    uint32_t pixels;             /* pixels of the rectangle this instance won */
    uint32_t triangle;           /* primitive id within the instance at the nearest pixel */
    uint32_t x, y;               /* the nearest pixel: least depth, ties to the least y*W + x */
    float    depth;              /* its D32F depth (GBuffer target 0) */
    uint32_t reserved;           /* 0 */
} zr_hit;
/* Distinct (object, instance) winners in the rectangle, clipped to the frame.  Sorted by depth, then object, then instance.
 * *n = the total count; min(*n, cap) entries are written.  w == 0 or h == 0: ZR_ERR_ARG.  w = h = 1 is a point pick. */
int  zr_pick(zr_ctx* ctx, uint32_t x, uint32_t y, uint32_t w, uint32_t h, zr_hit* hits, uint32_t cap, uint32_t* n);

/* Pixels each instance won in the last frame.  One uint32 per instance slot: objects in add order, then their instances in order;
 * a non-instanced draw has one slot.  bytes = 4 * sum over objects of max(1, instances). */
int  zr_instance_coverage(zr_ctx* ctx, uint32_t* counts, size_t bytes);
/* The same counts into a caller-owned DEVICE buffer, stream-ordered on the render stream behind the frame enqueued last, with no host
 * sync (the pattern of zr_copy_frame_async).  The frame after next, which reuses that frame's winner plane, waits for it. */
int  zr_instance_coverage_async(zr_ctx* ctx, void* counts_dev, size_t bytes);

/* --- casting rays ("Casting rays"; DESIGN.md §5, "Casting rays") ---
 * The nearest triangle along each ray: object, instance, triangle, the ray parameter t, the barycentric weights and the face normal.
 * Rays see the scene AS THE FRAME ENQUEUED LAST DREW IT, like the identity queries: that frame's draw table, instance records, vertex
 * sets and model matrix (a corner's world position is the camera pass's own arithmetic, bit for bit); updates made since take effect
 * with the next zr_render.  Hidden objects and instances are not hit; the skydome is no object and is never hit.  Id capture is not
 * needed.  A rank context (tile_world > 1) and the native multi-GPU host hold the whole scene and answer like any other context.
 * The rule (one statement for host and device, csrc/zr_raycast.h): a watertight float32 / float64 test - a ray through a closed
 * surface cannot slip between two triangles that share an edge; the hit with the least t wins, ties go to the least global primitive
 * id (ZR_IDS_PRIMITIVE's numbering).  The hit point is origin + t * dir = (1 - u - v) A + u B + v C.  A ray with a non-finite
 * component, dir == 0, a NaN bound or t_min > t_max hits nothing and is flagged ZR_RAY_INVALID.
 * Out of scope: an acceleration structure over instances (every ray tests every instance's bounding sphere: fine for an editor's rays
 * and tens of thousands of instances), the skydome, interpolated normals / UVs / materials, a scene no frame has drawn. */
typedef struct zr_ray     { float origin[3]; float t_min; float dir[3]; float t_max; } zr_ray;          /* 32 bytes */
typedef struct zr_ray_hit { uint32_t object, instance;   /* as ZR_IDS_OBJECT; 0xFFFFFFFF both = nothing hit */
                            uint32_t triangle;           /* draw-order triangle within the instance, as zr_hit::triangle (0xFFFFFFFF: none) */
                            uint32_t flags;              /* ZR_RAY_HIT | ZR_RAY_HIT_BACK | ZR_RAY_INVALID */
                            float t, u, v; uint32_t reserved;   /* 0 */
                            float normal[3]; uint32_t reserved2; } zr_ray_hit;   /* 48 bytes; normal = (B-A) x (C-A), not normalised */
#define ZR_RAY_HIT       1u   /* hit flag: something was hit */
#define ZR_RAY_HIT_BACK  2u   /* hit flag: from behind - dir and (B-A) x (C-A) point the same way (the side the camera pass culls) */
#define ZR_RAY_INVALID   4u   /* hit flag: the ray itself was refused; nothing hit */
#define ZR_RAY_CULL_BACK 1u   /* query flag: BACK hits do not count */
#define ZR_RAY_ANY_HIT   2u   /* query flag: only flags & ZR_RAY_HIT is defined (line of sight); every other field reads as a miss */
#define ZR_RAY_NO_BOUNDS 4u   /* query flag, parity A/B: test every triangle of every shown instance, no sphere or box rejects anything */
/* n rays, n records (bytes == n * 48).  Calls zr_finish first and passes its error on.  ZR_ERR_ARG: n > 0 with a null pointer, a wrong
 * byte count, an unknown flag bit, n above 2^24; then ZR_ERR_STATE: no finished frame enqueued (also after zr_resize until the next
 * frame), the scene changed after the last frame, between the stages of a frame; then n == 0: ZR_OK. */
int  zr_raycast(zr_ctx* ctx, const zr_ray* rays, uint32_t n, uint32_t flags, zr_ray_hit* hits, size_t bytes);
/* The same from and into caller-owned DEVICE buffers (16-byte aligned, else ZR_ERR_ARG), stream-ordered on the render stream behind the
 * frame enqueued last and ahead of whatever the next zr_render puts there, with no host sync (the first cast after the object list
 * changed builds a small table and drains once).  The frame after next, which rewrites what this launch reads, waits for it. */
int  zr_raycast_async(zr_ctx* ctx, const void* rays_dev, uint32_t n, uint32_t flags, void* hits_dev);
/* The world-space ray of the uniforms set last through frame position (px, py) - pixel centres at +0.5, the camera pass's viewport
 * mapping: origin on the near plane, dir = the far-plane point minus the origin, t_min = 0, t_max = 1; float64 from the inverse of
 * Proj * View, rounded once.  ZR_ERR_STATE without uniforms or when Proj * View has no inverse. */
int  zr_camera_ray(zr_ctx* ctx, float px, float py, zr_ray* out);
/* The rule on the host, context-free: n_rays rays against n_tris triangles of 9 floats (A, B, C), primitive id = the triangle's
 * index; a hit's object and instance are 0.  Either count may be 0. */
int  zr_ray_triangles(const zr_ray* rays, uint32_t n_rays, const float* tris /* 9 floats each */, uint32_t n_tris,
                      uint32_t flags, zr_ray_hit* hits);

/* --- multi-GPU screen-tile partition --- */
/* Owner of tile (tx, ty) in a world of `world` ranks, and the list of tiles a rank owns in increasing tile index (= its slot order
 * in the packed buffer); slots_per_rank = the largest count over all ranks (every rank contributes that many slots to the all-gather).
 * Context-free; owned may be NULL. */
uint32_t zr_tile_owner(uint32_t tx, uint32_t ty, uint32_t world);
int  zr_tile_partition(uint32_t width, uint32_t height, uint32_t world, uint32_t rank, uint32_t* owned, uint32_t* n_owned,
                       uint32_t* slots_per_rank);
/* Shadow pass split: this context draws instances i % world == rank into its shadow map; the caller min-reduces the maps
 * (depth test LESS_OR_EQUAL = min) between zr_render_shadow and zr_render_lighting.  Default 0 / 1 = everything. */
int  zr_set_shadow_partition(zr_ctx* ctx, uint32_t rank, uint32_t world);
/* Shadow pass split, second form: the MAP is owned by light-space super-tiles (zr_tile_owner on the map's 32 x 32-texel tiles) the way
 * the frame is owned by screen super-tiles.  This context then draws only the casters whose texel box can reach a tile it owns - whole,
 * so its owned tiles equal the single-GPU map's bit for bit; the ranks exchange tiles with ONE all-gather and nothing is reduced:
 *   zr_render_geometry | zr_shadow_pack -> all-gather of world x zr_shadow_tiles_bytes -> zr_shadow_unpack | zr_render_lighting
 * (zr_tile_partition(shadow_dim, shadow_dim, world, rank, ...) lists the owned tiles = the slots of the packed buffer; unused slots hold
 * depth 1.0.)  Replaces nothing in the reference (one device, ZE:2241); the pass it shards is ZE:3239-3393.  Default 0 / 1 = the whole map.
 * hip_stream NULL = the render stream. */
int  zr_set_shadow_tiles(zr_ctx* ctx, uint32_t rank, uint32_t world);
int  zr_shadow_tiles_bytes(zr_ctx* ctx, size_t* bytes_per_rank);
int  zr_shadow_pack(zr_ctx* ctx, void* packed_dev, void* hip_stream);
int  zr_shadow_unpack(zr_ctx* ctx, const void* gathered_dev, void* hip_stream);
/* Caller-owned shadow map, float[shadow_dim^2] device memory (NULL = internal). */
int  zr_set_shadow_buffer(zr_ctx* ctx, void* dev_ptr);
/* Packed tile-major RGBA8 of the tiles this rank owns.  The caller's to READ: on a single-rank ZR_FLAG_PACKED_TILES context a resting
 * frame leaves the settled parts of it as they stand (see zr_render); a caller who writes tiles gives the library a buffer of its own
 * (zr_set_tiles_buffer).  A device pointer, stable until zr_destroy or a zr_resize. */
int  zr_tiles_device_buffer(zr_ctx* ctx, void** dev_ptr, size_t* bytes_per_rank);
/* Caller-owned packed buffer for the following frames (same size; NULL = the internal one).  Two alternating buffers let
 * frame k's all-gather overlap frame k+1's rendering. */
int  zr_set_tiles_buffer(zr_ctx* ctx, void* dev_ptr);
int  zr_read_tiles(zr_ctx* ctx, uint8_t* dst, size_t bytes);             /* host copy of that buffer (tests) */
/* Scatter the all-gathered buffer (tile_world * bytes_per_rank, rank-major, device pointer) into the frame. */
int  zr_composite(zr_ctx* ctx, const void* gathered_dev);
/* The row-major frame.  The caller may write through it: from this call on the context's resting frames write every pixel again (see
 * zr_render). */
int  zr_color_device_ptr(zr_ctx* ctx, void** dev_ptr);                  /* (stable until zr_destroy or a zr_resize) */

/* --- native multi-GPU host: one process per GPU, RCCL over xGMI called by the library itself (no Python, no torch in the frame) ---
 * rank 0 makes the id (zr_dist_unique_id: 128 bytes, ncclGetUniqueId) and hands it to the other ranks by any means; every rank then
 * calls zr_dist_init on a context created with the matching tile_rank / tile_world.  zr_dist_frame enqueues one frame:
 *   render stream + camera lane: the frame of this rank's tiles into packed buffer k & 1
 *   collective stream: ncclAllGather of the packed RGBA8 tiles (4 B per pixel of the frame in total) -> untile into the frame,
 *   overlapped with the rendering of frame k + 1 (buffers are double-buffered, ordering is by events).
 * The all-gather of the composite is the ONLY collective, unless ZR_DIST_SPLIT_SHADOW is given: then each rank rasterises the shadow
 * casters i % world == rank and the 1024^2 maps are reduced with ncclAllReduce(min) next to the camera passes.
 * zr_finish / the read-back entry points wait for the collective stream too.  librccl is loaded on first use (dlopen). */
#define ZR_DIST_SPLIT_SHADOW 1u
/* ... or ZR_DIST_SHADOW_TILES: the shadow MAP is owned by light-space super-tiles (zr_set_shadow_tiles) and the second collective is an
 * ncclAllGather of the packed shadow tiles (4 MiB in total for a 1024^2 map, no reduction), between the shadow pass and the lighting pass. */
#define ZR_DIST_SHADOW_TILES 2u
int  zr_dist_unique_id(void* id, size_t bytes);                       /* bytes must be 128 */
int  zr_dist_init(zr_ctx* ctx, const void* id, size_t bytes, uint32_t rank, uint32_t world, uint32_t dist_flags);
/* The same bring-up in two steps, for hosts that can agree between them: zr_dist_prepare is LOCAL (librccl, collective stream, packed /
 * gathered buffers) and may fail on one rank alone; zr_dist_connect calls ncclCommInitRank, which is itself a collective - a rank that
 * never reaches it leaves the others blocked inside it - so call it only after every rank reported a successful prepare.
 * zr_dist_init = prepare + connect.  A failed connect leaves a plain single-context renderer behind (whole shadow map). */
int  zr_dist_prepare(zr_ctx* ctx, uint32_t rank, uint32_t world, uint32_t dist_flags);
int  zr_dist_connect(zr_ctx* ctx, const void* id, size_t bytes);
int  zr_dist_frame(zr_ctx* ctx);
/* The composite of the frame zr_dist_frame enqueued last, copied into a caller-owned DEVICE buffer (W*H*4 bytes of RGBA8) in the order of
 * the collective stream: behind that frame's all-gather + untile, ahead of the next frame's - zr_copy_frame_async for a multi-GPU host
 * that keeps frames in flight (a presenting rank, a test that checks EVERY frame of a pipelined sequence). */
int  zr_dist_copy_frame_async(zr_ctx* ctx, void* color_dev);

/* --- world JSON + livelink (replaces XkWorld::Load ZE:1051-1147, socket thread ZE:1617-1710) --- */
/* A Profab is the engine's asset bundle `Profabs/<name>/{models, textures}` (ZE:4922-5000).  Either the caller registers each
 * model of a Profab (mesh + 7-texture material) under its name, or - after zr_set_asset_root - zr_world_load_json finds
 * `Profabs/<name>` on disk itself.  Unknown names draw nothing, like a missing directory. */
int  zr_profab_register(zr_ctx* ctx, const char* name, uint32_t mesh_id, const zr_material* mat);

/* --- the content tree (replaces ASSETS()/AssetPathSearch ZE:7173-7263, LoadMeshAsset ZE:6899-6948, LoadTextureAsset ZE:6882-6896,
 *     LoadMeshletAsset ZE:7046-7169, the Profab walk ZE:4922-5000 and the world's sky / cubemap / background overrides ZE:4147-4183) --- */
/* dir = the engine's working directory (holds Profabs/ and Content/); NULL switches file-system lookups off again.  With a root
 * set, zr_world_load_json also applies OverrideCubemap / OverrideSkydome (mesh: Content/Models/skydome.obj) / OverrideBackground. */
int  zr_set_asset_root(zr_ctx* ctx, const char* dir);
/* literal path -> Profabs/<set>/{models,textures} -> Content/<set>/...; returns the input (rooted) when nothing is found */
int  zr_asset_path_search(zr_ctx* ctx, const char* name, char* dst, size_t cap, size_t* len);
/* context-free loaders (host code only).  NULL outputs = size query (*nv / *ni, or *w / *h, are set). */
int  zr_load_obj(const char* path, XkVertex* v, uint32_t* nv, uint32_t* idx, uint32_t* ni);
int  zr_load_png_rgba8(const char* path, uint8_t* dst, size_t cap, uint32_t* w, uint32_t* h);
/* `.meshlet` file (ZM:52-75) -> mesh with the file's meshlets attached (zr_mesh_create + zr_mesh_set_meshlets) */
int  zr_load_meshlet_file(zr_ctx* ctx, const char* path, uint32_t* mesh_id);
/* XkWorld::Load() / Save() on a file (NULL = "Content/World.json", ZE:1027), relative to the asset root */
int  zr_world_load_file(zr_ctx* ctx, const char* path);
int  zr_world_save_file(zr_ctx* ctx, const char* path);
/* per-frame UpdateWorld + UpdateUniformBuffer from the loaded world's camera and lights (ZE:4294-4308, 4585-4664) */
int  zr_world_update_uniforms(zr_ctx* ctx, float roll_stage, float roll_light, float time);
/* XkWorld::Load + CreateEngineScene + the first UpdateUniformBuffer: replaces the scene's objects (InstanceCount > 1 ->
 * GenerateInstance, seeded PCG32(1234 + object index)) and sets camera + lights. */
int  zr_world_load_json(zr_ctx* ctx, const char* utf8, size_t len);
int  zr_world_get_camera(zr_ctx* ctx, zr_camera* out);
int  zr_world_save_json(zr_ctx* ctx, char* dst, size_t cap, size_t* len);
/* Context-free Load -> Save (pure host code, no GPU): validates a payload; on error dst receives the message. */
int  zr_world_json_normalize(const char* utf8, size_t len_in, char* dst, size_t cap, size_t* len);
/* Listens on loopback by default (the payload is unauthenticated); any != 0 selects the engine's wildcard bind (AI_PASSIVE,
 * ZE:1630-1636).  Call before zr_livelink_serve.  A client that connects and stays silent is dropped after 2 s. */
int  zr_livelink_bind_any(zr_ctx* ctx, int any);
int  zr_livelink_serve(zr_ctx* ctx, uint16_t port);   /* port 0 = ephemeral (tests); the engine's port is 8080 */
int  zr_livelink_port(zr_ctx* ctx, uint16_t* port);
int  zr_livelink_poll(zr_ctx* ctx, int* reloaded);  /* DrawFrame's bReloadScene pickup, ZE:1943-1951 */
int  zr_livelink_stop(zr_ctx* ctx);

/* --- a world applied as a difference ("Reloading a world") ---
 * zr_world_update_json changes only what differs from the live scene.  Afterwards everything observable - every frame byte for byte,
 * covered_pixels / covered_shadow_texels, object order and count, zr_object_get_instances, zr_object_get_visibility (everything shown),
 * the identities of zr_read_ids / zr_pick / zr_instance_coverage (ZR_ERR_STATE until the next frame, as after a load),
 * zr_world_save_json, zr_world_get_camera - equals that of a NEW context of the same configuration, registered Profabs and asset root
 * after zr_world_load_json of the same payload.  Only the time differs, and what the frame loop keeps: objects and their textures on the
 * device, the visibility history, the work lists, the record plan and the kept shadow map.
 *
 * Files are taken as unchanged while their names are unchanged (the Profab cache assumes that too): an edited image under an old name
 * needs zr_world_load_json.
 *
 * Matching rules.  Every object made by a world load or update remembers where it came from: Profab name, index of the model in that
 * Profab's list, and "material as the Profab gave it" (zr_object_set_texture and zr_object_update_texture_async clear that; objects
 * of zr_object_add have no such record and are dropped, as a load drops them).  The target list is the one a load would build: the
 * payload's Objects in order, each Profab's models in order, instances from GenerateInstance seeded PCG32(1234 + index in Objects) -
 * so inserting or removing an entry re-seeds the later ones, as a load does.  Each target takes the first unused live object of the
 * same (name, model index):
 *   - same instancing and count, host copy of the instances bit-equal and current: kept untouched;
 *   - same count, other values (or values last written by zr_object_update_instances_async): replaced through the instance-update
 *     path of zr_object_set_instances (objects_reinstanced);
 *   - other count, or instanced <-> not instanced: instance buffers and update state re-made, the material's device memory stays
 *     (objects_reinstanced);
 *   - material no longer as the Profab gave it: rebuilt from the Profab (materials_rebuilt).
 * Every kept object is shown again, with every instance; meshes keep what zr_mesh_set_vertices did to them, as across a load.  The
 * objects are put in target order by moving them: no kept object's device memory is copied or freed.  Cubemap, skydome and background
 * are re-read only if their names or flags differ or the host replaced them with zr_set_* since the world named them; one the world no
 * longer names is dropped.  Camera and lights go the way of zr_world_update_uniforms.
 *
 * When nothing but camera or lights differs, scene_changed == 0: the call enqueues, frees and synchronises nothing, and the work lists,
 * the plan, the histories and the kept shadow map stand or fall by their own keys (a payload that moves only MainCamera.Position /
 * Lookat keeps the shadow map; FOV, zNear, zFar or the first directional light redraw it).  When objects are added, removed, resized or
 * reordered the call synchronises, rebuilds the draw table itself and carries the visibility marks and shadow flags of the kept
 * meshlet-instances to their new work-item numbers (history_items).
 *
 * Errors: ZR_ERR_STATE between the stages of a frame; ZR_ERR_PARSE, bad names (ZR_ERR_ARG) and missing files (ZR_ERR_IO) are found
 * before anything is changed, so a refused call leaves the context as it was (Profabs read from disk on the way stay cached).  On a
 * context that never loaded a world the update is a load. */
typedef struct zr_world_delta {
    uint32_t struct_bytes;       /* sizeof as the LIBRARY knows it */
    uint32_t differs;            /* ZR_WORLD_DIFF_* bits of the payload against the live world */
    uint32_t scene_changed;      /* 0: no object, instance, material, sky or background was touched (uniforms at most) */
    uint32_t objects_kept;       /* live objects that stayed, device memory and all (instances bit-equal) */
    uint32_t objects_reinstanced;/* kept material and mesh, instance values or count replaced */
    uint32_t objects_added, objects_removed;
    uint32_t materials_rebuilt;  /* kept objects whose material was rebuilt from the Profab (see rules) */
    uint32_t history_items;      /* meshlet-instances whose visibility / shadow marks were carried to new numbers */
    uint32_t reserved[3];        /* 0 */
} zr_world_delta;
#define ZR_WORLD_DIFF_CAMERA 1u
#define ZR_WORLD_DIFF_LIGHTS 2u
#define ZR_WORLD_DIFF_SKY 4u        /* skydome / cubemap names or flags */
#define ZR_WORLD_DIFF_BACKGROUND 8u
#define ZR_WORLD_DIFF_OBJECTS 16u
/* out may be NULL; bytes = the caller's sizeof(zr_world_delta) (passed like zr_stats: the struct grows only at its end) */
int  zr_world_update_json(zr_ctx* ctx, const char* utf8, size_t len, zr_world_delta* out, size_t bytes);
int  zr_world_update_file(zr_ctx* ctx, const char* path, zr_world_delta* out, size_t bytes);   /* as zr_world_load_file */
/* Context-free, pure host code: which parts of two payloads differ (ZR_WORLD_DIFF_* into *differs); a malformed one: ZR_ERR_PARSE. */
int  zr_world_json_diff(const char* a, size_t len_a, const char* b, size_t len_b, uint32_t* differs);
/* zr_livelink_poll applies payloads with the update instead of the load; default 0 = the load. */
int  zr_livelink_set_incremental(zr_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif /* ZELDA_RENDER_H */
