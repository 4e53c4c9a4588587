// zr_ids.h — object identity of the last frame (zr_set_id_capture, zr_read_ids, zr_pick, zr_instance_coverage): the tables the
// census kernels (zr_ids.hip) read.  Kept apart from ZrPass / ZrObject / GBufferPtrs, so that no existing kernel sees them.
#pragma once

#include "zr_types.h"

// One record per scene draw, in draw order (non-instanced draws, then instanced ones: ZE:3445-3476), plus a sentinel whose prim_base is
// the scene's primitive count.  object = add order, slot_base = that object's first instance slot (zr_instance_coverage).
struct ZrIdsDraw { uint32_t prim_base, n_tris, object, slot_base; };

struct ZrIdsArgs {
    const uint32_t* prim;            // the frame's winner plane (W*H, ZR_EMPTY_PRIM = none)
    const float* depth;              // the same frame's GBuffer target 0
    const ZrIdsDraw* draws; uint32_t n_draws;
    uint32_t W, x0, y0, w, h;        // the rectangle (already clipped to the frame)
    uint32_t* counts;                // per slot: pixels won (zeroed between queries)
    unsigned long long* keys;        // per slot: least depth_bits << 32 | y*W + x (all ones between queries)
    uint32_t* hit_list; uint32_t* n_hits;      // the slots the rectangle touched, in no particular order
    uint2* obj_plane;                // ZR_IDS_OBJECT (W*H)
};

#define ZR_IDS_COVERAGE 0            // counts only
#define ZR_IDS_PICK     1            // counts + nearest pixel + hit list
#define ZR_IDS_OBJECTS  2            // the {object, instance} plane only

void zr_launch_id_census(const ZrIdsArgs& A, int mode, hipStream_t s);
// the listed slots -> zr_hit records (unsorted), and those slots cleared for the next query
void zr_launch_id_hits(const ZrIdsArgs& A, uint32_t n, zr_hit* out, hipStream_t s);
// zr_highlight.hip: the winner plane resolved against the set (a bit per slot) into bit_plane, ceil(W / 64) 64-bit words per row; and
// `frame` (16-byte aligned) outlined and filled by it into dst (4-byte aligned), both W x H
void zr_launch_highlight_mask(const uint32_t* prim_plane, const ZrIdsDraw* draws, uint32_t n_draws, const uint32_t* set_bits, unsigned long long* bit_plane, uint32_t W,
                              uint32_t H, hipStream_t st);
void zr_launch_highlight_apply(const uint32_t* frame, const unsigned long long* bit_plane, uint32_t* dst, uint32_t W, uint32_t H, const zr_highlight_style& style,
                               hipStream_t st);

// zr_raycast.hip: casting rays (zr_raycast.h has the rule).  rays / hits: n_rays records each, 16-byte aligned; objs: the draw table of
// the frame enqueued last, of which the first n_draws records are the scene's (the skydome's, last, is never visited) with n_inst
// instances over all of them; draws: the census's table (draw order -> add order); M, m_scale: that frame's model matrix and the
// bound of its stretch (ZrPass::M, m_scale); flags: ZR_RAY_*, the query's
struct ZrRayArgs {
    const zr_ray* rays; zr_ray_hit* hits;
    const ZrObject* objs; const ZrIdsDraw* draws;
    uint32_t n_rays, n_draws, n_inst, flags;
    float M[16]; float m_scale;
};
void zr_launch_raycast(const ZrRayArgs& A, hipStream_t s);

// zr_wire.hip: the wireframe (zr_wire.h has the rule).  frame (W x H, row-major RGBA8) with the edges of each pixel's winner drawn over
// it into dst (4-byte aligned); prim, draws, n_draws: the census's (ZrIdsArgs); objs: the draw table of the frame enqueued last, in the
// same draw order; set_bits: the highlight's bitset for a selected-only style, else null; PVM, hw, hh: that frame's camera block;
// colour: zr_hl_pack of the style's; tiles_x: the launcher's
struct ZrWireArgs {
    const uint32_t* frame; const uint32_t* prim; uint32_t* dst;
    const ZrIdsDraw* draws; const ZrObject* objs; const uint32_t* set_bits;
    uint32_t n_draws, W, H, tiles_x, colour, width_256;
    float PVM[16]; float hw, hh;
};
void zr_launch_wire_apply(const ZrWireArgs& A, hipStream_t s);
