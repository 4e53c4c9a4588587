// zr_wire.hip — k_wire_apply: the wireframe of the visible triangles drawn over a delivered frame (zelda_render.h, "wireframe";
// DESIGN.md section 5, "Wireframe"; zr_wire.h has the rule).  One launch on the render stream behind the lighting pass.
// A 256-thread workgroup takes eight rows of a 32 x 32 tile, a thread per pixel, row-major: a wave's loads and stores are two whole
// 128-byte row segments.  Per wave: the winners are read and the candidates balloted (a scene primitive - and, for a selected-only
// style, one whose slot's bit is in the highlight set); a wave without one copies its pixels and is done.  Else primitive -> draw ->
// instance -> triangle as the census does (zr_ids_dev.h, one search for the wave in the common case), then per candidate lane the
// vertex part of pixel_geom (zr_surface.h) - the first 16 bytes of the three corner records at rtris + 3 tri + k, the instance record,
// zr_mat4_point(PVM, vs_position(..)), its very expressions - the rule, the blend, the store.  No per-block set-up of distinct
// triangles: neighbouring lanes' loads of the same records hit the cache (DESIGN.md section 9 item 3 has what such a scheme bought the
// resolve: nothing).
// Nothing is loaded beyond x < W, y < H of the frame or the winner plane.  In a wave with a candidate every lane reads the draw record
// it was given (a lane without a winner: the first candidate's) and, for a selected-only style, that slot's word of the bitset - valid
// addresses both; the scene's own data - the draw table's record, corner records, instance record - is loaded by candidates alone.
// Nothing is stored beyond the destination's W * H pixels.  No atomics, no LDS, no scratch, ordinary vector loads and stores; 42 VGPRs
// and 44 SGPRs: 8 waves per SIMD (the float64 edge values do not cost the eighth).
#include "zr_dev.h"
#include "zr_ids_dev.h"
#include "zr_wire.h"

__global__ __launch_bounds__(256) void k_wire_apply(ZrWireArgs A)
{
    const uint32_t tile = blockIdx.x >> 2, ty0 = tile / A.tiles_x, t = threadIdx.x;
    const uint32_t x = (tile - ty0 * A.tiles_x) * kZrHlTile + (t & 31u), y = ty0 * kZrHlTile + (blockIdx.x & 3u) * 8u + (t >> 5);
    const bool inside = x < A.W && y < A.H;
    const size_t p = (size_t)y * A.W + x;
    uint32_t prim = ZR_EMPTY_PRIM, px = 0u;
    if (inside) { prim = A.prim[p]; px = A.frame[p]; }
    bool cand = ids_scene_prim(A.draws, A.n_draws, prim);
    const unsigned long long hm = __ballot(cand);
    if (hm != 0ull) {                                        // (wave-uniform)
        const uint32_t d = ids_wave_draw(A.draws, A.n_draws, prim, cand, hm);
        const ZrIdsDraw D = A.draws[d];
        const uint32_t local = ids_local(D, prim, cand), inst = ids_instance(D, local), tri = local - inst * D.n_tris;
        if (A.set_bits) {                                    // a selected-only style
            const uint32_t slot = D.slot_base + inst;
            cand = cand && ((A.set_bits[slot >> 5] >> (slot & 31u)) & 1u) != 0u;
        }
        if (cand) {
            const ZrObject* __restrict__ O = A.objs + d;
            const bool instanced = O->instanced != 0u;
            const float4* __restrict__ rv = (const float4*)(O->rtris + 3u * (size_t)tri);      // 32-byte records: position.xyz u | normal.xyz v
            const float4 q0 = ld_global(rv), q1 = ld_global(rv + 2), q2 = ld_global(rv + 4);
            const ZrInstance I = ld_record(O->inst + inst);
            const zf4 c0 = zr_mat4_point(A.PVM, vs_position(zr3(q0.x, q0.y, q0.z), I, instanced));
            const zf4 c1 = zr_mat4_point(A.PVM, vs_position(zr3(q1.x, q1.y, q1.z), I, instanced));
            const zf4 c2 = zr_mat4_point(A.PVM, vs_position(zr3(q2.x, q2.y, q2.z), I, instanced));
            const float c[9] = { c0.x, c0.y, c0.w, c1.x, c1.y, c1.w, c2.x, c2.y, c2.w };
            if (zr_wire_on(c, (double)A.hw, (double)A.hh, x, y, A.width_256)) px = zr_hl_blend_px(px, A.colour);
        }
    }
    if (inside) A.dst[p] = px;
}

// grid: four workgroups per tile, tiles row-major (A.tiles_x is set here)
void zr_launch_wire_apply(const ZrWireArgs& args, hipStream_t st)
{
    ZrWireArgs A = args;
    A.tiles_x = (A.W + kZrHlTile - 1u) / kZrHlTile;
    const uint32_t tiles_y = (A.H + kZrHlTile - 1u) / kZrHlTile;
    if (A.W == 0u || A.H == 0u) return;
    hipLaunchKernelGGL(k_wire_apply, dim3(A.tiles_x * tiles_y * 4u), dim3(256), 0, st, A);
}
