// zr_highlight.hip — highlighting a selection in a delivered frame (zelda_render.h, "highlighting a selection"; DESIGN.md section 5,
// "Highlighting a selection"; zr_highlight.h has the rule).  Two launches on the render stream behind the lighting pass.
//   k_highlight_mask    each pixel's winner resolved once, into one bit.  A wave takes 64 consecutive pixels of a row (256 B of the
//                       winner plane, k_id_census's access pattern), maps primitive -> draw -> instance -> slot as the census does
//                       (zr_ids_dev.h), tests the slot's bit in the set and stores __ballot(selected): one 8-byte store from one
//                       lane, into a plane of ceil(W / 64) words per row.  A lane beyond x < W loads nothing and stays in the wave
//                       with a false predicate, so the last word's upper bits are 0.
//   k_highlight_apply   a 256-thread workgroup per 32 x 32 tile.  A lane per row of the window y0 - r .. y0 + 31 + r builds that
//                       row's bits x0 - r .. x0 + 31 + r from one or two words of the plane (zr_hl_window; rows and words outside
//                       the frame are never loaded and count as 0) and ORs it with itself shifted by -r .. r; after a barrier a lane
//                       per tile row ORs 2 r + 1 of those; after another each thread takes four neighbouring pixels of one row,
//                       decides from its M and dilated bits (zr_hl_pixel), blends and stores.  A tile whose whole window is 0
//                       copies through (workgroup-uniform: __syncthreads_or).
// Nothing is loaded beyond x < W, y < H of the frame or the winner plane, nor beyond ceil(W / 64) * H words of the bit plane; nothing
// is stored beyond the destination's W * H pixels.  No atomics, no scratch, ordinary vector loads and stores; 768 bytes of LDS (512 of
// the three row arrays, the rest the workgroup-wide OR's), 20 VGPRs, 8 waves per SIMD (k_highlight_mask: 12 VGPRs, no LDS).
#include "zr_highlight.h"
#include "zr_ids_dev.h"

// grid: ceil(ceil(W / 64) * H / 4) workgroups of four waves, a wave per word of the bit plane
__global__ __launch_bounds__(256) void k_highlight_mask(const uint32_t* __restrict__ prim_plane, const ZrIdsDraw* __restrict__ draws, uint32_t n_draws,
                                                        const uint32_t* __restrict__ set_bits, unsigned long long* __restrict__ bit_plane, uint32_t W, uint32_t H)
{
    const uint32_t words = zr_hl_row_words(W), g = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (g >= words * H) return;                          // (wave-uniform: a whole wave leaves)
    const uint32_t y = g / words, x = (g - y * words) * 64u + lane;
    uint32_t prim = ZR_EMPTY_PRIM;
    if (x < W) prim = prim_plane[(size_t)y * W + x];
    const bool hit = ids_scene_prim(draws, n_draws, prim);
    const unsigned long long hm = __ballot(hit);
    unsigned long long sel = 0ull;
    if (hm != 0ull) {                                    // (wave-uniform)
        const ZrIdsDraw D = draws[ids_wave_draw(draws, n_draws, prim, hit, hm)];
        const uint32_t slot = D.slot_base + ids_instance(D, ids_local(D, prim, hit));
        sel = __ballot(hit && ((set_bits[slot >> 5] >> (slot & 31u)) & 1u) != 0u);
    }
    if (lane == 0u) bit_plane[g] = sel;
}

// VEC: W % 4 == 0 (the frame's loads are 16 bytes); VST: and dst is on a 16-byte boundary (so are the stores; else 4 bytes per pixel: a
// caller's buffer may be aligned to no more than that).  grid: a workgroup per tile, row-major.
template <bool VEC, bool VST>
__global__ __launch_bounds__(256) void k_highlight_apply(const uint32_t* __restrict__ frame, const unsigned long long* __restrict__ bit_plane, uint32_t* __restrict__ dst,
                                                         uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t r, uint32_t fill, uint32_t outline)
{
    __shared__ uint32_t own[kZrHlTile + 2u * kZrHlRadiusMax];       // per window row: M of the tile's 32 columns
    __shared__ uint32_t wide[kZrHlTile + 2u * kZrHlRadiusMax];      // ... and M dilated along the row
    __shared__ uint32_t near[kZrHlTile];                            // per tile row: M dilated both ways
    const uint32_t t = threadIdx.x, ty0 = blockIdx.x / tiles_x, x0 = (blockIdx.x - ty0 * tiles_x) * kZrHlTile, y0 = ty0 * kZrHlTile;
    const uint32_t rows = kZrHlTile + 2u * r, words = zr_hl_row_words(W);
    uint64_t win = 0ull;
    if (t < rows && y0 + t >= r && y0 + t - r < H) {                // (the window's row t is the frame's row y0 + t - r)
        const unsigned long long* row = bit_plane + (size_t)(y0 + t - r) * words;
        const uint32_t k = x0 >> 6, half = (x0 >> 5) & 1u;
        // half 0: the word ahead of x0's and x0's own; half 1: x0's own and the one behind it - r = 0 needs neither neighbour
        const uint32_t klo = half ? k : k - 1u, khi = klo + 1u;     // (k = 0, half 0: klo wraps and is not below `words`)
        const uint64_t lo = (half || r) && klo < words ? row[klo] : 0ull;
        const uint64_t hi = (!half || r) && khi < words ? row[khi] : 0ull;
        win = zr_hl_window(lo, hi, half, r);
    }
    const bool any = __syncthreads_or(win != 0ull) != 0;            // (the same for the whole workgroup)
    if (any) {
        if (t < rows) { own[t] = (uint32_t)(win >> r); wide[t] = (uint32_t)(zr_hl_dilate_row(win, r) >> r); }
        __syncthreads();
        if (t < kZrHlTile) {
            uint32_t v = 0u;
            for (uint32_t i = 0u; i <= 2u * r; ++i) v |= wide[t + i];
            near[t] = v;
        }
        __syncthreads();
    }
    const uint32_t ty = t >> 3, cx = (t & 7u) * 4u, px = x0 + cx, py = y0 + ty;
    uint4 v = plane_load4<VEC>(frame, W, H, px, py);
    if (any) {
        const uint32_t m = own[ty + r] >> cx, n = near[ty] >> cx;
        v.x = zr_hl_pixel(v.x, m & 1u, n & 1u, fill, outline);
        v.y = zr_hl_pixel(v.y, (m >> 1) & 1u, (n >> 1) & 1u, fill, outline);
        v.z = zr_hl_pixel(v.z, (m >> 2) & 1u, (n >> 2) & 1u, fill, outline);
        v.w = zr_hl_pixel(v.w, (m >> 3) & 1u, (n >> 3) & 1u, fill, outline);
    }
    plane_store4<VST>(dst, W, H, px, py, v);
}

// The frame's winner plane resolved against the set into bit_plane (ceil(W / 64) * H words), on st
void zr_launch_highlight_mask(const uint32_t* prim_plane, const ZrIdsDraw* draws, uint32_t n_draws, const uint32_t* set_bits, unsigned long long* bit_plane, uint32_t W,
                              uint32_t H, hipStream_t st)
{
    const uint32_t waves = zr_hl_row_words(W) * H;
    hipLaunchKernelGGL(k_highlight_mask, dim3((waves + 3u) / 4u), dim3(256), 0, st, prim_plane, draws, n_draws, set_bits, bit_plane, W, H);
}

// `frame` (W x H, row-major RGBA8, 16-byte aligned) highlighted by bit_plane and the style into dst (W x H, 4-byte aligned), on st
void zr_launch_highlight_apply(const uint32_t* frame, const unsigned long long* bit_plane, uint32_t* dst, uint32_t W, uint32_t H, const zr_highlight_style& style,
                               hipStream_t st)
{
    const uint32_t tiles_x = (W + kZrHlTile - 1u) / kZrHlTile, tiles_y = (H + kZrHlTile - 1u) / kZrHlTile;
    const uint32_t fill = zr_hl_pack(style.fill), outline = zr_hl_pack(style.outline), r = style.radius;
    const dim3 grid(tiles_x * tiles_y), block(256);
    if (W % 4u != 0u) hipLaunchKernelGGL((k_highlight_apply<false, false>), grid, block, 0, st, frame, bit_plane, dst, W, H, tiles_x, r, fill, outline);
    else if ((uintptr_t)dst % 16u != 0u) hipLaunchKernelGGL((k_highlight_apply<true, false>), grid, block, 0, st, frame, bit_plane, dst, W, H, tiles_x, r, fill, outline);
    else hipLaunchKernelGGL((k_highlight_apply<true, true>), grid, block, 0, st, frame, bit_plane, dst, W, H, tiles_x, r, fill, outline);
}
