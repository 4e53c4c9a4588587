// zr_highlight.h — highlighting a selection in a delivered frame (zelda_render.h, "highlighting a selection"; DESIGN.md section 5,
// "Highlighting a selection"): the ONE statement of the blend, the style check, the per-pixel decision and the window of mask bits a
// tile dilates, which the kernels (zr_highlight.hip), the host function (zr_frame_highlight) and a stand-alone program
// (tests/highlight_check.cpp, under the sanitizers) all call.  Plain C++ and nothing of HIP.
//
// Everything is integer arithmetic.  M(x, y) = 1 where the frame's winner is a scene primitive of a highlighted slot, 0 elsewhere and
// outside the frame.  With r = the style's radius: a pixel with M = 1 has R, G, B blended with `fill`; a pixel with M = 0 and some M = 1
// within |dx| <= r, |dy| <= r has them blended with `outline`; any other pixel, and every A, stays.
//   blend(p, q, a) = floor((p (255 - a) + q a + 127) / 255)         the nearest integer of the mix (255 is odd: no tie), <= 65 152 inside
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/zelda_render.h"      // zr_highlight_style

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_HL_FN __host__ __device__ static inline
#else
#define ZR_HL_FN static inline
#endif

constexpr uint32_t kZrHlRadiusMax = 8u;          // the widest outline
constexpr uint32_t kZrHlTile = 32u;              // k_highlight_apply's tile, and the side of its window less 2 r

// x / 255 rounded to nearest for x = p (255 - a) + q a, 0 <= x <= 65 025, by shifts: t = x + 128, (t + (t >> 8)) >> 8
// (tests/test_highlight_cpu.py holds it to floor((x + 127) / 255) for every such x)
ZR_HL_FN uint32_t zr_hl_div255(uint32_t x) { const uint32_t t = x + 128u; return (t + (t >> 8)) >> 8; }
ZR_HL_FN uint32_t zr_hl_blend(uint32_t p, uint32_t q, uint32_t a) { return zr_hl_div255(p * (255u - a) + q * a); }

// A style's colour as the kernels take it: R in the low byte, the opacity in the high one
ZR_HL_FN uint32_t zr_hl_pack(const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24); }

// A pixel as the frame holds it (R in the low byte) with R, G, B blended with `colour` at its opacity; A stays
ZR_HL_FN uint32_t zr_hl_blend_px(uint32_t px, uint32_t colour)
{
    const uint32_t a = colour >> 24;
    return zr_hl_blend(px & 255u, colour & 255u, a) | (zr_hl_blend((px >> 8) & 255u, (colour >> 8) & 255u, a) << 8) |
           (zr_hl_blend((px >> 16) & 255u, (colour >> 16) & 255u, a) << 16) | (px & 0xFF000000u);
}

// The per-pixel decision: m = the pixel's M, near = some M = 1 within the radius (the pixel's own included)
ZR_HL_FN uint32_t zr_hl_pixel(uint32_t px, bool m, bool near, uint32_t fill, uint32_t outline)
{
    return m ? zr_hl_blend_px(px, fill) : near ? zr_hl_blend_px(px, outline) : px;
}

ZR_HL_FN bool zr_hl_style_ok(const zr_highlight_style* s) { return s->radius <= kZrHlRadiusMax && s->reserved == 0u; }
ZR_HL_FN zr_highlight_style zr_hl_style_default() { return zr_highlight_style{ { 255, 160, 0, 255 }, { 255, 160, 0, 0 }, 2u, 0u }; }

// The bit plane: ceil(W / 64) 64-bit words per row, bit (x & 63) of word x >> 6 = M(x, y); the last word's upper bits are 0
ZR_HL_FN uint32_t zr_hl_row_words(uint32_t W) { return (W + 63u) / 64u; }

// A tile's window of one row: bit j = M(x0 - r + j, y) for j = 0 .. 31 + 2 r, the bits above that 0; x0 a multiple of 32, r <= 8.
// The 48 bits at most lie in two neighbouring words of the plane's row: with x0 on a word boundary (half = 0) the r bits ahead of it
// are the top of the word before (lo) and the rest the bottom of its own (hi); with x0 in the middle of a word (half = 1) all but the
// last r come from its own word (lo) and those from the word behind (hi).  The caller passes 0 for a word outside the row.  No shift
// count is negative or reaches 64: r = 0 on a boundary would shift lo by 64 and takes hi alone.
ZR_HL_FN uint64_t zr_hl_window(uint64_t lo, uint64_t hi, uint32_t half, uint32_t r)
{
    const uint64_t w = half ? (lo >> (32u - r)) | (hi << (32u + r)) : r ? (lo >> (64u - r)) | (hi << r) : hi;
    return w & ((1ull << (kZrHlTile + 2u * r)) - 1ull);
}
// ... dilated along the row: bit j = the OR of the window's bits j - r .. j + r, exact for j = r .. 31 + r, the tile's own pixels
ZR_HL_FN uint64_t zr_hl_dilate_row(uint64_t win, uint32_t r)
{
    uint64_t h = win;
    for (uint32_t d = 1u; d <= r; ++d) h |= (win >> d) | (win << d);
    return h;
}

// The host statement: rgba8 is width x height, row-major; mask a byte per pixel, non-zero = highlighted.  Reads nothing beyond
// rgba8[width * height * 4) and mask[width * height), writes nothing beyond dst[width * height * 4).  (Pixel by pixel from the rule,
// not through the windows: the stand-alone program holds the windows to it.)
static inline void zr_hl_frame(const uint8_t* rgba8, const uint8_t* mask, uint32_t width, uint32_t height, const zr_highlight_style* s, uint8_t* dst)
{
    const uint32_t fill = zr_hl_pack(s->fill), outline = zr_hl_pack(s->outline), r = s->radius;
    for (uint32_t y = 0; y < height; ++y) {
        const uint32_t ya = y > r ? y - r : 0u, yb = y + r < height ? y + r : height - 1u;
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const bool m = mask[i] != 0;
            bool near = m;
            if (!m && r) {
                const uint32_t xa = x > r ? x - r : 0u, xb = x + r < width ? x + r : width - 1u;
                for (uint32_t v = ya; v <= yb && !near; ++v)
                    for (uint32_t u = xa; u <= xb; ++u)
                        if (mask[(size_t)v * width + u]) { near = true; break; }
            }
            const uint8_t* p = rgba8 + i * 4u;
            const uint32_t px = zr_hl_pixel((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24), m, near, fill, outline);
            uint8_t* q = dst + i * 4u;
            q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); q[3] = (uint8_t)(px >> 24);
        }
    }
}
