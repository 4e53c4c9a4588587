// zr_wire.h — the wireframe of the visible triangles in a delivered frame (zelda_render.h, "wireframe"; DESIGN.md section 5,
// "Wireframe"): the ONE statement of the rule, the style check and the host statement over a whole frame, which the kernel
// (zr_wire.hip), the host function (zr_frame_wire) and a stand-alone program (tests/wire_check.cpp, under the sanitizers) all call.
// Plain C++ and nothing of HIP.  Contraction is off in every floating-point function here, no sqrt, no division.
//
// A pixel (x, y) was won by a triangle with the clip-space corners c0, c1, c2: float32 (x, y, w) each, the camera pass's own values.
// Everything from there on is float64.
//   screen     Hk = (hw (xk + wk), hh (yk + wk), wk), hw = W / 2, hh = H / 2: the corner in homogeneous pixel coordinates (the sum of
//              the two floats is exact in float64, the product is rounded once)
//   edge       for (a, b) = (0, 1), (1, 2), (2, 0):  l = Ha x Hb,
//                lx = Hay Hbw - Haw Hby,  ly = Haw Hbx - Hax Hbw,  lz = Hax Hby - Hay Hbx      each product rounded, then the difference
//   test       s = (lx (x + 0.5) + ly (y + 0.5)) + lz,  n2 = lx lx + ly ly,  r = width_256 / 512
//              on the wire iff for some edge  n2 > 0  and  s s <= (r r) n2;  a NaN anywhere compares false
// s / sqrt(n2) is the distance, in pixels, from the pixel's centre to the edge's LINE.  A homogeneous line does not care for the sign of
// w: the rule holds for corners behind the eye, one rule for triangles the camera pass drew on its fast path and on its clip path.
// Why the line is enough: the pixel was won by this triangle, so its centre lies inside it (or within the rasteriser's snap of it).
// Inside a triangle an edge's line and its segment are equally far except beyond an obtuse corner, where the line reaches further than
// the segment by less than r: the wire is at most that much longer there, still on the triangle's own pixels.
// Two coincident projected corners give n2 = 0: no wire from that edge.
// A pixel on the wire has R, G, B blended with the style's colour at its opacity (zr_highlight.h's blend, not a second one); A stays.
//
// Not done: anti-aliased edges (a pixel is on the wire or not), hidden-line "x-ray" wires, suppressing the diagonals of quads, rank
// contexts (tile_world > 1).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "zr_highlight.h"                    // the blend; zelda_render.h: zr_wire_style, ZR_WIRE_*

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_WR_FN __host__ __device__ static inline
#else
#define ZR_WR_FN static inline
#endif

static_assert(sizeof(zr_wire_style) == 16, "one 16-byte word");

ZR_WR_FN bool zr_wire_style_ok(const zr_wire_style* s)
{
    return s->width_256 >= 1u && s->width_256 <= ZR_WIRE_WIDTH_MAX && (s->flags & ~ZR_WIRE_SELECTED) == 0u && s->reserved == 0u;
}
ZR_WR_FN zr_wire_style zr_wire_style_default() { return zr_wire_style{ { 0, 0, 0, 255 }, 256u, 0u, 0u }; }

// A corner in homogeneous pixel coordinates
struct ZrWireH { double x, y, w; };
ZR_WR_FN ZrWireH zr_wire_corner(float cx, float cy, float cw, double hw, double hh)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double sx = (double)cx + (double)cw, sy = (double)cy + (double)cw;
    ZrWireH h;
    h.x = hw * sx; h.y = hh * sy; h.w = (double)cw;
    return h;
}

// The pixel centre (px, py) against the line of the edge a -> b; r2 = r r
ZR_WR_FN bool zr_wire_edge(const ZrWireH& a, const ZrWireH& b, double px, double py, double r2)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double p0 = a.y * b.w, p1 = a.w * b.y, p2 = a.w * b.x, p3 = a.x * b.w, p4 = a.x * b.y, p5 = a.y * b.x;
    const double lx = p0 - p1, ly = p2 - p3, lz = p4 - p5;
    const double sx = lx * px, sy = ly * py, sxy = sx + sy, s = sxy + lz;
    const double nx = lx * lx, ny = ly * ly, n2 = nx + ny;
    const double ss = s * s, lim = r2 * n2;
    return n2 > 0.0 && ss <= lim;
}

// c: x, y, w of the three corners (9 floats).  Edge order (0,1), (1,2), (2,0).
ZR_WR_FN bool zr_wire_on(const float* c, double hw, double hh, uint32_t x, uint32_t y, uint32_t width_256)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const ZrWireH h0 = zr_wire_corner(c[0], c[1], c[2], hw, hh), h1 = zr_wire_corner(c[3], c[4], c[5], hw, hh), h2 = zr_wire_corner(c[6], c[7], c[8], hw, hh);
    const double px = (double)x + 0.5, py = (double)y + 0.5, r = (double)width_256 / 512.0, r2 = r * r;      // (a power of two: the quotient is exact)
    return zr_wire_edge(h0, h1, px, py, r2) || zr_wire_edge(h1, h2, px, py, r2) || zr_wire_edge(h2, h0, px, py, r2);
}

// The host statement: rgba8 and prim are width x height, row-major; corners 9 floats per primitive; a winner at or above n_prims is no
// triangle; selected: n_prims bytes, read only with ZR_WIRE_SELECTED in the style, or null (every primitive is a candidate).  Reads
// nothing beyond rgba8[width * height * 4), prim[width * height), corners[n_prims * 9) and selected[n_prims), writes nothing beyond
// dst[width * height * 4).
static inline void zr_wire_frame(const uint8_t* rgba8, const uint32_t* prim, uint32_t width, uint32_t height, const float* corners, uint32_t n_prims,
                                 const uint8_t* selected, const zr_wire_style* s, uint8_t* dst)
{
    const uint32_t colour = zr_hl_pack(s->rgba);
    const bool only = (s->flags & ZR_WIRE_SELECTED) != 0u && selected != nullptr;
    const double hw = 0.5 * (double)width, hh = 0.5 * (double)height;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const uint32_t p = prim[i];
            const uint8_t* q = rgba8 + i * 4u;
            uint32_t px = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            if (p < n_prims && (!only || selected[p]) && zr_wire_on(corners + (size_t)p * 9u, hw, hh, x, y, s->width_256)) px = zr_hl_blend_px(px, colour);
            uint8_t* o = dst + i * 4u;
            o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16); o[3] = (uint8_t)(px >> 24);
        }
}
