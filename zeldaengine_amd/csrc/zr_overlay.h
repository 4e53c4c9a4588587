// zr_overlay.h — depth-tested line overlays in a delivered frame (zelda_render.h, "overlaying lines"; DESIGN.md section 5, "Overlaying
// lines"): the ONE statement of a segment's way from its two end points to the pixels it covers, their depth, the test and the blend,
// which the kernels (zr_overlay.hip), the host function (zr_frame_overlay) and a stand-alone program (tests/overlay_check.cpp, under the
// sanitizers) all call.  Plain C++ and nothing of HIP.
//
// A segment, in list order:
//   1 transform   ca, cb = PVM * (p, 1), the expression sequence of zr_mat4_point (zr_math.h); a non-finite component: nothing drawn
//   2 clip        the two-point polygon against near (z >= 0), the four guard-band planes (4 w +- x, 4 w +- y: plane_dist of zr_raster.h,
//                 in its order) and far (w - z >= 0); d >= 0 is inside; both ends outside a plane: nothing; one: it becomes
//                 lerp(in, out, d_in / (d_in - d_out)), lerp4's expression; afterwards w > 0 at both ends, else nothing
//   3 project     project() of zr_dev.h, snap_to_int included: X, Y in 1/256 pixel, z = c.z * (1 / c.w).  X is then clamped to
//                 128 W +- 2^23 and Y to 128 H +- 2^23 (below)
//   4 walk        dX = Xb - Xa, dY = Yb - Ya, both 0: nothing; X-major iff |dX| >= |dY|; the ends swapped so that the major delta is
//                 positive; X-major: every column x in [0, W) with cx = 256 x + 128, Xa <= cx < Xb, gets the row
//                 (Ya + floor((2 (cx - Xa) dY + dX) / (2 dX))) >> 8, skipped outside [0, H); Y-major the mirror image
//   5 depth       t = float(cx - Xa) / float(dX), d = fma(t, zb - za, za) clamped to [min(za, zb), max(za, zb)] (minimumNumber /
//                 maximumNumber: a NaN yields the other operand)
//   6 test+blend  visible iff ZR_OVERLAY_XRAY or (d - depth_bias) <= the frame's depth at the pixel (a NaN compares false: hidden);
//                 visible: zr_hl_blend_px at opacity rgba[3]; hidden: at opacity zr_hl_div255(rgba[3] * hidden_opacity); A stays
// A pixel crossed by several segments takes them in list order.
//
// The bound.  Behind the clip |x|, |y| <= 4 w up to rounding, so a snapped coordinate lies within 4 * 256 * (W / 2) = 512 W of the
// frame's centre 128 W: at most 512 * 8 160 = 4 177 920 at the largest extent zr_create accepts (255 tiles of 32 a side), 8 355 840 in a
// build with ZR_TILE 64 (16 320) - both below 2^23 = 8 388 608, the second by 32 768 units of rounding room.  The clamp to centre +- 2^23
// therefore touches no segment the clip bounded and only defines the rest (a denormal w makes 1 / w infinite and the snap +-2^31).
// With it dX, dY <= 2^24 and 0 <= cx - Xa < dX: both exact in fp32, and every product below is at most 2 * 2^24 * 2^24 + 2^24 < 2^50
// (the walk) or 256 * 2^14 * 2^25 + 2^23 * 2^25 < 2^50 (the kernel's form without a division) - inside int64.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/zelda_render.h"      // zr_overlay_segment, zr_overlay_style
#include "zr_highlight.h"                    // the blend

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_OV_FN __host__ __device__ static inline
#else
#define ZR_OV_FN static inline
#endif

constexpr uint32_t kZrOvTile = 32u;              // k_overlay_apply's tile
constexpr float kZrOvGuard = 4.0f;               // the guard band, multiples of w (ZR_GUARD)
constexpr int32_t kZrOvReach = 1 << 23;          // a snapped coordinate's largest distance from the frame's centre
constexpr uint32_t kZrOvXray = ZR_OVERLAY_XRAY, kZrOvYMajor = 2u, kZrOvNothing = 4u;      // a record's flags

struct ZrOvVec4 { float x, y, z, w; };
// A segment set up: the swapped, snapped ends, their depths, the colour as the blend takes it, the flags above
struct ZrOvRecord { int32_t Xa, Ya, Xb, Yb; float za, zb; uint32_t colour, flags; };
static_assert(sizeof(ZrOvRecord) == 32 && sizeof(zr_overlay_segment) == 32 && sizeof(zr_overlay_style) == 16, "two 16-byte words each; the style is one");
// The pixels a record can touch, inside the frame (x0 <= x1, y0 <= y1)
struct ZrOvBox { int32_t x0, y0, x1, y1; };

ZR_OV_FN bool zr_ov_finite(float f) { return __builtin_fabsf(f) <= 3.402823466e38f; }      // (NaN: false)
ZR_OV_FN bool zr_ov_style_ok(const zr_overlay_style* s)
{
    return s->depth_bias >= 0.0f && zr_ov_finite(s->depth_bias) && s->hidden_opacity <= 255u && s->reserved[0] == 0u && s->reserved[1] == 0u;
}
ZR_OV_FN bool zr_ov_flags_ok(uint32_t flags) { return (flags & ~ZR_OVERLAY_XRAY) == 0u; }

// 1: M * vec4(p, 1), M column-major
ZR_OV_FN ZrOvVec4 zr_ov_point(const float* m, const float* p)
{
    ZrOvVec4 r;
    r.x = __builtin_fmaf(m[8], p[2], __builtin_fmaf(m[4], p[1], m[0] * p[0])) + m[12];
    r.y = __builtin_fmaf(m[9], p[2], __builtin_fmaf(m[5], p[1], m[1] * p[0])) + m[13];
    r.z = __builtin_fmaf(m[10], p[2], __builtin_fmaf(m[6], p[1], m[2] * p[0])) + m[14];
    r.w = __builtin_fmaf(m[11], p[2], __builtin_fmaf(m[7], p[1], m[3] * p[0])) + m[15];
    return r;
}
// 2: the six planes' distances, and the point between an inside and an outside end
ZR_OV_FN float zr_ov_plane(ZrOvVec4 c, int plane)
{
    switch (plane) {
    case 0: return c.z;
    case 1: return __builtin_fmaf(kZrOvGuard, c.w, c.x);
    case 2: return __builtin_fmaf(kZrOvGuard, c.w, -c.x);
    case 3: return __builtin_fmaf(kZrOvGuard, c.w, c.y);
    case 4: return __builtin_fmaf(kZrOvGuard, c.w, -c.y);
    default: return c.w - c.z;
    }
}
ZR_OV_FN ZrOvVec4 zr_ov_lerp(ZrOvVec4 in, ZrOvVec4 out, float t)
{
    ZrOvVec4 r;
    r.x = __builtin_fmaf(t, out.x - in.x, in.x); r.y = __builtin_fmaf(t, out.y - in.y, in.y);
    r.z = __builtin_fmaf(t, out.z - in.z, in.z); r.w = __builtin_fmaf(t, out.w - in.w, in.w);
    return r;
}
// 3: float -> int of a snapped coordinate (NaN -> -2^31), the projection, the clamp
ZR_OV_FN int32_t zr_ov_snap(float f) { return (int32_t)__builtin_fminf(__builtin_fmaxf(f, -2147483648.0f), 2147483520.0f); }
ZR_OV_FN int32_t zr_ov_reach(int32_t v, int32_t centre) { return v < centre - kZrOvReach ? centre - kZrOvReach : v > centre + kZrOvReach ? centre + kZrOvReach : v; }
ZR_OV_FN void zr_ov_project(ZrOvVec4 c, float hw, float hh, int32_t* X, int32_t* Y, float* z)
{
    const float rw = 1.0f / c.w;
    const float nx = c.x * rw, ny = c.y * rw;
    const float xs = __builtin_fmaf(nx, hw, hw), ys = __builtin_fmaf(ny, hh, hh);
    *X = zr_ov_snap(__builtin_floorf(__builtin_fmaf(xs, 256.0f, 0.5f)));
    *Y = zr_ov_snap(__builtin_floorf(__builtin_fmaf(ys, 256.0f, 0.5f)));
    *z = c.z * rw;
}
ZR_OV_FN int32_t zr_ov_min(int32_t a, int32_t b) { return a < b ? a : b; }
ZR_OV_FN int32_t zr_ov_max(int32_t a, int32_t b) { return a > b ? a : b; }

// Steps 1 - 4's set-up of one segment for a W x H frame (hw = W / 2, hh = H / 2 as floats).  false: it draws nothing (R->flags =
// kZrOvNothing); true: *R is the record and *B the box of pixels it can touch.
ZR_OV_FN bool zr_ov_setup(const float* pvm, float hw, float hh, uint32_t W, uint32_t H, const zr_overlay_segment& s, ZrOvRecord* R, ZrOvBox* B)
{
    R->Xa = R->Ya = R->Xb = R->Yb = 0; R->za = R->zb = 0.0f; R->colour = 0u; R->flags = kZrOvNothing;
    B->x0 = B->y0 = 0; B->x1 = B->y1 = -1;
    ZrOvVec4 a = zr_ov_point(pvm, s.a), b = zr_ov_point(pvm, s.b);
    if (!(zr_ov_finite(a.x) && zr_ov_finite(a.y) && zr_ov_finite(a.z) && zr_ov_finite(a.w) && zr_ov_finite(b.x) && zr_ov_finite(b.y) && zr_ov_finite(b.z) &&
          zr_ov_finite(b.w)))
        return false;
    for (int plane = 0; plane < 6; ++plane) {
        const float da = zr_ov_plane(a, plane), db = zr_ov_plane(b, plane);
        const bool ia = da >= 0.0f, ib = db >= 0.0f;
        if (!ia && !ib) return false;
        if (ia && !ib) b = zr_ov_lerp(a, b, da / (da - db));
        else if (ib && !ia) a = zr_ov_lerp(b, a, db / (db - da));
    }
    if (!(a.w > 0.0f) || !(b.w > 0.0f)) return false;
    int32_t Xa, Ya, Xb, Yb;
    float za, zb;
    zr_ov_project(a, hw, hh, &Xa, &Ya, &za);
    zr_ov_project(b, hw, hh, &Xb, &Yb, &zb);
    const int32_t cx = 128 * (int32_t)W, cy = 128 * (int32_t)H;
    Xa = zr_ov_reach(Xa, cx); Xb = zr_ov_reach(Xb, cx); Ya = zr_ov_reach(Ya, cy); Yb = zr_ov_reach(Yb, cy);
    const int32_t dX = Xb - Xa, dY = Yb - Ya;
    if (dX == 0 && dY == 0) return false;
    const bool ymajor = !((dX < 0 ? -dX : dX) >= (dY < 0 ? -dY : dY));
    if ((ymajor ? dY : dX) < 0) {
        int32_t t = Xa; Xa = Xb; Xb = t;
        t = Ya; Ya = Yb; Yb = t;
        const float z = za; za = zb; zb = z;
    }
    // the pixels along the major axis whose centre lies in [a, b): ceil((a - 128) / 256) .. ceil((b - 128) / 256) - 1; across it the
    // walk stays between the two ends
    const int32_t Ma = ymajor ? Ya : Xa, Mb = ymajor ? Yb : Xb, Na = ymajor ? Xa : Ya, Nb = ymajor ? Xb : Yb;
    const int32_t mlim = (int32_t)(ymajor ? H : W) - 1, nlim = (int32_t)(ymajor ? W : H) - 1;
    const int32_t m0 = zr_ov_max((Ma + 127) >> 8, 0), m1 = zr_ov_min(((Mb + 127) >> 8) - 1, mlim);
    const int32_t n0 = zr_ov_max(zr_ov_min(Na, Nb) >> 8, 0), n1 = zr_ov_min(zr_ov_max(Na, Nb) >> 8, nlim);
    if (m0 > m1 || n0 > n1) return false;
    R->Xa = Xa; R->Ya = Ya; R->Xb = Xb; R->Yb = Yb; R->za = za; R->zb = zb;
    R->colour = zr_hl_pack(s.rgba);
    R->flags = (s.flags & kZrOvXray) | (ymajor ? kZrOvYMajor : 0u);
    if (ymajor) { B->x0 = n0; B->x1 = n1; B->y0 = m0; B->y1 = m1; }
    else { B->x0 = m0; B->x1 = m1; B->y0 = n0; B->y1 = n1; }
    return true;
}

// 4 without a division (the kernel's form): does the record cover pixel (x, y)?  floor(N / D) lies in [256 n - Na, 256 (n + 1) - Na) iff
// (256 n - Na) D <= N < (256 (n + 1) - Na) D for D > 0.  *k = the centre's distance from the first end along the major axis, *dm = the
// major delta: what the depth takes.
ZR_OV_FN bool zr_ov_covers(const ZrOvRecord& R, int32_t x, int32_t y, int32_t* k, int32_t* dm)
{
    const bool ymajor = (R.flags & kZrOvYMajor) != 0u;
    const int32_t Ma = ymajor ? R.Ya : R.Xa, Mb = ymajor ? R.Yb : R.Xb, Na = ymajor ? R.Xa : R.Ya, Nb = ymajor ? R.Xb : R.Yb;
    const int32_t cm = 256 * (ymajor ? y : x) + 128, n = ymajor ? x : y;
    if (!(Ma <= cm && cm < Mb)) return false;
    const int64_t dM = (int64_t)Mb - Ma, dN = (int64_t)Nb - Na, kk = (int64_t)cm - Ma;
    const int64_t N = 2 * kk * dN + dM, D = 2 * dM;
    const int64_t lo = (256 * (int64_t)n - Na) * D;
    if (!(lo <= N && N < lo + 256 * D)) return false;
    *k = (int32_t)kk; *dm = (int32_t)dM;
    return true;
}
// 4 with the division (the host's walk): the pixel across the major axis of the pixel m along it (Ma <= 256 m + 128 < Mb)
ZR_OV_FN int32_t zr_ov_walk(const ZrOvRecord& R, int32_t m, int32_t* k, int32_t* dm)
{
    const bool ymajor = (R.flags & kZrOvYMajor) != 0u;
    const int32_t Ma = ymajor ? R.Ya : R.Xa, Mb = ymajor ? R.Yb : R.Xb, Na = ymajor ? R.Xa : R.Ya, Nb = ymajor ? R.Xb : R.Yb;
    const int64_t dM = (int64_t)Mb - Ma, dN = (int64_t)Nb - Na, kk = (int64_t)(256 * m + 128) - Ma;
    const int64_t N = 2 * kk * dN + dM, D = 2 * dM;
    int64_t q = N / D;
    if (N % D != 0 && N < 0) --q;                 // floor: D > 0
    *k = (int32_t)kk; *dm = (int32_t)dM;
    return (int32_t)(((int64_t)Na + q) >> 8);
}
// 5: the line's depth at the centre k of dm along the major axis
ZR_OV_FN float zr_ov_depth(const ZrOvRecord& R, int32_t k, int32_t dm)
{
    const float t = (float)k / (float)dm;
    const float d = __builtin_fmaf(t, R.zb - R.za, R.za);
    return __builtin_fminf(__builtin_fmaxf(d, __builtin_fminf(R.za, R.zb)), __builtin_fmaxf(R.za, R.zb));
}
// 6: the pixel with the segment over it; depth_at = the frame's depth there
ZR_OV_FN uint32_t zr_ov_shade(uint32_t px, float depth_at, float d, uint32_t colour, uint32_t flags, float depth_bias, uint32_t hidden_opacity)
{
    const bool visible = (flags & kZrOvXray) != 0u || (d - depth_bias) <= depth_at;
    const uint32_t a = visible ? colour >> 24 : zr_hl_div255((colour >> 24) * hidden_opacity);
    return zr_hl_blend_px(px, (colour & 0x00FFFFFFu) | (a << 24));
}

// The host statement: rgba8 and depth are width x height, row-major; pvm the frame's proj * view * model, column-major.  Reads nothing
// beyond rgba8[width * height * 4), depth[width * height) and seg[n), writes nothing beyond dst[width * height * 4).
static inline void zr_ov_frame(const uint8_t* rgba8, const float* depth, uint32_t width, uint32_t height, const float* pvm, const zr_overlay_segment* seg, uint32_t n,
                               const zr_overlay_style* style, uint8_t* dst)
{
    const size_t bytes = (size_t)width * height * 4u;
    for (size_t i = 0; i < bytes; ++i) dst[i] = rgba8[i];
    const float hw = 0.5f * (float)width, hh = 0.5f * (float)height;
    for (uint32_t i = 0; i < n; ++i) {
        ZrOvRecord R;
        ZrOvBox B;
        if (!zr_ov_setup(pvm, hw, hh, width, height, seg[i], &R, &B)) continue;
        const bool ymajor = (R.flags & kZrOvYMajor) != 0u;
        const int32_t nlim = (int32_t)(ymajor ? width : height);
        for (int32_t m = ymajor ? B.y0 : B.x0; m <= (ymajor ? B.y1 : B.x1); ++m) {
            int32_t k, dm;
            const int32_t c = zr_ov_walk(R, m, &k, &dm);
            if (c < 0 || c >= nlim) continue;
            const size_t at = ymajor ? (size_t)m * width + (size_t)c : (size_t)c * width + (size_t)m;
            uint8_t* q = dst + at * 4u;
            const uint32_t px = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            const uint32_t out = zr_ov_shade(px, depth[at], zr_ov_depth(R, k, dm), R.colour, R.flags, style->depth_bias, style->hidden_opacity);
            q[0] = (uint8_t)out; q[1] = (uint8_t)(out >> 8); q[2] = (uint8_t)(out >> 16); q[3] = (uint8_t)(out >> 24);
        }
    }
}
