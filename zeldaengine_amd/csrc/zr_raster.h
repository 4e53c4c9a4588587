// zr_raster.h — the rasteriser proper: exact integer edge functions with the top-left rule over a tile's LDS keys (raster_sub), the
// near-plane / guard-band clipper (raster_clipped), and the steps every kernel that owns a tile's keys takes: the tile's context
// (tile_ctx), a queued or recorded triangle (tri_unpack), the keys' clear and merge (keys_clear, keys_merge), the slow-triangle record
// (slow_read), the claim of a persistent workgroup's next unit (claim_unit).  Shared by the shadow pass (zr_shadow.hip)
// and the camera pass (zr_camera.hip).  Raster state: ZE:5094-5201, 3247-3287; rules: DESIGN.md §4.
#pragma once
#include "zr_dev.h"

struct TileCtx {
    int px0, py0;                 // tile origin in pixels
    int W, H;                     // target extent
};

// Cheap per-triangle rejection of the shadow rasteriser, identical in effect to raster_sub's box test: no texel centre of the window
// inside the snapped bounding box.  (The pass is two-sided: the rare degenerate triangles are left to raster_sub.)
__device__ __forceinline__ bool tri_prefilter(int X0, int Y0, int X1, int Y1, int X2, int Y2, const TileCtx& T)
{
    constexpr int WIN = SPAN(ZR_MODE_SHADOW);
    const int x0 = max((imin3(X0, X1, X2) - 128 + 255) >> 8, T.px0), x1 = min((imax3(X0, X1, X2) - 128) >> 8, min(T.px0 + WIN - 1, T.W - 1));
    const int y0 = max((imin3(Y0, Y1, Y2) - 128 + 255) >> 8, T.py0), y1 = min((imax3(Y0, Y1, Y2) - 128) >> 8, min(T.py0 + WIN - 1, T.H - 1));
    return x0 <= x1 && y0 <= y1;
}

template <int MODE>
__device__ __forceinline__ void shade_key(int x, int y, float fy, const SV& v0, float gx, float gy, float zlo, float zhi,
                                          float bias, uint32_t prim, const TileCtx& T, unsigned long long* __restrict__ keys64, uint32_t* __restrict__ keys32)
{
    const float fx = (float)(x * 256 + 128 - v0.X);
    float z = __builtin_fmaf(gy, fy, __builtin_fmaf(gx, fx, v0.z));
    z = __builtin_fminf(__builtin_fmaxf(z, zlo), zhi);      // fragments stay within their vertices' depths (Hi-Z relies on it)
    z = z + 0.0f;
    const int li = (y - T.py0) * SPAN(MODE) + (x - T.px0);
    if (MODE == ZR_MODE_GBUFFER) {
        if (z >= 0.0f && z < 1.0f)   // depth clip (depthClampEnable FALSE) + LESS against the 1.0 clear
            atomicMin(&keys64[li], (unsigned long long)zr_f2u(z) << 32 | prim);
    } else {
        if (z >= 0.0f && z <= 1.0f) {
            const float zb = __builtin_fminf(__builtin_fmaxf(z + bias, 0.0f), 1.0f);
            atomicMin(&keys32[li], zr_f2u(zb));
        }
    }
}

// Rasterise one snapped triangle into the tile's LDS keys.
//   GBUFFER: key = depth_bits << 32 | prim, ds_min_u64  == depth test LESS in draw order (ties: lower prim wins)
//   SHADOW : key = biased depth bits,        ds_min_u32  == depth test LESS_OR_EQUAL, depth write only
// Coverage is exact integer arithmetic (edge functions of the snapped vertices, top-left rule as a -1 bias); the
// 32-bit loop is taken when every edge value met while walking the clipped bounding box fits, and is bit-identical.
// SMALL: every lane's triangle is small (every edge component below 2^14 sub-pixel units = 64 px) and given in TILE-RELATIVE
// coordinates.  The whole setup then stays in 32 bits: the clipped box lies in the tile, so |P - v| < 2^14 + 2^13 for every corner P of
// the walk and vertex v, an edge value is a difference of two products below 1.5 * 2^28 (|E| < 2^29.6 at the box origin), and the walk
// adds at most 31 steps of 256 |e| < 2^22 per axis (< 2^28): everything stays below 2^31; the area is a difference of two products
// below 2^28.  The tile kernels instantiate ONLY this form in their hot loop - bigger triangles take the clipper's route
// (raster_clipped, a call), which holds the general form - so the loop's register budget carries no 64-bit edge state.  Both forms
// produce the same integers.
#define ZR_SMALL_EDGE (1 << 14)
// every component of every EDGE below ZR_SMALL_EDGE  <=>  the snapped box is narrower than that on both axes (the widest edge
// component along an axis IS the box's extent along it).  All three edges: a triangle whose two edges at vertex 0 are short can still
// have a long third one (found by tests/test_gpu_fuzz.py: such a triangle overflowed the tile-relative 16-bit coordinates).
__device__ __forceinline__ bool tri_is_small(int x0, int y0, int x1, int y1, int x2, int y2)
{
    return imax3(x0, x1, x2) - imin3(x0, x1, x2) < ZR_SMALL_EDGE && imax3(y0, y1, y2) - imin3(y0, y1, y2) < ZR_SMALL_EDGE;
}
// BOXED: the caller hands over the clipped box it already formed with these very expressions (k_tile sorts its records by it).
template <int MODE, bool SMALL, bool BOXED = false>
__device__ __forceinline__ void raster_sub(const SV& v0, const SV& v1, const SV& v2, uint32_t prim, const TileCtx& T,
                                           unsigned long long* __restrict__ keys64, uint32_t* __restrict__ keys32, uint32_t box = 0u)
{
    const int dX1 = v1.X - v0.X, dY1 = v1.Y - v0.Y, dX2 = v2.X - v0.X, dY2 = v2.Y - v0.Y;
    constexpr bool all_small = SMALL;
    long long A;
    if (all_small) A = (long long)(dX1 * dY2 - dX2 * dY1);
    else A = (long long)dX1 * dY2 - (long long)dX2 * dY1;
    if (A == 0) return;
    // Vulkan facing: a = -A/2 in framebuffer coordinates; COUNTER_CLOCKWISE front  <=>  A < 0 (ZE:5113-5123)
    if (MODE == ZR_MODE_GBUFFER && A > 0) return;
    int x0, y0, x1, y1;
    if (BOXED) { x0 = (int)(box & 255u); y0 = (int)((box >> 8) & 255u); x1 = (int)((box >> 16) & 255u); y1 = (int)(box >> 24); }
    else {
        x0 = (imin3(v0.X, v1.X, v2.X) - 128 + 255) >> 8; x1 = (imax3(v0.X, v1.X, v2.X) - 128) >> 8;
        y0 = (imin3(v0.Y, v1.Y, v2.Y) - 128 + 255) >> 8; y1 = (imax3(v0.Y, v1.Y, v2.Y) - 128) >> 8;
        x0 = max(x0, T.px0); y0 = max(y0, T.py0);
        x1 = min(x1, min(T.px0 + SPAN(MODE) - 1, T.W - 1)); y1 = min(y1, min(T.py0 + SPAN(MODE) - 1, T.H - 1));
    }
    if (x0 > x1 || y0 > y1) return;

    const int sgn = A > 0 ? 1 : -1;
    // oriented edges (inside positive): e0 = v1->v2, e1 = v2->v0, e2 = v0->v1; top-left rule folded in as a bias
    const int ex0 = sgn * (v2.X - v1.X), ey0 = sgn * (v2.Y - v1.Y);
    const int ex1 = sgn * (v0.X - v2.X), ey1 = sgn * (v0.Y - v2.Y);
    const int ex2 = sgn * (v1.X - v0.X), ey2 = sgn * (v1.Y - v0.Y);
    const int Px0 = x0 * 256 + 128, Py0 = y0 * 256 + 128;
    const int tl0 = ((ey0 < 0) || (ey0 == 0 && ex0 > 0)) ? 0 : 1, tl1 = ((ey1 < 0) || (ey1 == 0 && ex1 > 0)) ? 0 : 1;
    const int tl2 = ((ey2 < 0) || (ey2 == 0 && ex2 > 0)) ? 0 : 1;

    // depth plane anchored at vertex 0, gradients per sub-pixel unit
    const float invA = 1.0f / (float)A;
    const float a1 = (float)(v2.Y - v0.Y) * invA, b1 = (float)(v0.X - v2.X) * invA;
    const float a2 = (float)(v0.Y - v1.Y) * invA, b2 = (float)(v1.X - v0.X) * invA;
    const float dz1 = v1.z - v0.z, dz2 = v2.z - v0.z;
    const float gx = __builtin_fmaf(a2, dz2, a1 * dz1), gy = __builtin_fmaf(b2, dz2, b1 * dz1);
    const float zlo = __builtin_fminf(__builtin_fminf(v0.z, v1.z), v2.z), zhi = __builtin_fmaxf(__builtin_fmaxf(v0.z, v1.z), v2.z);
    float bias = 0.0f;
    if (MODE == ZR_MODE_SHADOW) {
        // vkCmdSetDepthBias(1.25, 0, 7.5) on D32 (ZE:3280-3287): o = m * slope + r * constant, r = 2^(e - 23) of the primitive
        // clipped to z <= w: the far plane is clipped per fragment, so a vertex depth beyond it counts as 1 (as the oracle)
        const float m = __builtin_fmaxf(__builtin_fabsf(gx), __builtin_fabsf(gy)) * 256.0f;
        const float zm0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v0.z), __builtin_fabsf(v1.z)), __builtin_fabsf(v2.z));
        const float zm = zm0 > 1.0f ? 1.0f : zm0;
        const uint32_t e = zr_f2u(zm) & 0x7F800000u;
        const float r = (e > (23u << 23) && e < 0x7F800000u) ? zr_u2f(e - (23u << 23)) : 0.0f;
        bias = __builtin_fmaf(m, 7.5f, r * 1.25f);
    }
    int e0 = 0, e1 = 0, e2 = 0;
    long long E0 = 0, E1 = 0, E2 = 0;
    bool fits;
    if (all_small) {
        e0 = ex0 * (Py0 - v1.Y) - ey0 * (Px0 - v1.X) - tl0;
        e1 = ex1 * (Py0 - v2.Y) - ey1 * (Px0 - v2.X) - tl1;
        e2 = ex2 * (Py0 - v0.Y) - ey2 * (Px0 - v0.X) - tl2;
        fits = true;
    } else {
        E0 = (long long)ex0 * (Py0 - v1.Y) - (long long)ey0 * (Px0 - v1.X) - tl0;
        E1 = (long long)ex1 * (Py0 - v2.Y) - (long long)ey1 * (Px0 - v2.X) - tl1;
        E2 = (long long)ex2 * (Py0 - v0.Y) - (long long)ey2 * (Px0 - v0.X) - tl2;
        // |E| anywhere in the walk <= |E at the origin| + nx*|sx| + ny*|sy|
        const long long nx = x1 - x0 + 1, ny = y1 - y0 + 1;
        const long long lim = 0x3FFFFFFFll;
        const long long m0 = (E0 < 0 ? -E0 : E0) + 256 * (nx * (ey0 < 0 ? -(long long)ey0 : ey0) + ny * (ex0 < 0 ? -(long long)ex0 : ex0));
        const long long m1 = (E1 < 0 ? -E1 : E1) + 256 * (nx * (ey1 < 0 ? -(long long)ey1 : ey1) + ny * (ex1 < 0 ? -(long long)ex1 : ex1));
        const long long m2 = (E2 < 0 ? -E2 : E2) + 256 * (nx * (ey2 < 0 ? -(long long)ey2 : ey2) + ny * (ex2 < 0 ? -(long long)ex2 : ex2));
        fits = m0 < lim && m1 < lim && m2 < lim;
        if (fits) { e0 = (int)E0; e1 = (int)E1; e2 = (int)E2; }
    }
    if (fits) {
        const int sx0 = -ey0 * 256, sx1 = -ey1 * 256, sx2 = -ey2 * 256, sy0 = ex0 * 256, sy1 = ex1 * 256, sy2 = ex2 * 256;
        for (int y = y0; y <= y1; ++y) {
            int r0 = e0, r1 = e1, r2 = e2;
            const float fy = (float)(y * 256 + 128 - v0.Y);
            for (int x = x0; x <= x1; ++x) {
                if ((r0 | r1 | r2) >= 0) shade_key<MODE>(x, y, fy, v0, gx, gy, zlo, zhi, bias, prim, T, keys64, keys32);
                r0 += sx0; r1 += sx1; r2 += sx2;
            }
            e0 += sy0; e1 += sy1; e2 += sy2;
        }
    } else {
        const long long sx0 = -(long long)ey0 * 256, sx1 = -(long long)ey1 * 256, sx2 = -(long long)ey2 * 256;
        const long long sy0 = (long long)ex0 * 256, sy1 = (long long)ex1 * 256, sy2 = (long long)ex2 * 256;
        for (int y = y0; y <= y1; ++y) {
            long long r0 = E0, r1 = E1, r2 = E2;
            const float fy = (float)(y * 256 + 128 - v0.Y);
            for (int x = x0; x <= x1; ++x) {
                if ((r0 | r1 | r2) >= 0) shade_key<MODE>(x, y, fy, v0, gx, gy, zlo, zhi, bias, prim, T, keys64, keys32);
                r0 += sx0; r1 += sx1; r2 += sx2;
            }
            E0 += sy0; E1 += sy1; E2 += sy2;
        }
    }
}

// Sutherland-Hodgman against near (z >= 0) and the 4x guard band; intersections always run inside -> outside.
__device__ __forceinline__ float plane_dist(zf4 c, int plane)
{
    switch (plane) {
    case 0: return c.z;
    case 1: return __builtin_fmaf(ZR_GUARD, c.w, c.x);
    case 2: return __builtin_fmaf(ZR_GUARD, c.w, -c.x);
    case 3: return __builtin_fmaf(ZR_GUARD, c.w, c.y);
    default: return __builtin_fmaf(ZR_GUARD, c.w, -c.y);
    }
}
__device__ __forceinline__ zf4 lerp4(zf4 in, zf4 out, float t)
{
    zf4 r;
    r.x = __builtin_fmaf(t, out.x - in.x, in.x); r.y = __builtin_fmaf(t, out.y - in.y, in.y);
    r.z = __builtin_fmaf(t, out.z - in.z, in.z); r.w = __builtin_fmaf(t, out.w - in.w, in.w);
    return r;
}
// T and the keys are tile-relative (see k_raster_chunks): (ox, oy) = the tile's origin in sub-pixel units is taken off after projecting.
template <int MODE>
__device__ __forceinline__ void raster_clipped_body(zf4 c0, zf4 c1, zf4 c2, uint32_t prim, TileCtx T, float hw, float hh, int ox, int oy,
                                                    unsigned long long* keys64, uint32_t* keys32)
{
    zf4 a[10], b[10];
    int na = 3;
    a[0] = c0; a[1] = c1; a[2] = c2;
    for (int plane = 0; plane < 5; ++plane) {
        int nb = 0;
        for (int i = 0; i < na; ++i) {
            const zf4 p = a[i], q = a[(i + 1 == na) ? 0 : i + 1];
            const float dp = plane_dist(p, plane), dq = plane_dist(q, plane);
            const bool ip = dp >= 0.0f, iq = dq >= 0.0f;
            if (ip) b[nb++] = p;
            if (ip != iq) b[nb++] = ip ? lerp4(p, q, dp / (dp - dq)) : lerp4(q, p, dq / (dq - dp));
        }
        na = nb;
        if (na < 3) return;
        for (int i = 0; i < na; ++i) a[i] = b[i];
    }
    for (int i = 0; i < na; ++i) if (!(a[i].w > 0.0f)) return;
    SV s0 = project(a[0], hw, hh); s0.X -= ox; s0.Y -= oy;
    SV sp = project(a[1], hw, hh); sp.X -= ox; sp.Y -= oy;
    for (int i = 2; i < na; ++i) {
        SV sn = project(a[i], hw, hh); sn.X -= ox; sn.Y -= oy;
        raster_sub<MODE, false>(s0, sp, sn, prim, T, keys64, keys32);
        sp = sn;
    }
}
// (a call in k_shadow_slow and k_sky_tiles; k_tile<LAST> inlines the body under its own register budget)
template <int MODE>
__device__ __noinline__ void raster_clipped(zf4 c0, zf4 c1, zf4 c2, uint32_t prim, TileCtx T, float hw, float hh, int ox, int oy,
                                            unsigned long long* keys64, uint32_t* keys32)
{
    raster_clipped_body<MODE>(c0, c1, c2, prim, T, hw, hh, ox, oy, keys64, keys32);
}


// ------------------------------------------------------------------------------------------------ what the kernels that own a tile's keys share

// A tile in TILE-RELATIVE coordinates (origin = the tile's first pixel, (tpx0, tpy0) in the target): edge functions, depth planes and
// bounding boxes are built from coordinate differences, so the integers and floats are the ones absolute coordinates give.
__device__ __forceinline__ TileCtx tile_ctx(const ZrPass& P, uint32_t tile, int& tpx0, int& tpy0)
{
    tpx0 = (int)(tile % P.tiles_x) * TILE; tpy0 = (int)(tile / P.tiles_x) * TILE;
    TileCtx T;
    T.px0 = 0; T.py0 = 0; T.W = (int)P.W - tpx0; T.H = (int)P.H - tpy0;
    return T;
}

// A small triangle as the shadow rasteriser's queue and the camera pass's records hold it: per vertex X | Y << 16 (tile-relative, int16
// each) and the depth's bits; the primitive id.
struct RecTri { SV a, b, c; uint32_t prim; };
__device__ __forceinline__ SV sv_unpack(uint32_t xy, uint32_t z)
{
    SV s;
    s.X = (int)(short)(xy & 0xFFFFu); s.Y = (int)xy >> 16; s.z = zr_u2f(z); s.rw = 0.0f;
    return s;
}
__device__ __forceinline__ RecTri tri_unpack(uint32_t xy0, uint32_t z0, uint32_t xy1, uint32_t z1, uint32_t xy2, uint32_t z2, uint32_t prim)
{
    RecTri t;
    t.a = sv_unpack(xy0, z0); t.b = sv_unpack(xy1, z1); t.c = sv_unpack(xy2, z2); t.prim = prim;
    return t;
}

// The LDS keys of a tile (64-bit: depth << 32 | prim) or of a shadow window (32-bit: depth), `threads` threads: cleared to "nothing
// drawn", and the touched ones merged into the key buffer / the map with atomic min: the merge IS the depth write.
// COMPARE: the texel is read first and the atomic issued only for a key that lowers it (a list drawn into a buffer that already holds
// the frame); without, every touched key goes out (k_tile's units: the key buffer is empty but for this tile's other units).
__device__ __forceinline__ void keys_clear(unsigned long long* keys64, uint32_t tid, uint32_t threads)
{
    for (uint32_t i = tid; i < TILE_PIX; i += threads) keys64[i] = ZR_EMPTY_KEY;
}
__device__ __forceinline__ void keys_clear(uint32_t* keys32, uint32_t tid, uint32_t threads)
{
    for (uint32_t i = tid; i < (uint32_t)SPAN_PIX(ZR_MODE_SHADOW); i += threads) keys32[i] = 0x3F800000u;
}
template <bool COMPARE>
__device__ __forceinline__ void keys_merge(const ZrPass& P, int tpx0, int tpy0, const unsigned long long* keys64, unsigned long long* vis64,
                                           uint32_t tid, uint32_t threads)
{
    for (uint32_t i = tid; i < TILE_PIX; i += threads) {
        const int px = tpx0 + (int)(i & (TILE - 1)), py = tpy0 + (int)(i / TILE);
        if (px >= (int)P.W || py >= (int)P.H) continue;
        const size_t p = (size_t)py * P.W + (size_t)px;
        const unsigned long long k = keys64[i];
        if ((uint32_t)k != ZR_EMPTY_PRIM && (!COMPARE || k < vis64[p])) atomicMin(&vis64[p], k);
    }
}
// (a key still at its clear value 1.0 cannot lower the map, whose texels never exceed 1.0: its texel is not even read - the untouched
// four fifths of a window's 1 936 texels were 15 MB of the shadow pass's 25 MB of reads, profiles/r06_shadow_tcc.txt)
__device__ __forceinline__ void keys_merge(const ZrPass& P, int tpx0, int tpy0, const uint32_t* keys32, uint32_t* shadow_bits,
                                           uint32_t tid, uint32_t threads)
{
    constexpr uint32_t WIN = SPAN(ZR_MODE_SHADOW);
    for (uint32_t i = tid; i < WIN * WIN; i += threads) {
        const int px = tpx0 + (int)(i % WIN), py = tpy0 + (int)(i / WIN);
        if (px >= (int)P.W || py >= (int)P.H) continue;
        const size_t p = (size_t)py * P.W + (size_t)px;
        const uint32_t k = keys32[i];
        if (k != 0x3F800000u && k < shadow_bits[p]) atomicMin(&shadow_bits[p], k);
    }
}

// A SLOW triangle (it needs the clipper, or has an edge of 64 px or more) is not drawn where it is found but listed: 4 x uint4 - its three
// clip-space vertices and (prim, where, 0, 0); `where` is the tile whose list named it (shadow pass) or the rectangle of tiles it can
// touch (camera pass).  Record j's vertices, for a kernel that tries it on a tile through the clipper (the fourth word is the caller's:
// it decides whether to):
__device__ __forceinline__ void slow_read(const uint4* slow, uint32_t j, zf4& c0, zf4& c1, zf4& c2)
{
    const uint4 q0 = slow[4u * j], q1 = slow[4u * j + 1u], q2 = slow[4u * j + 2u];
    c0.x = zr_u2f(q0.x); c0.y = zr_u2f(q0.y); c0.z = zr_u2f(q0.z); c0.w = zr_u2f(q0.w);
    c1.x = zr_u2f(q1.x); c1.y = zr_u2f(q1.y); c1.z = zr_u2f(q1.z); c1.w = zr_u2f(q1.w);
    c2.x = zr_u2f(q2.x); c2.y = zr_u2f(q2.y); c2.z = zr_u2f(q2.z); c2.w = zr_u2f(q2.w);
}

// The next work unit of a persistent workgroup.  The first two are its own index and that + the grid (no atomic: an empty pass costs
// nothing, and when the grid's first units end together, a claim apiece on one counter would queue up for ~10 ns each); later ones come
// from the counter, through *s_next in LDS (rewritten by the next claim: hence the barrier after it is read).  The unit is claimed only
// when the last one is done: claiming early costs more in tail balance than the atomic's latency.
__device__ __forceinline__ uint32_t claim_unit(bool& first, uint32_t unit, uint32_t* counter, uint32_t* s_next, uint32_t tid)
{
    if (first) { first = false; __syncthreads(); return unit + gridDim.x; }
    if (tid == 0) *s_next = 2u * gridDim.x + atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t next = *s_next;
    __syncthreads();
    return next;
}
