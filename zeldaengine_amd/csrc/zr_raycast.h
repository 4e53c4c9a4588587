// zr_raycast.h — casting rays into the scene (zelda_render.h, "casting rays"; DESIGN.md section 5, "Casting rays"): the ONE statement of
// the ray / triangle rule, which the kernel (zr_raycast.hip), the host function (zr_ray_triangles) and a stand-alone program
// (tests/raycast_check.cpp, under the sanitizers) all call.  Plain C++ and nothing of HIP.  Contraction is off wherever this is compiled
// (-ffp-contract=off), '/' is the IEEE operation.
//
// A ray is (o, d, t_min, t_max), a triangle three world-space float32 corners A, B, C.
//   invalid    a non-finite component of o or d, d == 0, a NaN bound, t_min > t_max: the ray hits nothing, its record carries ZR_RAY_INVALID
//   axes       kz = the component of d with the largest |d| (ties: the lowest index), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky
//              swapped when d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]  (float32)
//   corner     P' = P - o per component;  Px = P'[kx] - Sx * P'[kz],  Py = P'[ky] - Sy * P'[kz],  Pz = Sz * P'[kz]: every product and every
//              difference rounded once, in float32.  A corner's three values depend on that corner and the ray alone: two triangles that
//              share an edge see the same values there, and a ray through a closed surface cannot slip between them.
//   edges      in float64 from those values:  U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax.  The product of two float32
//              values is exact in float64 and the difference is rounded once: every sign is exact.
//   miss       some of U, V, W < 0 and some > 0 (zero counts as either sign);  det = U + V + W == 0;  a NaN anywhere
//   hit        T = (U Az + V Bz) + W Cz (float64);  t = (float)(T / det), u = (float)(V / det), v = (float)(W / det);  hit iff
//              t_min <= t <= t_max.  The hit point is (1 - u - v) A + u B + v C.  (t = -0 is reported, and ordered, as +0.)
//   facing     The map (x, y, z) -> (Px, Py, Pz) keeps orientation and sends d to +z, and det = -((B' - A') x (C' - A')).z there: so
//              det < 0  <=>  d and (B - A) x (C - A) point the same way  <=>  ZR_RAY_HIT_BACK.  det > 0 is FRONT: the side the camera pass
//              draws (cull BACK, front = counter-clockwise as the viewer sees it, the normal towards the viewer).
//   normal     (B - A) x (C - A) in float32, not normalised: e1 = B - A, e2 = C - A per component, then per component of the cross
//              product the two products rounded, then their difference.
// A scene's answer is the hit with the least t, ties to the least primitive id: the least 64-bit key (t as an ordered integer in the
// high word, the id in the low one) - the same whatever order the triangles are visited in.
//
// Out of scope: an acceleration structure over instances (the kernel's instance level is linear per ray: fine for an editor's handful of
// rays and for tens of thousands of instances, slow for millions of rays against a million instances); hits on the skydome;
// interpolated shading normals, UVs and materials; rays against a scene no frame has drawn.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/zelda_render.h"      // zr_ray, zr_ray_hit, ZR_RAY_*

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_RC_FN __host__ __device__ static inline
#else
#define ZR_RC_FN static inline
#endif

#define ZR_RAY_QUERY_FLAGS (ZR_RAY_CULL_BACK | ZR_RAY_ANY_HIT | ZR_RAY_NO_BOUNDS)
#define ZR_RAY_MAX_RAYS (1u << 24)
#define ZR_RAY_NO_KEY 0xFFFFFFFFFFFFFFFFull

static_assert(sizeof(zr_ray) == 32 && sizeof(zr_ray_hit) == 48, "two and three 16-byte words");

// A ray set up: the axes and the shear; valid = none of the cases above
struct ZrRcRay { float o[3], d[3], t_min, t_max, Sx, Sy, Sz; int kx, ky, kz; bool valid; };
// A corner in the ray's sheared coordinates
struct ZrRcCorner { float x, y, z; };
// One triangle against one ray
struct ZrRcTri { float t, u, v; bool hit, back; };

ZR_RC_FN bool zr_rc_finite(float f) { return __builtin_fabsf(f) <= 3.402823466e38f; }      // (NaN: false)

ZR_RC_FN float zr_rc_pick(const float* p, int k) { return k == 0 ? p[0] : (k == 1 ? p[1] : p[2]); }      // (no indexed register file on the device)

ZR_RC_FN ZrRcRay zr_rc_ray(const zr_ray& r)
{
    ZrRcRay R;
    for (int k = 0; k < 3; ++k) { R.o[k] = r.origin[k]; R.d[k] = r.dir[k]; }
    R.t_min = r.t_min; R.t_max = r.t_max;
    R.valid = zr_rc_finite(R.o[0]) && zr_rc_finite(R.o[1]) && zr_rc_finite(R.o[2]) && zr_rc_finite(R.d[0]) && zr_rc_finite(R.d[1]) && zr_rc_finite(R.d[2]) &&
              !(R.d[0] == 0.0f && R.d[1] == 0.0f && R.d[2] == 0.0f) && R.t_min == R.t_min && R.t_max == R.t_max && !(R.t_min > R.t_max);
    const float a0 = __builtin_fabsf(R.d[0]), a1 = __builtin_fabsf(R.d[1]), a2 = __builtin_fabsf(R.d[2]);
    int kz = 0;
    if (a1 > a0) kz = 1;
    if (a2 > (kz ? a1 : a0)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = zr_rc_pick(R.d, kz);
    if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    R.kx = kx; R.ky = ky; R.kz = kz;
    R.Sx = R.Sy = R.Sz = 0.0f;
    if (R.valid) { R.Sx = zr_rc_pick(R.d, kx) / dz; R.Sy = zr_rc_pick(R.d, ky) / dz; R.Sz = 1.0f / dz; }
    return R;
}

ZR_RC_FN ZrRcCorner zr_rc_corner(const ZrRcRay& R, const float* P)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float q[3] = { P[0] - R.o[0], P[1] - R.o[1], P[2] - R.o[2] };
    const float qx = zr_rc_pick(q, R.kx), qy = zr_rc_pick(q, R.ky), qz = zr_rc_pick(q, R.kz);
    const float sx = R.Sx * qz, sy = R.Sy * qz;
    ZrRcCorner c;
    c.x = qx - sx; c.y = qy - sy; c.z = R.Sz * qz;
    return c;
}

ZR_RC_FN ZrRcTri zr_rc_triangle(const ZrRcRay& R, const ZrRcCorner& A, const ZrRcCorner& B, const ZrRcCorner& C)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    ZrRcTri h; h.t = h.u = h.v = 0.0f; h.hit = false; h.back = false;
    const double ax = A.x, ay = A.y, bx = B.x, by = B.y, cx = C.x, cy = C.y;
    const double cxby = cx * by, cybx = cy * bx, axcy = ax * cy, aycx = ay * cx, bxay = bx * ay, byax = by * ax;      // exact
    const double U = cxby - cybx, V = axcy - aycx, W = bxay - byax;
    if (!(U == U && V == V && W == W)) return h;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return h;
    const double uv = U + V, det = uv + W;
    if (!(det == det) || det == 0.0) return h;
    const double ua = U * (double)A.z, vb = V * (double)B.z, wc = W * (double)C.z;
    const double uavb = ua + vb, T = uavb + wc;
    float t = (float)(T / det);
    const float u = (float)(V / det), v = (float)(W / det);
    if (t == 0.0f) t = 0.0f;                 // (-0 -> +0)
    if (!(t >= R.t_min && t <= R.t_max) || !(u == u) || !(v == v)) return h;
    h.t = t; h.u = u; h.v = v; h.hit = true; h.back = det < 0.0;
    return h;
}

ZR_RC_FN void zr_rc_normal(const float* A, const float* B, const float* C, float* n)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float e1[3] = { B[0] - A[0], B[1] - A[1], B[2] - A[2] }, e2[3] = { C[0] - A[0], C[1] - A[1], C[2] - A[2] };
    const float p0 = e1[1] * e2[2], q0 = e1[2] * e2[1], p1 = e1[2] * e2[0], q1 = e1[0] * e2[2], p2 = e1[0] * e2[1], q2 = e1[1] * e2[0];
    n[0] = p0 - q0; n[1] = p1 - q1; n[2] = p2 - q2;
}

// t as an integer that orders as the float does (t is never NaN here, and never -0)
ZR_RC_FN uint32_t zr_rc_ordered(float t)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, t);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ZR_RC_FN uint64_t zr_rc_key(float t, uint32_t prim) { return (uint64_t)zr_rc_ordered(t) << 32 | prim; }

// The records.  A miss: object = instance = triangle = all ones, every other word 0 but `flags` (0 or ZR_RAY_INVALID).
ZR_RC_FN zr_ray_hit zr_rc_miss(uint32_t flags)
{
    zr_ray_hit h;
    h.object = h.instance = h.triangle = 0xFFFFFFFFu; h.flags = flags;
    h.t = h.u = h.v = 0.0f; h.reserved = 0u;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0f; h.reserved2 = 0u;
    return h;
}
// ... and the hit of the triangle with the world corners A, B, C (the winner's, tested again: the same arithmetic gives the same t)
ZR_RC_FN zr_ray_hit zr_rc_record(const ZrRcRay& R, const float* A, const float* B, const float* C, uint32_t object, uint32_t instance, uint32_t triangle)
{
    const ZrRcTri T = zr_rc_triangle(R, zr_rc_corner(R, A), zr_rc_corner(R, B), zr_rc_corner(R, C));
    zr_ray_hit h = zr_rc_miss(0u);
    if (!T.hit) return h;
    h.object = object; h.instance = instance; h.triangle = triangle;
    h.flags = ZR_RAY_HIT | (T.back ? ZR_RAY_HIT_BACK : 0u);
    h.t = T.t; h.u = T.u; h.v = T.v;
    zr_rc_normal(A, B, C, h.normal);
    return h;
}

// The context-free statement: every ray against n_tris triangles of 9 floats (A, B, C), primitive id = the triangle's index.  A hit's
// object and instance are 0, its triangle the index.
ZR_RC_FN void zr_rc_triangles(const zr_ray* rays, uint32_t n_rays, const float* tris, uint32_t n_tris, uint32_t flags, zr_ray_hit* hits)
{
    for (uint32_t i = 0; i < n_rays; ++i) {
        const ZrRcRay R = zr_rc_ray(rays[i]);
        if (!R.valid) { hits[i] = zr_rc_miss(ZR_RAY_INVALID); continue; }
        uint64_t best = ZR_RAY_NO_KEY;
        for (uint32_t k = 0; k < n_tris; ++k) {
            const float* P = tris + (size_t)k * 9u;
            const ZrRcTri T = zr_rc_triangle(R, zr_rc_corner(R, P), zr_rc_corner(R, P + 3), zr_rc_corner(R, P + 6));
            if (!T.hit || ((flags & ZR_RAY_CULL_BACK) && T.back)) continue;
            const uint64_t key = zr_rc_key(T.t, k);
            if (key < best) best = key;
            if (flags & ZR_RAY_ANY_HIT) break;
        }
        if (best == ZR_RAY_NO_KEY) { hits[i] = zr_rc_miss(0u); continue; }
        if (flags & ZR_RAY_ANY_HIT) { hits[i] = zr_rc_miss(ZR_RAY_HIT); continue; }
        const uint32_t k = (uint32_t)best;
        const float* P = tris + (size_t)k * 9u;
        hits[i] = zr_rc_record(R, P, P + 3, P + 6, 0u, 0u, k);
    }
}
