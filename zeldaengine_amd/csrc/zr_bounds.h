// zr_bounds.h — bounding sphere + normal cone of one meshlet: ONE statement for the host (zr_meshlet_bounds: the clusteriser,
// zr_mesh_set_meshlets, zr_mesh_set_vertices) and the device (k_mesh_refit after a vertex update), as instance_record is for instances.
//
// float64 throughout, no contraction (every product and sum below is rounded once, on both compilers), sqrt and '/' are the IEEE
// operations on both sides: a record refitted on the device equals the one a new context computes on the host from the same vertices.
// No array of per-triangle normals: the normal of a triangle is formed again in each pass over the triangles (the same arithmetic gives
// the same value), so the function needs no storage that grows with the meshlet.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/zelda_abi.h"

struct ZrD3 { double x, y, z; };
#define ZR_BHD __host__ __device__ inline
ZR_BHD ZrD3 zr_d3_sub(ZrD3 a, ZrD3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
ZR_BHD ZrD3 zr_d3_add(ZrD3 a, ZrD3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
ZR_BHD ZrD3 zr_d3_mul(ZrD3 a, double s) { return { a.x * s, a.y * s, a.z * s }; }
ZR_BHD double zr_d3_dot(ZrD3 a, ZrD3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ZR_BHD ZrD3 zr_d3_cross(ZrD3 a, ZrD3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
ZR_BHD ZrD3 zr_d3_pos(const XkVertex& v) { return { (double)v.Position[0], (double)v.Position[1], (double)v.Position[2] }; }

// unit normal of triangle t (zero for a degenerate one); *a0 = its first corner
template <class Corner>
ZR_BHD ZrD3 zr_bounds_normal(const XkVertex* verts, const uint32_t* mv, const Corner& corner, uint32_t t, ZrD3* a0)
{
#pragma clang fp contract(off)
    const ZrD3 a = zr_d3_pos(verts[mv[corner(t, 0u)]]), b = zr_d3_pos(verts[mv[corner(t, 1u)]]), d = zr_d3_pos(verts[mv[corner(t, 2u)]]);
    const ZrD3 nn = zr_d3_cross(zr_d3_sub(b, a), zr_d3_sub(d, a));
    const double l = sqrt(zr_d3_dot(nn, nn));
    *a0 = a;
    return l > 0 ? zr_d3_mul(nn, 1.0 / l) : ZrD3{ 0, 0, 0 };
}

// verts: the mesh's vertices; mv[0 .. nv): the meshlet's vertex indices; corner(t, k): meshlet-local index of corner k of triangle t < nt.
// Writes BoundsCenter, BoundsRadius, ConeApex, ConeAxis, ConeCutoff of *out (meshoptimizer's published definition of the cone:
// cutoff = sqrt(1 - mindp^2), 1 = never culled).  A meshlet with a non-finite coordinate: radius +inf, cutoff 1 - no cull drops it.
template <class Corner>
ZR_BHD void zr_meshlet_bounds_of(const XkVertex* verts, const uint32_t* mv, uint32_t nv, const Corner& corner, uint32_t nt, XkMeshlet* out)
{
#pragma clang fp contract(off)
    bool finite = true;
    for (uint32_t i = 0; i < nv; ++i) {
        const float* p = verts[mv[i]].Position;
        if (!(fabsf(p[0]) <= 3.402823466e38f && fabsf(p[1]) <= 3.402823466e38f && fabsf(p[2]) <= 3.402823466e38f)) finite = false;
    }
    if (!finite) {
        out->BoundsCenter[0] = out->BoundsCenter[1] = out->BoundsCenter[2] = 0.0f; out->BoundsRadius = INFINITY;
        out->ConeApex[0] = out->ConeApex[1] = out->ConeApex[2] = 0.0f;
        out->ConeAxis[0] = 1.0f; out->ConeAxis[1] = out->ConeAxis[2] = 0.0f; out->ConeCutoff = 1.0f;
        return;
    }
    // bounding sphere: Ritter's two-pass sphere over the meshlet's vertices, then inflated to enclose exactly
    ZrD3 c = { 0, 0, 0 };
    double r = 0;
    if (nv) {
        const ZrD3 p0 = zr_d3_pos(verts[mv[0]]);
        uint32_t a = 0, b = 0; double best = -1;
        for (uint32_t i = 0; i < nv; ++i) { const ZrD3 d = zr_d3_sub(zr_d3_pos(verts[mv[i]]), p0); const double l = zr_d3_dot(d, d); if (l > best) { best = l; a = i; } }
        const ZrD3 pa = zr_d3_pos(verts[mv[a]]); best = -1;
        for (uint32_t i = 0; i < nv; ++i) { const ZrD3 d = zr_d3_sub(zr_d3_pos(verts[mv[i]]), pa); const double l = zr_d3_dot(d, d); if (l > best) { best = l; b = i; } }
        const ZrD3 pb = zr_d3_pos(verts[mv[b]]);
        c = zr_d3_mul(zr_d3_add(pa, pb), 0.5); r = sqrt(best) * 0.5;
        for (uint32_t i = 0; i < nv; ++i) {
            const ZrD3 d = zr_d3_sub(zr_d3_pos(verts[mv[i]]), c); const double l = sqrt(zr_d3_dot(d, d));
            if (l > r) { const double nr = (r + l) * 0.5; c = zr_d3_add(c, zr_d3_mul(d, (nr - r) / l)); r = nr; }
        }
        const float cf[3] = { (float)c.x, (float)c.y, (float)c.z };
        double rr = 0;
        for (uint32_t i = 0; i < nv; ++i) {
            const float* p = verts[mv[i]].Position;
            const double dx = (double)p[0] - cf[0], dy = (double)p[1] - cf[1], dz = (double)p[2] - cf[2];
            const double l = sqrt(dx * dx + dy * dy + dz * dz);
            rr = rr < l ? l : rr;
        }
        r = rr;
    }
    out->BoundsCenter[0] = (float)c.x; out->BoundsCenter[1] = (float)c.y; out->BoundsCenter[2] = (float)c.z;
    out->BoundsRadius = nextafterf((float)(r * (1.0 + 1e-6)), INFINITY);

    // normal cone
    ZrD3 axis = { 0, 0, 0 }, a0;
    for (uint32_t t = 0; t < nt; ++t) axis = zr_d3_add(axis, zr_bounds_normal(verts, mv, corner, t, &a0));
    const double al = sqrt(zr_d3_dot(axis, axis));
    double mindp = 1.0;
    if (al > 0) {
        axis = zr_d3_mul(axis, 1.0 / al);
        for (uint32_t t = 0; t < nt; ++t) { const double dp = zr_d3_dot(zr_bounds_normal(verts, mv, corner, t, &a0), axis); mindp = dp < mindp ? dp : mindp; }
    } else { axis = { 1, 0, 0 }; mindp = -1.0; }
    out->ConeAxis[0] = (float)axis.x; out->ConeAxis[1] = (float)axis.y; out->ConeAxis[2] = (float)axis.z;
    // degenerate cluster (cone wider than a hemisphere, or nearly so): cutoff 1 = never culled
    // (a flat cluster's mindp may round to a hair above 1: its cutoff is the least positive one, not the root of a negative number)
    const double s2 = 1.0 - mindp * mindp;
    out->ConeCutoff = (mindp <= 0.1) ? 1.0f : nextafterf((float)sqrt(s2 > 0 ? s2 : 0.0), 2.0f);
    // apex: meshoptimizer backs the centre off along the axis far enough to see every triangle's back side
    double maxt = 0;
    if (mindp > 0.1)
        for (uint32_t t = 0; t < nt; ++t) {
            const ZrD3 n = zr_bounds_normal(verts, mv, corner, t, &a0);
            const double dc = zr_d3_dot(zr_d3_sub(c, a0), n), dn = zr_d3_dot(axis, n);
            if (dn > 1e-12) { const double q = dc / dn; maxt = maxt < q ? q : maxt; }
        }
    const ZrD3 apex = zr_d3_sub(c, zr_d3_mul(axis, maxt));
    out->ConeApex[0] = (float)apex.x; out->ConeApex[1] = (float)apex.y; out->ConeApex[2] = (float)apex.z;
}
