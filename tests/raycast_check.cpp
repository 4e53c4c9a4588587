// raycast_check.cpp — csrc/zr_raycast.h alone, as a stand-alone program under the sanitizers (tests/test_raycast_cpu.py builds and runs
// it): the rule's details, one small case each, and the watertightness of a dyadic grid plane.
//   raycast_check            the cases; prints a line per failure, ends with "cases N failed F", exits 0 iff F == 0
//   raycast_check IN OUT     IN: u32 n_rays, n_tris, flags, 0, then n_rays zr_ray, then n_tris * 9 floats; OUT: n_rays zr_ray_hit -
//                            the same bytes as the library's zr_ray_triangles gives (two compilers, one statement)
#include "zr_raycast.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int g_cases = 0, g_failed = 0;
static void check(bool ok, const char* what)
{
    ++g_cases;
    if (!ok) { ++g_failed; printf("FAILED: %s\n", what); }
}

static zr_ray ray(float ox, float oy, float oz, float dx, float dy, float dz, float t0 = 0.0f, float t1 = INFINITY)
{
    zr_ray r; r.origin[0] = ox; r.origin[1] = oy; r.origin[2] = oz; r.t_min = t0; r.dir[0] = dx; r.dir[1] = dy; r.dir[2] = dz; r.t_max = t1;
    return r;
}
static zr_ray_hit cast1(const zr_ray& r, const std::vector<float>& tris, uint32_t flags = 0u)
{
    zr_ray_hit h;
    zr_rc_triangles(&r, 1u, tris.data(), (uint32_t)(tris.size() / 9u), flags, &h);
    return h;
}
static bool is_miss(const zr_ray_hit& h, uint32_t flags)
{
    const zr_ray_hit m = zr_rc_miss(flags);
    return memcmp(&h, &m, sizeof h) == 0;
}
static void tri(std::vector<float>& v, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz)
{
    const float p[9] = { ax, ay, az, bx, by, bz, cx, cy, cz };
    v.insert(v.end(), p, p + 9);
}

static void rule_details()
{
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // counter-clockwise seen from +z: the normal is +z, a ray going down -z meets the FRONT
    std::vector<float> one; tri(one, 0, 0, 0, 1, 0, 0, 0, 1, 0);
    zr_ray_hit h = cast1(ray(0.25f, 0.25f, 2, 0, 0, -1), one);
    check(h.flags == ZR_RAY_HIT && h.triangle == 0u && h.object == 0u && h.instance == 0u && h.t == 2.0f && h.u == 0.25f && h.v == 0.25f &&
          h.normal[0] == 0.0f && h.normal[1] == 0.0f && h.normal[2] == 1.0f && h.reserved == 0u && h.reserved2 == 0u, "a front hit: t, u, v, normal");
    h = cast1(ray(0.25f, 0.25f, -2, 0, 0, 1), one);
    check(h.flags == (ZR_RAY_HIT | ZR_RAY_HIT_BACK) && h.t == 2.0f, "the same triangle from behind is BACK");
    check(is_miss(cast1(ray(0.25f, 0.25f, -2, 0, 0, 1), one, ZR_RAY_CULL_BACK), 0u), "ZR_RAY_CULL_BACK: a BACK hit does not count");
    check(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1), one, ZR_RAY_CULL_BACK).flags == ZR_RAY_HIT, "ZR_RAY_CULL_BACK keeps a FRONT hit");
    std::vector<float> mirrored; tri(mirrored, 0, 0, 0, -1, 0, 0, 0, 1, 0);      // x -> -x: the winding turns round
    check(cast1(ray(-0.25f, 0.25f, 2, 0, 0, -1), mirrored).flags == (ZR_RAY_HIT | ZR_RAY_HIT_BACK), "a mirrored triangle flips the BACK flag");
    check(cast1(ray(-0.25f, 0.25f, -2, 0, 0, 1), mirrored).flags == ZR_RAY_HIT, "... both ways");
    // every axis and sign of the ray's largest component
    for (int axis = 0; axis < 3; ++axis)
        for (int sign = -1; sign <= 1; sign += 2) {
            float A[3] = { 0, 0, 0 }, B[3] = { 0, 0, 0 }, C[3] = { 0, 0, 0 }, o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 };
            const int x = (axis + 1) % 3, y = (axis + 2) % 3;
            B[x] = 1; C[y] = 1;                              // normal = +axis
            o[x] = 0.25f; o[y] = 0.5f; o[axis] = 3.0f * (float)sign; d[axis] = -(float)sign; d[x] = 0.0625f; d[y] = -0.03125f;
            std::vector<float> t1; tri(t1, A[0], A[1], A[2], B[0], B[1], B[2], C[0], C[1], C[2]);
            h = cast1(ray(o[0], o[1], o[2], d[0], d[1], d[2]), t1);
            check(h.flags == (sign > 0 ? ZR_RAY_HIT : (ZR_RAY_HIT | ZR_RAY_HIT_BACK)) && h.t == 3.0f && h.u == 0.4375f && h.v == 0.40625f, "axes and signs");
        }
    // the tie goes to the least primitive id, whatever the order of visiting
    std::vector<float> two; tri(two, 0, 0, 0, 1, 0, 0, 0, 1, 0); tri(two, 0, 0, 0, 1, 0, 0, 0, 1, 0);
    check(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1), two).triangle == 0u, "two coincident triangles: the lower id");
    // t_min / t_max exclude the nearest and select the next
    std::vector<float> stack; tri(stack, 0, 0, 1, 1, 0, 1, 0, 1, 1); tri(stack, 0, 0, 0, 1, 0, 0, 0, 1, 0);
    check(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1), stack).triangle == 0u, "the nearest of two");
    h = cast1(ray(0.25f, 0.25f, 2, 0, 0, -1, 1.5f, 4.0f), stack);
    check(h.triangle == 1u && h.t == 2.0f, "t_min excludes the nearest and selects the next");
    check(is_miss(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1, 0.0f, 0.5f), stack), 0u), "t_max before the nearest: a miss");
    check(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1, 1.0f, 1.0f), stack).triangle == 0u, "the bounds are inclusive");
    check(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1, 0.0f, 4.0f), stack, ZR_RAY_ANY_HIT).flags == ZR_RAY_HIT &&
          cast1(ray(0.25f, 0.25f, 2, 0, 0, -1, 0.0f, 4.0f), stack, ZR_RAY_ANY_HIT).object == 0xFFFFFFFFu, "ZR_RAY_ANY_HIT: the flag alone, the rest a miss");
    check(is_miss(cast1(ray(0.25f, 0.25f, 2, 0, 0, -1, 0.0f, 0.5f), stack, ZR_RAY_ANY_HIT), 0u), "ZR_RAY_ANY_HIT: a miss");
    // det == 0: a triangle seen edge-on
    std::vector<float> edge_on; tri(edge_on, 0, 0, 0, 1, 0, 0, 0, 0, 1);
    check(is_miss(cast1(ray(0.25f, 0, 2, 0, 0, -1), edge_on), 0u), "det == 0 (an edge-on triangle) misses");
    // invalid rays
    check(is_miss(cast1(ray(0, 0, 1, 0, 0, 0), one), ZR_RAY_INVALID), "a zero direction is invalid");
    check(is_miss(cast1(ray(nan, 0, 1, 0, 0, -1), one), ZR_RAY_INVALID), "a NaN origin is invalid");
    check(is_miss(cast1(ray(0, 0, 1, 0, INFINITY, -1), one), ZR_RAY_INVALID), "an infinite direction is invalid");
    check(is_miss(cast1(ray(0.25f, 0.25f, 1, 0, 0, -1, nan, 1.0f), one), ZR_RAY_INVALID), "a NaN bound is invalid");
    check(is_miss(cast1(ray(0.25f, 0.25f, 1, 0, 0, -1, 2.0f, 1.0f), one), ZR_RAY_INVALID), "t_min > t_max is invalid");
    check(is_miss(cast1(ray(0.25f, 0.25f, 1, 0, 0, -1, 2.0f, 1.0f), one, ZR_RAY_ANY_HIT), ZR_RAY_INVALID), "... under ZR_RAY_ANY_HIT too");
    check(cast1(ray(0.25f, 0.25f, 1, 0, 0, -1, -INFINITY, INFINITY), one).flags == ZR_RAY_HIT, "infinite bounds are valid");
    // a NaN corner is a miss, and hides nothing
    std::vector<float> bad; tri(bad, 0, 0, 1, nan, 0, 1, 0, 1, 1); tri(bad, 0, 0, 0, 1, 0, 0, 0, 1, 0);
    h = cast1(ray(0.25f, 0.25f, 2, 0, 0, -1), bad);
    check(h.flags == ZR_RAY_HIT && h.triangle == 1u, "a NaN corner is a miss");
    // no rays, no triangles
    zr_rc_triangles(nullptr, 0u, one.data(), 1u, 0u, nullptr);
    const zr_ray r0 = ray(0.25f, 0.25f, 2, 0, 0, -1);
    zr_ray_hit h0; zr_rc_triangles(&r0, 1u, nullptr, 0u, 0u, &h0);
    check(is_miss(h0, 0u), "n_tris = 0: a miss");
    // t = -0 is reported as +0
    h = cast1(ray(0.25f, 0.25f, 0, 0, 0, -1, -1.0f, 1.0f), one);
    check(h.flags == ZR_RAY_HIT && h.t == 0.0f && !std::signbit(h.t), "t = -0 is +0");
}

// A 9 x 9-vertex grid plane at z = 0 with vertices at multiples of 1/8 (128 triangles) and 400 rays from dyadic origins aimed exactly
// at points of interior edges and at interior vertices: every one hits, and the hit is a triangle that shares the edge or vertex.
static void watertight_grid()
{
    std::vector<float> tris;
    for (int j = 0; j < 8; ++j)
        for (int i = 0; i < 8; ++i) {
            const float x0 = (float)i / 8.0f, x1 = (float)(i + 1) / 8.0f, y0 = (float)j / 8.0f, y1 = (float)(j + 1) / 8.0f;
            tri(tris, x0, y0, 0, x1, y0, 0, x1, y1, 0);
            tri(tris, x0, y0, 0, x1, y1, 0, x0, y1, 0);
        }
    uint32_t seed = 12345u;
    auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
    int leaks = 0, wrong = 0;
    for (int k = 0; k < 400; ++k) {
        // a target on an interior grid line (64ths along it) or, every fourth ray, at an interior vertex; k % 3 == 2: on a diagonal
        float tx, ty;
        if (k % 4 == 0) { tx = (float)(1 + rnd(7)) / 8.0f; ty = (float)(1 + rnd(7)) / 8.0f; }
        else if (k % 3 == 2) { const uint32_t i = rnd(8), j = rnd(8), s = 1 + rnd(7); tx = (float)i / 8.0f + (float)s / 64.0f; ty = (float)j / 8.0f + (float)s / 64.0f; }
        else if (k % 2) { tx = (float)(1 + rnd(7)) / 8.0f; ty = (float)(1 + rnd(62)) / 64.0f; }
        else { tx = (float)(1 + rnd(62)) / 64.0f; ty = (float)(1 + rnd(7)) / 8.0f; }
        const float ox = (float)((int)rnd(65) - 32) / 16.0f, oy = (float)((int)rnd(65) - 32) / 16.0f, oz = (float)(1 + rnd(16)) / 4.0f * (k % 5 == 0 ? -1.0f : 1.0f);
        const zr_ray r = ray(ox, oy, oz, tx - ox, ty - oy, -oz);      // dyadic: the differences are exact, the target is at t = 1
        zr_ray_hit h;
        zr_rc_triangles(&r, 1u, tris.data(), 128u, 0u, &h);
        if (!(h.flags & ZR_RAY_HIT)) { ++leaks; continue; }
        // The triangles that hold the target (closed: edges and corners included), by exact dyadic arithmetic.  The shear's quotients are
        // rounded, so the rule may see the ray a hair to one side of the edge: the hit is one of the sharers - and where several accept
        // at one t, the least id (the key's order, checked alone above).  t = 1 up to the rounding of Sz and the quotient.
        bool holds = false;
        {
            const float* P = tris.data() + (size_t)h.triangle * 9u;
            const double e0 = ((double)P[3] - P[0]) * ((double)ty - P[1]) - ((double)P[4] - P[1]) * ((double)tx - P[0]);
            const double e1 = ((double)P[6] - P[3]) * ((double)ty - P[4]) - ((double)P[7] - P[4]) * ((double)tx - P[3]);
            const double e2 = ((double)P[0] - P[6]) * ((double)ty - P[7]) - ((double)P[1] - P[7]) * ((double)tx - P[6]);
            holds = h.triangle < 128u && e0 >= 0 && e1 >= 0 && e2 >= 0;
        }
        if (!holds || !(std::fabs((double)h.t - 1.0) <= 8.0 / 16777216.0)) ++wrong;
    }
    // Where the shear is exact - the direction's z is +-1, 2 or 4 and its largest component, x and y sixteenths below 1, so the three
    // quotients and every sheared value are exact - the target lies on the edge for the rule itself: every sharer accepts at t = 1 and
    // the hit is the one with the least id.
    int not_least = 0;
    for (int k = 0; k < 400; ++k) {
        float tx, ty;
        if (k % 4 == 0) { tx = (float)(1 + rnd(7)) / 8.0f; ty = (float)(1 + rnd(7)) / 8.0f; }
        else if (k % 3 == 2) { const uint32_t i = rnd(8), j = rnd(8), s = 1 + rnd(7); tx = (float)i / 8.0f + (float)s / 64.0f; ty = (float)j / 8.0f + (float)s / 64.0f; }
        else if (k % 2) { tx = (float)(1 + rnd(7)) / 8.0f; ty = (float)(1 + rnd(62)) / 64.0f; }
        else { tx = (float)(1 + rnd(62)) / 64.0f; ty = (float)(1 + rnd(7)) / 8.0f; }
        const float oz = (float)(1u << rnd(3)) * (k % 5 == 0 ? -1.0f : 1.0f);
        const float ox = tx - (float)((int)rnd(31) - 15) / 16.0f, oy = ty - (float)((int)rnd(31) - 15) / 16.0f;
        const zr_ray r = ray(ox, oy, oz, tx - ox, ty - oy, -oz);
        zr_ray_hit h;
        zr_rc_triangles(&r, 1u, tris.data(), 128u, 0u, &h);
        uint32_t want = 0xFFFFFFFFu;
        for (uint32_t t = 0; t < 128u && want == 0xFFFFFFFFu; ++t) {
            const float* P = tris.data() + (size_t)t * 9u;
            const double e0 = ((double)P[3] - P[0]) * ((double)ty - P[1]) - ((double)P[4] - P[1]) * ((double)tx - P[0]);
            const double e1 = ((double)P[6] - P[3]) * ((double)ty - P[4]) - ((double)P[7] - P[4]) * ((double)tx - P[3]);
            const double e2 = ((double)P[0] - P[6]) * ((double)ty - P[7]) - ((double)P[1] - P[7]) * ((double)tx - P[6]);
            if (e0 >= 0 && e1 >= 0 && e2 >= 0) want = t;
        }
        if (!(h.flags & ZR_RAY_HIT) || h.triangle != want || h.t != 1.0f) ++not_least;
    }
    check(not_least == 0, "watertightness: with an exact shear the hit is the sharing triangle with the least id, at t = 1");
    check(leaks == 0, "watertightness: a ray aimed at an interior edge or vertex slipped through");
    check(wrong == 0, "watertightness: the hit is a triangle that shares the edge or vertex, at t = 1");
}

int main(int argc, char** argv)
{
    if (argc == 3) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        uint32_t head[4];
        if (fread(head, 4, 4, f) != 4) { fclose(f); return 2; }
        std::vector<zr_ray> rays(head[0]); std::vector<float> tris((size_t)head[1] * 9u); std::vector<zr_ray_hit> hits(head[0]);
        const bool ok = fread(rays.data(), sizeof(zr_ray), rays.size(), f) == rays.size() && fread(tris.data(), 4, tris.size(), f) == tris.size();
        fclose(f);
        if (!ok) return 2;
        zr_rc_triangles(rays.data(), head[0], tris.data(), head[1], head[2], hits.data());
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        const bool wrote = fwrite(hits.data(), sizeof(zr_ray_hit), hits.size(), f) == hits.size();
        return fclose(f) == 0 && wrote ? 0 : 2;
    }
    rule_details();
    watertight_grid();
    printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed == 0 ? 0 : 1;
}
