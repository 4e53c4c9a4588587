// zr_raycast_host.cpp — casting rays behind the C-ABI (zelda_render.h, "casting rays"): the host form and the device form of the query,
// the camera's ray through a frame position, and the context-free host statement of the rule (zr_raycast.h).
//
// What the rays see is the frame enqueued last: zr_ctx::d_objs is that frame's draw table (its parity's instance planes and mesh sets
// hang off it), cam_prev_key its camera pass's block (M, m_scale), and the census's table (ids_prepare: draw order -> add order) names
// the objects; no id capture is needed, the table is made here when no captured frame made it.
// The device form against frames in flight.  Its launch rides the render stream: behind the last frame's passes, ahead of the next
// frame's.  The frame after next rewrites the planes and sets of this parity at its head (zr_update_frame) - on the camera lane, where
// stream order says nothing: the launch is noted as the census notes its own (ids_reader_enqueued), and that frame's head waits.
// A scene that no update has split into parities yet is read from parity 0 by every frame, and the first update makes the very next
// frame the writer: there the launch is noted in both copies.
#include "zr_ctx.h"
#include "zr_raycast.h"

#include <cmath>
#include <cstring>

static int rays_args_ok(zr_ctx* c, const void* rays, uint32_t n, uint32_t flags, const void* hits)
{
    ARGCHK(c, n == 0u || (rays != nullptr && hits != nullptr));
    ARGCHK(c, (flags & ~ZR_RAY_QUERY_FLAGS) == 0u);
    ARGCHK(c, n <= ZR_RAY_MAX_RAYS);
    return ZR_OK;
}

static int rays_launch(zr_ctx* c, const zr_ray* rays_dev, uint32_t n, uint32_t flags, zr_ray_hit* hits_dev)
{
    if (int rc = ids_prepare(c)) return rc;
    ZrRayArgs A; memset(&A, 0, sizeof A);
    A.rays = rays_dev; A.hits = hits_dev;
    A.objs = c->d_objs; A.draws = c->ids.draws;
    A.n_rays = n; A.n_draws = c->ids.n_draws; A.n_inst = c->n_inst_total; A.flags = flags;
    memcpy(A.M, c->cam_prev_key.M, sizeof A.M); A.m_scale = c->cam_prev_key.m_scale;
    zr_launch_raycast(A, c->stream);
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}

extern "C" int zr_raycast(zr_ctx* c, const zr_ray* rays, uint32_t n, uint32_t flags, zr_ray_hit* hits, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = rays_args_ok(c, rays, n, flags, hits)) return rc;
        ARGCHK(c, bytes == (size_t)n * sizeof(zr_ray_hit));
        if (int rc = ids_ready(c, "zr_raycast", true, false)) return rc;
        if (n == 0u) return ZR_OK;
        zr_ctx::Rays& S = c->rays;
        if (S.cap < n) {
            S.mem.release(); S.rays = nullptr; S.hits = nullptr; S.cap = 0;
            size_t cap = 256; while (cap < n) cap *= 2;
            HIPCHK(c, S.mem.alloc(&S.rays, cap)); HIPCHK(c, S.mem.alloc(&S.hits, cap));
            S.cap = cap;
        }
        HIPCHK(c, hipMemcpyAsync(S.rays, rays, (size_t)n * sizeof(zr_ray), hipMemcpyHostToDevice, c->stream));
        if (int rc = rays_launch(c, S.rays, n, flags, S.hits)) return rc;
        HIPCHK(c, hipMemcpyAsync(hits, S.hits, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ZR_OK;
    });
}

extern "C" int zr_raycast_async(zr_ctx* c, const void* rays_dev, uint32_t n, uint32_t flags, void* hits_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = rays_args_ok(c, rays_dev, n, flags, hits_dev)) return rc;
        ARGCHK(c, ((uintptr_t)rays_dev & 15u) == 0u && ((uintptr_t)hits_dev & 15u) == 0u);
        if (int rc = ids_ready(c, "zr_raycast_async", false, false)) return rc;
        if (n == 0u) return ZR_OK;
        if (int rc = rays_launch(c, (const zr_ray*)rays_dev, n, flags, (zr_ray_hit*)hits_dev)) return rc;
        // (the launch reads the last frame's table, planes and sets.  Until the first update every frame reads parity 0's, whatever its own
        // parity: the NEXT frame may then be the one that rewrites them, so both copies note the reader)
        // A frame that keeps its camera pass takes no note and needs none: it rewrites nothing at its head - an update due in its parity
        // would have ended the keep (zr_update_end).
        return ids_reader_enqueued(c, !c->upd.dual);
    });
}

// A 4 x 4 matrix (column-major) inverted in float64 by Gauss-Jordan elimination with partial pivoting; false: singular or not finite
static bool invert4(const double* m, double* inv)
{
    double a[4][8];
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) { a[r][k] = m[k * 4 + r]; a[r][4 + k] = r == k ? 1.0 : 0.0; }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (!(std::fabs(a[piv][col]) > 0.0) || !std::isfinite(a[piv][col])) return false;
        if (piv != col) for (int k = 0; k < 8; ++k) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 8; ++k) a[col][k] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            for (int k = 0; k < 8; ++k) a[r][k] -= f * a[col][k];
        }
    }
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) inv[k * 4 + r] = a[r][4 + k];
    return true;
}

extern "C" int zr_camera_ray(zr_ctx* c, float px, float py, zr_ray* out)
{
    if (!c || !out) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, std::isfinite(px) && std::isfinite(py));
        if (!c->frame_valid) return zr_fail(c, ZR_ERR_STATE, "zr_camera_ray: no frame uniforms: call zr_update_uniforms or zr_set_frame first");
        double pv[16], inv[16];
        for (int col = 0; col < 4; ++col)
            for (int r = 0; r < 4; ++r) {
                double s = 0.0;
                for (int k = 0; k < 4; ++k) s += (double)c->cam.Proj[k * 4 + r] * (double)c->cam.View[col * 4 + k];
                pv[col * 4 + r] = s;
            }
        if (!invert4(pv, inv)) return zr_fail(c, ZR_ERR_STATE, "zr_camera_ray: Proj * View has no inverse");
        // the camera pass's viewport: x_s = ndc.x * W / 2 + W / 2, depth 0 (near) .. 1 (far)
        const double nx = (double)px / (0.5 * (double)c->W) - 1.0, ny = (double)py / (0.5 * (double)c->H) - 1.0;
        double ends[2][3];
        for (int e = 0; e < 2; ++e) {
            const double ndc[4] = { nx, ny, (double)e, 1.0 };
            double p[4];
            for (int r = 0; r < 4; ++r) p[r] = inv[r] * ndc[0] + inv[4 + r] * ndc[1] + inv[8 + r] * ndc[2] + inv[12 + r] * ndc[3];
            if (!(std::fabs(p[3]) > 0.0)) return zr_fail(c, ZR_ERR_STATE, "zr_camera_ray: Proj * View has no inverse");
            for (int k = 0; k < 3; ++k) ends[e][k] = p[k] / p[3];
        }
        for (int k = 0; k < 3; ++k) { out->origin[k] = (float)ends[0][k]; out->dir[k] = (float)(ends[1][k] - ends[0][k]); }
        out->t_min = 0.0f; out->t_max = 1.0f;
        return ZR_OK;
    });
}

extern "C" int zr_ray_triangles(const zr_ray* rays, uint32_t n_rays, const float* tris, uint32_t n_tris, uint32_t flags, zr_ray_hit* hits)
{
    if ((n_rays && (!rays || !hits)) || (n_rays && n_tris && !tris) || (flags & ~ZR_RAY_QUERY_FLAGS)) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        zr_rc_triangles(rays, n_rays, tris, n_tris, flags, hits);
        return ZR_OK;
    });
}
