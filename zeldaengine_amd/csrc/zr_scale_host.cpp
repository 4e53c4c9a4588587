// zr_scale_host.cpp — delivering a scaled frame behind the C-ABI (zelda_render.h, "delivering a scaled frame"): the frame box-filtered by
// an integer factor in linear light (zr_scale.h has the rule), in a host form and a device form, the context-free host statement of the
// filter, and the scale the deliveries of changes work at (zr_delta_host.cpp).  Like a delivery of changes, a scaled frame is no stage of
// the frame: it is one launch (zr_scale.hip) on the render stream behind the lighting pass of the frame enqueued last, where
// zr_copy_frame_async's copy goes, and the frame schedule knows nothing of it.
#include "zr_ctx.h"
#include "zr_scale.h"

static bool scale_ok(uint32_t s) { return s >= 1u && s <= kZrScaleMax; }

extern "C" int zr_frame_scaled_extent(uint32_t width, uint32_t height, uint32_t scale, uint32_t* w, uint32_t* h)
{
    if (!w || !h || !width || !height || !scale_ok(scale)) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        *w = zr_scale_extent(width, scale); *h = zr_scale_extent(height, scale);
        return ZR_OK;
    });
}

extern "C" int zr_frame_downscale(const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t scale, uint8_t* dst, size_t bytes)
{
    if (!rgba8 || !dst || !width || !height || !scale_ok(scale)) return ZR_ERR_ARG;
    if (bytes != (size_t)zr_scale_extent(width, scale) * zr_scale_extent(height, scale) * 4u) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        zr_scale_frame(rgba8, width, height, scale, dst);
        return ZR_OK;
    });
}

// The context's lighting pass writes the row-major frame, and the frame enqueued last is a finished one
int scale_ready(zr_ctx* c, const char* what)
{
    if (c->cfg.tile_world > 1 || (c->cfg.flags & ZR_FLAG_PACKED_TILES))
        return zr_fail(c, ZR_ERR_UNSUPPORTED, std::string(what) + ": this context's lighting pass writes packed tiles, not the frame (tile_world > 1, ZR_FLAG_PACKED_TILES)");
    if (int rc = zr_stage_idle(c, what)) return rc;
    if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": no finished frame enqueued");
    return ZR_OK;
}

extern "C" int zr_read_color_scaled(zr_ctx* c, uint32_t scale, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && scale_ok(scale));
        ARGCHK(c, bytes == (size_t)zr_scale_extent(c->W, scale) * zr_scale_extent(c->H, scale) * 4u);
        int rc = scale_ready(c, "zr_read_color_scaled");
        if (rc == ZR_OK) rc = zr_finish(c);
        if (rc) return rc;
        if (scale == 1u) { HIPCHK(c, hipMemcpy(dst, c->d_color, bytes, hipMemcpyDeviceToHost)); return ZR_OK; }
        if (!c->d_scaled) HIPCHK(c, c->ext.alloc(&c->d_scaled, (size_t)zr_scale_extent(c->W, 2u) * zr_scale_extent(c->H, 2u)));
        zr_launch_frame_scale(c->d_color, c->d_scaled, c->W, c->H, scale, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(dst, c->d_scaled, bytes, hipMemcpyDeviceToHost));      // (the scaled frame is all that crosses the link)
        return ZR_OK;
    });
}

extern "C" int zr_copy_frame_scaled_async(zr_ctx* c, uint32_t scale, void* color_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, color_dev && (uintptr_t)color_dev % 4 == 0 && scale_ok(scale));
        if (int rc = scale_ready(c, "zr_copy_frame_scaled_async")) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        zr_launch_frame_scale(c->d_color, (uint32_t*)color_dev, c->W, c->H, scale, c->stream);
        HIPCHK(c, hipGetLastError());
        return ZR_OK;
    });
}

extern "C" int zr_set_frame_delta_scale(zr_ctx* c, uint32_t scale)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, scale_ok(scale));
        if (c->delta.on) return zr_fail(c, ZR_ERR_STATE, "zr_set_frame_delta_scale: frame delta is on (zr_set_frame_delta(ctx, 0) first)");
        c->delta.scale = scale;
        return ZR_OK;
    });
}

extern "C" int zr_get_frame_delta_extent(zr_ctx* c, uint32_t* width, uint32_t* height, uint32_t* total_tiles, uint32_t* scale)
{
    if (!c || !width || !height || !total_tiles || !scale) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const ZrDeltaExtent E = zr_delta_extent(c);
        *width = E.W; *height = E.H; *total_tiles = E.n_tiles; *scale = c->delta.scale;
        return ZR_OK;
    });
}
