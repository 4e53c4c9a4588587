// zr_overlay_host.cpp — overlaying lines behind the C-ABI (zelda_render.h, "overlaying lines"): the list and the style (host state of
// the context: zr_ctx::ov), the list's way to the device and the two launches of a delivery's overlay stage (zr_overlay_stage, which
// zr_deliver_host.cpp's source stage calls between the highlight and the filter), the overlaid frame in a host form and a device form,
// the switch that makes the deliveries of changes carry the lines, and the context-free host statement of the rule (zr_overlay.h).
//
// The list against deliveries in flight.  zr_overlay_set changes host bytes only.  The first delivery after a change sends them through
// the pinned staging ring ON THE RENDER STREAM into the device list, ahead of its own launches: stream order puts the copy behind every
// delivery enqueued before it - which keeps the list it was enqueued with - and no frame waits for anything.  The records and
// rectangles are rewritten by every delivery's set-up launch, for the camera of the frame it delivers, in the same order.
// The camera is zr_ctx::cam_prev_key's: the pass block the camera pass of the frame enqueued last was drawn from (a frame that keeps
// its camera pass has that very block, or it would not keep), so uniforms set after that frame move nothing.
// The depth plane is fc[fcur].G.depth, which the resolve of the frame after next rewrites - on the camera lane, where stream order
// says nothing: the stage notes its read as the highlight's mask notes its own (ids_reader_enqueued), and that frame's head waits.
#include "zr_ctx.h"

#include <cstring>

extern "C" int zr_overlay_set(zr_ctx* c, const zr_overlay_segment* seg, uint32_t n)
{
    if (!c || (n && !seg) || n > ZR_OVERLAY_MAX_SEGMENTS) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i)
            if (!zr_ov_flags_ok(seg[i].flags)) return zr_fail(c, ZR_ERR_ARG, "zr_overlay_set: segment " + std::to_string(i) + " has an unknown flag bit");
        std::vector<zr_overlay_segment> next(seg, seg + n);      // (may throw: the list stays)
        c->ov.seg.swap(next);
        c->ov.dirty = true;
        return ZR_OK;
    });
}

extern "C" int zr_overlay_get(zr_ctx* c, zr_overlay_segment* dst, uint32_t* n)
{
    if (!c || !n) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const uint32_t room = *n, have = (uint32_t)c->ov.seg.size();
        *n = have;
        if (!dst) return ZR_OK;
        if (room < have) return zr_fail(c, ZR_ERR_ARG, "zr_overlay_get: room for " + std::to_string(room) + " of " + std::to_string(have) + " segments");
        if (have) memcpy(dst, c->ov.seg.data(), (size_t)have * sizeof(zr_overlay_segment));
        return ZR_OK;
    });
}

extern "C" int zr_set_overlay_style(zr_ctx* c, const zr_overlay_style* style, size_t bytes)
{
    if (!c || !style) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes == sizeof(zr_overlay_style));
        if (!zr_ov_style_ok(style)) return zr_fail(c, ZR_ERR_ARG, "zr_set_overlay_style: depth_bias negative or not finite, hidden_opacity above 255, or reserved not 0");
        c->ov.style = *style;
        return ZR_OK;
    });
}

extern "C" int zr_get_overlay_style(zr_ctx* c, zr_overlay_style* style, size_t bytes)
{
    if (!c || !style) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes == sizeof(zr_overlay_style));
        *style = c->ov.style;
        return ZR_OK;
    });
}

extern "C" int zr_frame_overlay(const uint8_t* rgba8, const float* depth, uint32_t width, uint32_t height, const float* pvm, const zr_overlay_segment* seg, uint32_t n,
                                const zr_overlay_style* style, size_t style_bytes, uint8_t* dst, size_t bytes)
{
    if (!rgba8 || !depth || !pvm || !style || !dst || !width || !height || (n && !seg) || style_bytes != sizeof(zr_overlay_style)) return ZR_ERR_ARG;
    if (n > ZR_OVERLAY_MAX_SEGMENTS || !zr_ov_style_ok(style) || bytes != (size_t)width * height * 4u) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i) if (!zr_ov_flags_ok(seg[i].flags)) return ZR_ERR_ARG;
        zr_ov_frame(rgba8, depth, width, height, pvm, seg, n, style, dst);
        return ZR_OK;
    });
}

// The device list brought up to the host's, on the render stream
static int ov_upload(zr_ctx* c)
{
    zr_ctx::Overlay& L = c->ov;
    const size_t n = L.seg.size();
    if (n > L.cap) {
        if (L.cap) HIPCHK(c, zr_sync_all(c));            // (deliveries in flight read the old buffers)
        L.mem.release(); L.d_seg = nullptr; L.recs = nullptr; L.rects = nullptr; L.cap = 0;
        size_t cap = 256;
        while (cap < n) cap *= 2;
        HIPCHK(c, L.mem.alloc(&L.d_seg, cap)); HIPCHK(c, L.mem.alloc(&L.recs, cap)); HIPCHK(c, L.mem.alloc(&L.rects, cap));
        L.cap = cap; L.dirty = true;
    }
    if (!L.dirty) return ZR_OK;
    const size_t bytes = n * sizeof(zr_overlay_segment);
    int rc = zr_update_host_form_on(c, c->stream, L.seg.data(), bytes, [&](const void* staged, hipStream_t x) -> int {
        HIPCHK(c, hipMemcpyAsync(L.d_seg, staged, bytes, hipMemcpyDeviceToDevice, x));
        return ZR_OK;
    });
    if (rc) return rc;
    L.dirty = false;
    return ZR_OK;
}

int zr_overlay_stage(zr_ctx* c, const uint32_t* src, uint32_t* dst, const uint32_t** out)
{
    zr_ctx::Overlay& L = c->ov;
    const uint32_t n = (uint32_t)L.seg.size();
    if (!dst && !L.frame) HIPCHK(c, c->ext.alloc(&L.frame, (size_t)c->W * c->H));
    if (int rc = ov_upload(c)) return rc;
    uint32_t* const to = dst ? dst : L.frame;
    const ZrPass& P = c->cam_prev_key;
    zr_launch_overlay_setup(L.d_seg, n, P.PVM, P.hw, P.hh, c->W, c->H, L.recs, L.rects, c->stream);
    zr_launch_overlay_apply(src, c->fc[c->fcur].G.depth, L.recs, L.rects, n, to, c->W, c->H, L.style, c->stream);
    if (int rc = ids_reader_enqueued(c)) return rc;      // (the apply read the last frame's depth plane)
    *out = to;
    return ZR_OK;
}

extern "C" int zr_read_color_overlaid(zr_ctx* c, uint32_t scale, int highlight, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return zr_deliver_to_host(c, "zr_read_color_overlaid", { false, highlight != 0, true, scale }, dst, bytes); });
}

extern "C" int zr_copy_frame_overlaid_async(zr_ctx* c, uint32_t scale, int highlight, void* color_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return zr_deliver_to_device(c, "zr_copy_frame_overlaid_async", { false, highlight != 0, true, scale }, color_dev); });
}

extern "C" int zr_set_frame_delta_overlay(zr_ctx* c, int on)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->delta.on) return zr_fail(c, ZR_ERR_STATE, "zr_set_frame_delta_overlay: frame delta is on (zr_set_frame_delta(ctx, 0) first)");
        c->ov.delta = on != 0;
        return ZR_OK;
    });
}
