// zr_highlight_host.cpp — highlighting a selection behind the C-ABI (zelda_render.h, "highlighting a selection"): the set and the style
// (host state of the context: zr_ctx::hl), the highlighted frame in a host form and a device form, the switch that makes the deliveries
// of changes carry it (zr_delta_host.cpp), and the context-free host statement of the rule (zr_highlight.h).  Like a scaled frame, a
// highlighted one is no stage of the frame: two launches (zr_highlight.hip) on the render stream behind the lighting pass of the frame
// enqueued last, and the frame schedule knows nothing of it.
//
// The set against deliveries in flight.  The set calls change host bytes only.  The first delivery after a change packs them into a
// bit per slot and sends that through the pinned staging ring ON THE RENDER STREAM into the device bitset, ahead of its own launches:
// stream order puts the copy behind every delivery enqueued before it - which keeps the set it was enqueued with - and no frame waits
// for anything.
#include "zr_ctx.h"
#include "zr_highlight.h"

#include <cstring>

static bool scale_ok(uint32_t s) { return s >= 1u && s <= 8u; }

// The set as the scene stands: when the object list changed since it was sized (scene_gen moved), it is empty, at the new slot count
static void hl_current(zr_ctx* c)
{
    zr_ctx::Highlight& L = c->hl;
    const size_t slots = ids_slot_count(c);
    if (L.set_gen == c->scene_gen && L.set.size() == slots) return;
    L.set.assign(slots, 0);
    L.set_gen = c->scene_gen; L.dirty = true;
}

extern "C" int zr_highlight_set(zr_ctx* c, uint32_t object, uint32_t first, const uint8_t* on, uint32_t n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (object >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, "zr_highlight_set: bad object index");
        const ZrSceneObject& o = c->objects[object];
        if ((uint64_t)first + n > o.n_inst)
            return zr_fail(c, ZR_ERR_ARG, "zr_highlight_set: instances [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) +
                                          ") beyond the object's " + std::to_string(o.n_inst));
        if (n == 0) return ZR_OK;
        if (!on) return zr_fail(c, ZR_ERR_ARG, "zr_highlight_set: no data");
        hl_current(c);
        size_t base = first;
        for (uint32_t i = 0; i < object; ++i) base += c->objects[i].n_inst;
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t v = on[i] ? 1 : 0;
            if (c->hl.set[base + i] != v) { c->hl.set[base + i] = v; c->hl.dirty = true; }
        }
        return ZR_OK;
    });
}

extern "C" int zr_highlight_clear(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        hl_current(c);
        for (uint8_t& v : c->hl.set) if (v) { v = 0; c->hl.dirty = true; }
        return ZR_OK;
    });
}

extern "C" int zr_highlight_get(zr_ctx* c, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (dst || bytes == 0) && bytes == ids_slot_count(c));
        hl_current(c);
        if (bytes) memcpy(dst, c->hl.set.data(), bytes);
        return ZR_OK;
    });
}

extern "C" int zr_set_highlight_style(zr_ctx* c, const zr_highlight_style* style, size_t bytes)
{
    if (!c || !style) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes == sizeof(zr_highlight_style));
        if (!zr_hl_style_ok(style)) return zr_fail(c, ZR_ERR_ARG, "zr_set_highlight_style: radius above 8, or reserved not 0");
        c->hl.style = *style;
        return ZR_OK;
    });
}

extern "C" int zr_get_highlight_style(zr_ctx* c, zr_highlight_style* style, size_t bytes)
{
    if (!c || !style) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes == sizeof(zr_highlight_style));
        *style = c->hl.style;
        return ZR_OK;
    });
}

extern "C" int zr_frame_highlight(const uint8_t* rgba8, const uint8_t* mask, uint32_t width, uint32_t height, const zr_highlight_style* style, size_t style_bytes,
                                  uint8_t* dst, size_t bytes)
{
    if (!rgba8 || !mask || !style || !dst || !width || !height || style_bytes != sizeof(zr_highlight_style)) return ZR_ERR_ARG;
    if (!zr_hl_style_ok(style) || bytes != (size_t)width * height * 4u) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        zr_hl_frame(rgba8, mask, width, height, style, dst);
        return ZR_OK;
    });
}

int zr_highlight_ready(zr_ctx* c, const char* what)
{
    if (int rc = scale_ready(c, what)) return rc;
    return ids_ready(c, what, false);
}

// The device bitset brought up to the host's set, on the render stream
static int hl_upload(zr_ctx* c)
{
    zr_ctx::Highlight& L = c->hl;
    hl_current(c);
    const size_t words = (L.set.size() + 31u) / 32u;
    if (!L.bits || words > L.bits_words) {
        if (L.bits) HIPCHK(c, zr_sync_all(c));           // (deliveries in flight read the old one)
        L.bits_mem.release(); L.bits = nullptr; L.bits_words = 0;
        HIPCHK(c, L.bits_mem.alloc(&L.bits, words));
        L.bits_words = words ? words : 1u;
        L.dirty = true;
    }
    if (!L.dirty) return ZR_OK;
    std::vector<uint32_t> packed(L.bits_words, 0u);
    for (size_t i = 0; i < L.set.size(); ++i) if (L.set[i]) packed[i >> 5] |= 1u << (i & 31u);
    const size_t bytes = packed.size() * 4u;
    int rc = zr_update_host_form_on(c, c->stream, packed.data(), bytes, [&](const void* staged, hipStream_t x) -> int {
        HIPCHK(c, hipMemcpyAsync(L.bits, staged, bytes, hipMemcpyDeviceToDevice, x));
        return ZR_OK;
    });
    if (rc) return rc;
    L.dirty = false;
    return ZR_OK;
}

int zr_highlight_enqueue(zr_ctx* c, uint32_t* dst, const uint32_t** out)
{
    zr_ctx::Highlight& L = c->hl;
    if (!L.plane) HIPCHK(c, c->ext.alloc(&L.plane, (size_t)zr_hl_row_words(c->W) * c->H));
    if (!dst && !L.frame) HIPCHK(c, c->ext.alloc(&L.frame, (size_t)c->W * c->H));
    if (int rc = hl_upload(c)) return rc;
    uint32_t* to = dst ? dst : L.frame;
    const ZrIdsArgs A = ids_args(c, 0, 0, c->W, c->H);
    zr_launch_highlight_mask(A.prim, A.draws, A.n_draws, L.bits, L.plane, c->W, c->H, c->stream);
    zr_launch_highlight_apply(c->d_color, L.plane, to, c->W, c->H, L.style, c->stream);
    HIPCHK(c, hipGetLastError());
    // the mask reads the last frame's winner plane: the frame that writes that copy next (the one after next) waits for it
    HIPCHK(c, hipEventRecord(c->fc[c->fcur].ev_ids, c->stream));
    c->fc[c->fcur].ids_wait = true;
    if (out) *out = to;
    return ZR_OK;
}

// ... then filtered by `scale` into dst (scale 1: highlighted straight into dst)
static int hl_deliver(zr_ctx* c, uint32_t scale, uint32_t* dst)
{
    if (scale == 1u) return zr_highlight_enqueue(c, dst, nullptr);
    const uint32_t* hl = nullptr;
    if (int rc = zr_highlight_enqueue(c, nullptr, &hl)) return rc;
    zr_launch_frame_scale(hl, dst, c->W, c->H, scale, c->stream);
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}

extern "C" int zr_read_color_highlighted(zr_ctx* c, uint32_t scale, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && scale_ok(scale));
        ARGCHK(c, bytes == (size_t)((c->W + scale - 1u) / scale) * ((c->H + scale - 1u) / scale) * 4u);
        int rc = zr_highlight_ready(c, "zr_read_color_highlighted");
        if (rc == ZR_OK) rc = zr_finish(c);
        if (rc) return rc;
        const uint32_t* src = nullptr;
        if (scale == 1u) rc = zr_highlight_enqueue(c, nullptr, &src);
        else {
            if (!c->d_scaled) HIPCHK(c, c->ext.alloc(&c->d_scaled, (size_t)((c->W + 1u) / 2u) * ((c->H + 1u) / 2u)));
            rc = hl_deliver(c, scale, c->d_scaled);
            src = c->d_scaled;
        }
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}

extern "C" int zr_copy_frame_highlighted_async(zr_ctx* c, uint32_t scale, void* color_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, color_dev && (uintptr_t)color_dev % 4 == 0 && scale_ok(scale));
        if (int rc = zr_highlight_ready(c, "zr_copy_frame_highlighted_async")) return rc;
        return hl_deliver(c, scale, (uint32_t*)color_dev);
    });
}

extern "C" int zr_set_frame_delta_highlight(zr_ctx* c, int on)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->delta.on) return zr_fail(c, ZR_ERR_STATE, "zr_set_frame_delta_highlight: frame delta is on (zr_set_frame_delta(ctx, 0) first)");
        c->hl.delta = on != 0;
        return ZR_OK;
    });
}
