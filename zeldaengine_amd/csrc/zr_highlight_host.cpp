// zr_highlight_host.cpp — highlighting a selection behind the C-ABI (zelda_render.h, "highlighting a selection"): the set and the style
// (host state of the context: zr_ctx::hl), the set's way to the device (hl_upload), the switch that makes the deliveries of changes
// carry the highlight, and the context-free host statement of the rule (zr_highlight.h).  The deliveries themselves - the highlighted
// frame in a host form and a device form, and the changes - are zr_deliver_host.cpp's: its source stage launches zr_highlight.hip.
//
// The set against deliveries in flight.  The set calls change host bytes only.  The first delivery after a change packs them into a
// bit per slot and sends that through the pinned staging ring ON THE RENDER STREAM into the device bitset, ahead of its own launches:
// stream order puts the copy behind every delivery enqueued before it - which keeps the set it was enqueued with - and no frame waits
// for anything.
#include "zr_ctx.h"
#include "zr_highlight.h"

#include <cstring>

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

// The device bitset brought up to the host's set, on the render stream
int hl_upload(zr_ctx* c)
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

extern "C" int zr_set_frame_delta_highlight(zr_ctx* c, int on)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->delta.on) return zr_fail(c, ZR_ERR_STATE, "zr_set_frame_delta_highlight: frame delta is on (zr_set_frame_delta(ctx, 0) first)");
        c->hl.delta = on != 0;
        return ZR_OK;
    });
}
