// zr_texture_update_host.cpp — changing material textures between frames: zr_object_set_texture (host data, through the pinned staging
// ring), zr_object_update_texture_async (caller-owned device data, in the order of the caller's stream) and zr_object_get_texture.
// Kernels: zr_texture_update.hip.
//
// Ordering ("Changing textures").  The slot's mip chain and the packed material are rewritten IN PLACE - a parity copy of
// every texture would double the largest allocations of a textured scene - so an update is ordered against the frames on both sides:
//   - the update's stream x first waits for the end of the frame enqueued last (ev_end: that frame's lighting pass, which itself waited
//     for the camera lane - k_resolve_gbuffer there and k_forward on the render stream are the readers), so frames already enqueued
//     sample the old image;
//   - x waits for the update before (ev_tex): updates land in call order;
//   - the next frame's first stream waits for ev_tex (zr_update_frame); the frame's other lane joins that stream before it samples.
// The waits and the record are zr_update_tex_begin / zr_update_tex_end (zr_update.cpp); nothing else is invalidated.
#include <cstring>

#include "zr_ctx.h"

// the refusals both forms share; *out = the object
static int tex_slot(zr_ctx* c, uint32_t index, uint32_t slot, const void* data, uint32_t w, uint32_t h, const char* what, ZrSceneObject** out)
{
    if (int rc = zr_stage_idle(c, what)) return rc;
    if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": bad object index");
    if (slot > 6u) return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": slot " + std::to_string(slot) + " (0..6: bc, m, r, n, ao, ev, ms)");
    if (!data || ((uintptr_t)data & 3u)) return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": image data missing or not 4-byte aligned");
    ZrSceneObject& o = c->objects[index];
    if (!o.d_tex[slot])
        return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": slot " + std::to_string(slot) + " of object " + std::to_string(index) +
                                        " holds no image (zr_object_add took the engine default or collapsed a constant image to its texel): "
                                        "a slot meant to change must be added with a non-constant image of its final size");
    if (w != o.tex_w[slot] || h != o.tex_h[slot])
        return zr_fail(c, ZR_ERR_ARG, std::string(what) + ": image is " + std::to_string(w) + " x " + std::to_string(h) + ", the slot holds " +
                                      std::to_string(o.tex_w[slot]) + " x " + std::to_string(o.tex_h[slot]) + " (the size is fixed at zr_object_add)");
    *out = &o;
    return ZR_OK;
}

// the slot's chain (and packed bytes) from src on stream x, between the frame enqueued last and the next one
static int tex_enqueue(zr_ctx* c, ZrSceneObject& o, uint32_t slot, const void* src, hipStream_t x)
{
    ZrTexUpdate U; memset(&U, 0, sizeof U);
    U.chain = (uint32_t*)o.d_tex[slot]; U.packed = o.d_tex[7];
    U.srgb_lut = c->d_lut; U.unorm_lut = c->d_unorm_lut;
    U.w = o.tex_w[slot]; U.h = o.tex_h[slot]; U.levels = o.tex_levels[slot]; U.srgb = slot == 0u ? 1u : 0u;
    U.pk_ch = kSlotPack[slot].ch; U.pk_n = kSlotPack[slot].n;
    if (U.levels == 0 || U.levels > 16u) return zr_fail(c, ZR_ERR_STATE, "texture update: the slot's chain has no levels");
    for (uint32_t l = 0; l < U.levels; ++l) {       // build_mip_chain's sizes and steps
        const ZrMipLevel S = zr_mip_level(U.w, U.h, l ? l - 1 : 0), D = zr_mip_level(U.w, U.h, l);
        U.off[l] = (uint32_t)D.off; U.kx[l] = (float)S.w / (float)D.w; U.ky[l] = (float)S.h / (float)D.h;
    }
    int rc = zr_update_tex_begin(c, x);
    if (rc) return rc;
    U.srgb_thr = c->upd.d_srgb_thr;
    zr_launch_texture_update(U, (const uint32_t*)src, x);
    rc = zr_update_tex_end(c, x);
    if (rc) return rc;
    o.mat_pristine = false;             // (a world update rebuilds the material from its Profab)
    return ZR_OK;
}

extern "C" int zr_object_set_texture(zr_ctx* c, uint32_t index, uint32_t slot, const zr_image* img)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrSceneObject* o = nullptr;
        int rc = tex_slot(c, index, slot, img ? (const void*)img->rgba8 : nullptr, img ? img->width : 0u, img ? img->height : 0u, "zr_object_set_texture", &o);
        if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        return zr_update_host_form(c, img->rgba8, (size_t)img->width * img->height * 4u, [&](const void* staged, hipStream_t x) {
            return tex_enqueue(c, *o, slot, staged, x);
        });
    });
}

extern "C" int zr_object_update_texture_async(zr_ctx* c, uint32_t index, uint32_t slot, const void* rgba8_dev, uint32_t width, uint32_t height, void* hip_stream)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrSceneObject* o = nullptr;
        int rc = tex_slot(c, index, slot, rgba8_dev, width, height, "zr_object_update_texture_async", &o);
        if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        return tex_enqueue(c, *o, slot, rgba8_dev, hip_stream ? (hipStream_t)hip_stream : c->stream);
    });
}

extern "C" int zr_object_get_texture(zr_ctx* c, uint32_t index, uint32_t slot, uint32_t level, uint8_t* dst, size_t cap, uint32_t* w, uint32_t* h, uint32_t* levels)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, "zr_object_get_texture: bad object index");
        if (slot > 6u) return zr_fail(c, ZR_ERR_ARG, "zr_object_get_texture: slot " + std::to_string(slot) + " (0..6)");
        const ZrSceneObject& o = c->objects[index];
        if (!o.d_tex[slot]) return zr_fail(c, ZR_ERR_STATE, "zr_object_get_texture: slot " + std::to_string(slot) + " of object " + std::to_string(index) + " holds no image");
        if (level >= o.tex_levels[slot]) return zr_fail(c, ZR_ERR_ARG, "zr_object_get_texture: level " + std::to_string(level) + " of " + std::to_string(o.tex_levels[slot]));
        const ZrMipLevel L = zr_mip_level(o.tex_w[slot], o.tex_h[slot], level);
        if (w) *w = L.w;
        if (h) *h = L.h;
        if (levels) *levels = o.tex_levels[slot];
        if (!dst) return ZR_OK;
        const size_t bytes = (size_t)L.w * L.h * 4u;
        if (cap < bytes) return zr_fail(c, ZR_ERR_ARG, "zr_object_get_texture: the level needs " + std::to_string(bytes) + " bytes");
        HIPCHK(c, hipSetDevice(c->device));
        if (c->upd.ev_tex) HIPCHK(c, hipEventSynchronize(c->upd.ev_tex));      // the last update has landed in the chain
        HIPCHK(c, hipMemcpy(dst, o.d_tex[slot] + L.off * 4u, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
