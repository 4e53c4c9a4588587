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
//   - the next frame's first stream waits for ev_tex (zr_texture_frame); the frame's other lane joins that stream before it samples.
// No list, plan, history or shadow map depends on a texel: nothing else is invalidated (zr_update_end is not for these updates).
#include <cstring>

#include "zr_ctx.h"
#include "zr_srgb.h"

// first byte and channel count of a slot in the packed texel: kPack of zr_object_add_internal
static const struct { uint32_t ch, n; } kSlotPack[7] = { { ZR_PK_BC, 3 }, { ZR_PK_ME, 1 }, { ZR_PK_RO, 1 }, { ZR_PK_NO, 3 }, { ZR_PK_AO, 1 }, { ZR_PK_EM, 3 }, { ZR_PK_MS, 1 } };

static int tex_init_ctx(zr_ctx* c)
{
    if (c->ev_tex) return ZR_OK;
    if (!c->d_srgb_thr) {
        float thr[256];
        zr_srgb_thresholds(thr);
        HIPCHK(c, c->own.alloc(&c->d_srgb_thr, 256));
        HIPCHK(c, hipMemcpy(c->d_srgb_thr, thr, sizeof thr, hipMemcpyHostToDevice));
    }
    HIPCHK(c, c->own.event(&c->ev_tex, hipEventDisableTiming));      // (last: it marks the set as made)
    return ZR_OK;
}

// the refusals both forms share; *out = the object
static int tex_slot(zr_ctx* c, uint32_t index, uint32_t slot, const void* data, uint32_t w, uint32_t h, const char* what, ZrSceneObject** out)
{
    if (c->stage != 0) return zr_fail(c, ZR_ERR_STATE, std::string(what) + " between the stages of a frame (finish it with zr_render_lighting first)");
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
    int rc = tex_init_ctx(c);
    if (rc) return rc;
    ZrTexUpdate U; memset(&U, 0, sizeof U);
    U.chain = (uint32_t*)o.d_tex[slot]; U.packed = o.d_tex[7];
    U.srgb_lut = c->d_lut; U.unorm_lut = c->d_unorm_lut; U.srgb_thr = c->d_srgb_thr;
    U.w = o.tex_w[slot]; U.h = o.tex_h[slot]; U.levels = o.tex_levels[slot]; U.srgb = slot == 0u ? 1u : 0u;
    U.pk_ch = kSlotPack[slot].ch; U.pk_n = kSlotPack[slot].n;
    if (U.levels == 0 || U.levels > 16u) return zr_fail(c, ZR_ERR_STATE, "texture update: the slot's chain has no levels");
    uint32_t off = 0, sw = U.w, sh = U.h;
    for (uint32_t l = 0; l < U.levels; ++l) {       // build_mip_chain's sizes and steps
        const uint32_t dw = l ? (sw > 1 ? sw >> 1 : 1) : sw, dh = l ? (sh > 1 ? sh >> 1 : 1) : sh;
        U.off[l] = off; U.kx[l] = (float)sw / (float)dw; U.ky[l] = (float)sh / (float)dh;
        off += dw * dh; sw = dw; sh = dh;
    }
    // the readers of the old image: the frame enqueued last, on both lanes (on the render stream its lighting pass is ahead of this point)
    if (c->frame_no >= 1 && x != c->stream) HIPCHK(c, hipStreamWaitEvent(x, c->ev_end[(c->frame_no - 1) % zr_ctx::END_RING], 0));
    if (c->tex_s && c->tex_s != x) HIPCHK(c, hipStreamWaitEvent(x, c->ev_tex, 0));
    zr_launch_texture_update(U, (const uint32_t*)src, x);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_tex, x));
    c->tex_s = x; c->tex_wait = true;
    o.mat_pristine = false;             // (a world update rebuilds the material from its Profab)
    return ZR_OK;
}

// frame_begin on stream s: the frame's first stream behind the last update.  (Later frames follow this one on s, or wait for its end.)
int zr_texture_frame(zr_ctx* c, hipStream_t s)
{
    if (!c->tex_wait) return ZR_OK;
    if (c->tex_s != s) HIPCHK(c, hipStreamWaitEvent(s, c->ev_tex, 0));
    c->tex_wait = false;
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
        hipStream_t x = c->cam_s ? c->cam_s : c->stream;      // the camera lane, as zr_object_set_instances
        void* staged = nullptr; hipEvent_t ev = nullptr;
        rc = zr_update_stage(c, x, img->rgba8, (size_t)img->width * img->height * 4u, &staged, &ev);
        if (rc) return rc;
        rc = tex_enqueue(c, *o, slot, staged, x);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(ev, x));
        return ZR_OK;
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
        size_t off = 0;
        uint32_t lw = o.tex_w[slot], lh = o.tex_h[slot];
        for (uint32_t l = 0; l < level; ++l) { off += (size_t)lw * lh * 4u; lw = lw > 1 ? lw >> 1 : 1; lh = lh > 1 ? lh >> 1 : 1; }
        if (w) *w = lw;
        if (h) *h = lh;
        if (levels) *levels = o.tex_levels[slot];
        if (!dst) return ZR_OK;
        const size_t bytes = (size_t)lw * lh * 4u;
        if (cap < bytes) return zr_fail(c, ZR_ERR_ARG, "zr_object_get_texture: the level needs " + std::to_string(bytes) + " bytes");
        HIPCHK(c, hipSetDevice(c->device));
        if (c->ev_tex) HIPCHK(c, hipEventSynchronize(c->ev_tex));      // the last update has landed in the chain
        HIPCHK(c, hipMemcpy(dst, o.d_tex[slot] + off, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
