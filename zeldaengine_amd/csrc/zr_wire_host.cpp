// zr_wire_host.cpp — the wireframe behind the C-ABI (zelda_render.h, "wireframe"): the style (host state of the context: zr_ctx::wire),
// the one launch of a delivery's wire stage (zr_wire_stage, which zr_deliver_host.cpp's source stage calls first of all), the staged
// deliveries - one call for every combination of wire, highlight and overlay, in a host form and a device form - the switch that makes
// the deliveries of changes carry the wire, and the context-free host statement of the rule (zr_wire.h).
//
// What the stage reads is the frame enqueued last, exactly as a ray cast and the highlight's mask do: that frame's winner plane and the
// census's table (ids_args), zr_ctx::d_objs - its draw table, off which its parity's instance planes and mesh sets hang - and
// cam_prev_key, the block its camera pass was drawn from (PVM, hw, hh): uniforms set after that frame move nothing.  The frame after
// next rewrites the planes and sets of this parity at its head, on the camera lane, where stream order says nothing: the launch is
// noted (ids_reader_enqueued) and that frame's head waits.  A scene that no update has split into parities yet is read from parity 0
// by every frame, and the first update makes the very next frame the writer: there the launch is noted in both copies.
// A selected-only style reads the highlight's bitset, brought up to the host's set on the render stream first (hl_upload).
#include "zr_ctx.h"
#include "zr_wire.h"

#include <cstring>

extern "C" int zr_set_wire_style(zr_ctx* c, const zr_wire_style* style, size_t bytes)
{
    if (!c || !style) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes == sizeof(zr_wire_style));
        if (!zr_wire_style_ok(style)) return zr_fail(c, ZR_ERR_ARG, "zr_set_wire_style: width_256 outside 1..4096, an unknown flag, or reserved not 0");
        c->wire.style = *style;
        return ZR_OK;
    });
}

extern "C" int zr_get_wire_style(zr_ctx* c, zr_wire_style* style, size_t bytes)
{
    if (!c || !style) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes == sizeof(zr_wire_style));
        *style = c->wire.style;
        return ZR_OK;
    });
}

int zr_wire_stage(zr_ctx* c, const uint32_t* src, uint32_t* dst, const uint32_t** out)
{
    zr_ctx::Wire& L = c->wire;
    const bool only = (L.style.flags & ZR_WIRE_SELECTED) != 0u;
    if (!dst && !L.frame) HIPCHK(c, c->ext.alloc(&L.frame, (size_t)c->W * c->H));
    if (only)
        if (int rc = hl_upload(c)) return rc;
    const ZrIdsArgs I = ids_args(c, 0, 0, c->W, c->H);
    const ZrPass& P = c->cam_prev_key;
    ZrWireArgs A; memset(&A, 0, sizeof A);
    A.frame = src; A.prim = I.prim; A.dst = dst ? dst : L.frame;
    A.draws = I.draws; A.n_draws = I.n_draws; A.objs = c->d_objs; A.set_bits = only ? c->hl.bits : nullptr;
    A.W = c->W; A.H = c->H; A.colour = zr_hl_pack(L.style.rgba); A.width_256 = L.style.width_256;
    memcpy(A.PVM, P.PVM, sizeof A.PVM); A.hw = P.hw; A.hh = P.hh;
    zr_launch_wire_apply(A, c->stream);
    HIPCHK(c, hipGetLastError());
    if (int rc = ids_reader_enqueued(c, !c->upd.dual)) return rc;
    *out = A.dst;
    return ZR_OK;
}

static ZrDeliverWhat staged(uint32_t stages, uint32_t scale)
{
    return { (stages & ZR_STAGE_WIRE) != 0u, (stages & ZR_STAGE_HIGHLIGHT) != 0u, (stages & ZR_STAGE_OVERLAY) != 0u, scale };
}
static constexpr uint32_t kStages = ZR_STAGE_WIRE | ZR_STAGE_HIGHLIGHT | ZR_STAGE_OVERLAY;

extern "C" int zr_read_color_staged(zr_ctx* c, uint32_t stages, uint32_t scale, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (stages & ~kStages) == 0u);
        return zr_deliver_to_host(c, "zr_read_color_staged", staged(stages, scale), dst, bytes);
    });
}

extern "C" int zr_copy_frame_staged_async(zr_ctx* c, uint32_t stages, uint32_t scale, void* color_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (stages & ~kStages) == 0u);
        return zr_deliver_to_device(c, "zr_copy_frame_staged_async", staged(stages, scale), color_dev);
    });
}

extern "C" int zr_set_frame_delta_wire(zr_ctx* c, int on)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->delta.on) return zr_fail(c, ZR_ERR_STATE, "zr_set_frame_delta_wire: frame delta is on (zr_set_frame_delta(ctx, 0) first)");
        c->wire.delta = on != 0;
        return ZR_OK;
    });
}

extern "C" int zr_frame_wire(const uint8_t* rgba8, const uint32_t* prim, uint32_t width, uint32_t height, const float* corners, uint32_t n_prims, const uint8_t* selected,
                             const zr_wire_style* style, size_t style_bytes, uint8_t* dst, size_t bytes)
{
    if (!rgba8 || !prim || !style || !dst || !width || !height || (n_prims && !corners) || style_bytes != sizeof(zr_wire_style)) return ZR_ERR_ARG;
    if (!zr_wire_style_ok(style) || bytes != (size_t)width * height * 4u) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        zr_wire_frame(rgba8, prim, width, height, corners, n_prims, selected, style, dst);
        return ZR_OK;
    });
}
