// zr_deliver_host.cpp — delivering the frame enqueued last behind the C-ABI (zelda_render.h, "delivering a scaled frame", "highlighting a
// selection", "delivering changes").  Every delivery is one path: the SOURCE STAGE (zr_deliver_source: the frame, highlighted or not -
// zr_highlight.hip - with the overlay's lines over it or not - zr_overlay_host.cpp - and box-filtered or not - zr_scale.hip) and then a
// FORM: the whole frame to the host or into a device buffer, or the tiles that changed since the last delivery (zr_delta.hip), raw or as
// records of the tile codec, each to the host or to the device.
// One check says whether the frame can be delivered (zr_deliver_ready).  No delivery is a stage of the frame: its launches go on the
// render stream behind the lighting pass of the frame enqueued last, where zr_copy_frame_async's copy goes, and the frame schedule knows
// nothing of them.  DESIGN.md section 5, "Delivering a frame: one path", has the launches call by call.
// Also here: the state of the deliveries of changes (zr_ctx::delta, its buffers for the delta extent - zr_delta_extent - and the scale
// they work at), the context-free host statements of the filter (zr_scale.h) and zr_frame_delta_decode, the client's side of a packed
// delivery (zr_delta_codec.h).  The set, the style and the highlight's switch for the deliveries of changes: zr_highlight_host.cpp.
#include "zr_ctx.h"
#include "zr_delta_codec.h"
#include "zr_highlight.h"

#include <cstring>

static constexpr size_t kTileBytes = (size_t)ZR_TILE * ZR_TILE * 4;
static_assert(sizeof(zr_frame_delta_packed) == 32 && kZrCodecTile == ZR_TILE, "the packed header is eight words; the codec's tile is the frame's");
static_assert(sizeof(zr_frame_delta) == 16 && offsetof(zr_frame_delta_packed, bytes) == 16, "the raw header is the packed one's first four words");

static bool scale_ok(uint32_t s) { return s >= 1u && s <= kZrScaleMax; }
static size_t scaled_pixels(const zr_ctx* c, uint32_t s) { return (size_t)zr_scale_extent(c->W, s) * zr_scale_extent(c->H, s); }

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

// ------------------------------------------------------------------------------------------------ the check and the source stage

// The context's lighting pass writes the row-major frame (else the refusal, in `what`'s name)
static int frame_is_row_major(zr_ctx* c, const char* what)
{
    if (c->cfg.tile_world > 1 || (c->cfg.flags & ZR_FLAG_PACKED_TILES))
        return zr_fail(c, ZR_ERR_UNSUPPORTED, std::string(what) + ": this context's lighting pass writes packed tiles, not the frame (tile_world > 1, ZR_FLAG_PACKED_TILES)");
    return ZR_OK;
}

// The frame enqueued last can be delivered: the lighting pass writes the frame, no frame is between its stages, a finished one is
// enqueued - and, for a highlighted delivery, it kept its winners and still describes the scene.  The device is current afterwards.
static int zr_deliver_ready(zr_ctx* c, const char* what, bool winners)
{
    if (int rc = frame_is_row_major(c, what)) return rc;
    if (int rc = zr_stage_idle(c, what)) return rc;
    if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": no finished frame enqueued");
    if (winners)
        if (int rc = ids_ready(c, what, false)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return ZR_OK;
}

// The source stage, on the render stream: what `what` (ZrDeliverWhat, zr_ctx.h) names, in its order.  dst: where the result goes, or
// null: the context's own scratch - each stage but the last writes its own frame (wire.frame and ov.frame, made by their stages;
// hl.frame, made here), the filter d_scaled (made here), all at first use, through `ext`; *out: where it lies - c->d_color itself
// when nothing was to be done.  A caller's dst is always written, by the last stage that runs: where no stage does and there is no
// factor, by the filter at scale 1, which is a copy.
static int zr_deliver_source(zr_ctx* c, ZrDeliverWhat what, uint32_t* dst, const uint32_t** out)
{
    zr_ctx::Highlight& L = c->hl;
    const bool overlay = what.overlay && !c->ov.seg.empty();      // (an empty list: no stage)
    const bool filter = what.scale > 1u || (dst && !what.wire && !what.highlight && !overlay);
    uint32_t* const hl_dst = filter || overlay ? nullptr : dst;      // (filtered or drawn over afterwards: highlighted into the scratch frame)
    if (what.highlight && !L.plane) HIPCHK(c, c->ext.alloc(&L.plane, (size_t)zr_hl_row_words(c->W) * c->H));
    if (what.highlight && !hl_dst && !L.frame) HIPCHK(c, c->ext.alloc(&L.frame, scaled_pixels(c, 1u)));
    if (filter && !dst && !c->d_scaled) HIPCHK(c, c->ext.alloc(&c->d_scaled, scaled_pixels(c, 2u)));      // (scale 2: the largest output)
    const uint32_t* src = c->d_color;
    if (what.wire)
        if (int rc = zr_wire_stage(c, src, what.highlight || overlay || filter ? nullptr : dst, &src)) return rc;
    if (what.highlight) {
        if (int rc = hl_upload(c)) return rc;
        uint32_t* const to = hl_dst ? hl_dst : L.frame;
        const ZrIdsArgs A = ids_args(c, 0, 0, c->W, c->H);
        zr_launch_highlight_mask(A.prim, A.draws, A.n_draws, L.bits, L.plane, c->W, c->H, c->stream);
        zr_launch_highlight_apply(src, L.plane, to, c->W, c->H, L.style, c->stream);
        if (int rc = ids_reader_enqueued(c)) return rc;      // (the mask read the last frame's winner plane)
        src = to;
    }
    if (overlay)
        if (int rc = zr_overlay_stage(c, src, filter ? nullptr : dst, &src)) return rc;
    if (filter) {
        uint32_t* const to = dst ? dst : c->d_scaled;
        zr_launch_frame_scale(src, to, c->W, c->H, what.scale, c->stream);
        src = to;
    }
    if (src != c->d_color) HIPCHK(c, hipGetLastError());
    *out = src;
    return ZR_OK;
}

// ------------------------------------------------------------------------------------------------ the form: the whole frame

// ... to the host: zr_finish first (its overflow is the call's error), and the delivered frame is all that crosses the link
int zr_deliver_to_host(zr_ctx* c, const char* what, ZrDeliverWhat w, uint8_t* dst, size_t bytes)
{
    ARGCHK(c, dst && scale_ok(w.scale));
    ARGCHK(c, bytes == scaled_pixels(c, w.scale) * 4u);
    int rc = zr_deliver_ready(c, what, w.wire || w.highlight);
    if (rc == ZR_OK) rc = zr_finish(c);
    const uint32_t* src = nullptr;
    if (rc == ZR_OK) rc = zr_deliver_source(c, w, nullptr, &src);
    if (rc) return rc;
    if (src != c->d_color) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return ZR_OK;
}

// ... into a caller-owned device buffer, in stream order
int zr_deliver_to_device(zr_ctx* c, const char* what, ZrDeliverWhat w, void* color_dev)
{
    ARGCHK(c, color_dev && (uintptr_t)color_dev % 4 == 0 && scale_ok(w.scale));
    if (int rc = zr_deliver_ready(c, what, w.wire || w.highlight)) return rc;
    const uint32_t* at = nullptr;
    return zr_deliver_source(c, w, (uint32_t*)color_dev, &at);
}

extern "C" int zr_read_color_scaled(zr_ctx* c, uint32_t scale, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return zr_deliver_to_host(c, "zr_read_color_scaled", { false, false, false, scale }, dst, bytes); });
}

extern "C" int zr_copy_frame_scaled_async(zr_ctx* c, uint32_t scale, void* color_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return zr_deliver_to_device(c, "zr_copy_frame_scaled_async", { false, false, false, scale }, color_dev); });
}

extern "C" int zr_read_color_highlighted(zr_ctx* c, uint32_t scale, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return zr_deliver_to_host(c, "zr_read_color_highlighted", { false, true, false, scale }, dst, bytes); });
}

extern "C" int zr_copy_frame_highlighted_async(zr_ctx* c, uint32_t scale, void* color_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { return zr_deliver_to_device(c, "zr_copy_frame_highlighted_async", { false, true, false, scale }, color_dev); });
}

// ------------------------------------------------------------------------------------------------ the form: changed tiles - the state

// What the packed forms need beyond the raw forms' buffers, made into `mem`: the lengths (16 bits per tile, in whole 16-byte words, the
// padding 0), and the host form's header, offsets and stream with its pinned landing place
static int delta_make_packed(zr_ctx* c, const ZrDeltaExtent& E, ZrOwn& mem, ZrDeltaBuffers::Codec& P)
{
    if ((uint64_t)E.n_tiles * kZrCodecRawBytes > 0xFFFFFFFFull)
        return zr_fail(c, ZR_ERR_UNSUPPORTED, "zr_set_frame_delta: the frame's packed stream would not fit 32-bit offsets");
    const size_t len_words = ((size_t)E.n_tiles + 7u) / 8u * 8u;
    HIPCHK(c, mem.alloc(&P.lens, len_words)); HIPCHK(c, mem.alloc(&P.header, 8)); HIPCHK(c, mem.alloc(&P.offsets, (size_t)E.n_tiles + 1u));
    HIPCHK(c, mem.alloc(&P.stream, (size_t)E.n_tiles * kZrCodecRawBytes)); HIPCHK(c, mem.host(&P.h_header, 1));
    HIPCHK(c, zr_fill_sync({ { P.lens, 0, len_words * 2 }, { P.header, 0, 32 } }));
    P.on = true;
    return ZR_OK;
}

// Everything is made for the delivered extent: the frame's own, or at a delta scale above 1 the scaled frame's, which every delivery
// then filters into `scaled` first.  zr_set_frame_delta makes it for the context's extent, zr_resize for the new one.
int zr_delta_make(zr_ctx* c, uint32_t W, uint32_t H, bool codec, ZrDeltaBuffers* out)
{
    ZrDeltaBuffers& B = *out;
    const ZrDeltaExtent E = zr_delta_extent_of(W, H, c->delta.scale);
    const size_t n = (size_t)E.W * E.H, flag_bytes = ((size_t)E.n_tiles + 7u) / 8u * 8u;      // (k_delta_pack reads the flags eight at a time)
    if (c->delta.scale > 1u) HIPCHK(c, B.mem.alloc(&B.scaled, n));
    HIPCHK(c, B.mem.alloc(&B.delivered, n)); HIPCHK(c, B.mem.alloc(&B.packed, (size_t)E.n_tiles * kTileBytes)); HIPCHK(c, B.mem.alloc(&B.list, E.n_tiles));
    HIPCHK(c, B.mem.alloc(&B.header, 4)); HIPCHK(c, B.mem.alloc(&B.flags, flag_bytes)); HIPCHK(c, B.mem.host(&B.h_header, 1));
    HIPCHK(c, zr_fill_sync({ { B.delivered, 0, n * 4 }, { B.flags, 0, flag_bytes }, { B.header, 0, 16 } }));
    return codec ? delta_make_packed(c, E, B.codec_mem, B.codec) : ZR_OK;
}

extern "C" int zr_set_frame_delta(zr_ctx* c, int enable)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = zr_stage_idle(c, "zr_set_frame_delta", false)) return rc;
        zr_ctx::Delta& D = c->delta;
        const bool on = enable != 0, codec = enable == ZR_FRAME_DELTA_PACKED;
        if (on == D.on && (!on || codec == D.b.codec.on)) return ZR_OK;
        HIPCHK(c, hipSetDevice(c->device));
        if (!on) {
            HIPCHK(c, zr_sync_all(c));           // (deliveries in flight read and write what is released here)
            D.b = ZrDeltaBuffers();
            D.on = false; D.full = true; D.serial = 0;
            return ZR_OK;
        }
        if (D.on) {                              // between the raw and the packed forms: the delivered copy, full and serial stand
            HIPCHK(c, zr_sync_all(c));
            ZrOwn pmem; ZrDeltaBuffers::Codec P;
            if (codec) if (int rc = delta_make_packed(c, zr_delta_extent(c), pmem, P)) return rc;
            D.b.codec_mem = std::move(pmem); D.b.codec = P;
            return ZR_OK;
        }
        if (int rc = frame_is_row_major(c, "zr_set_frame_delta")) return rc;
        ZrDeltaBuffers B;
        if (int rc = zr_delta_make(c, c->W, c->H, codec, &B)) return rc;
        D.b = std::move(B);
        D.on = true; D.full = true; D.serial = 0;
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

extern "C" int zr_frame_delta_reset(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->delta.on) return zr_fail(c, ZR_ERR_STATE, "zr_frame_delta_reset: frame delta is off (zr_set_frame_delta)");
        c->delta.full = true;
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ the form: changed tiles - a delivery

// What the raw and the packed form of a delivery differ in: the header's size, where header, list and payload (raw: the tiles' pixels;
// packed: the stream of records, with its offsets) go on the device, and with `offsets` which launcher runs.  h_header: the host forms'
// pinned landing place of the header.
struct DeltaForm {
    const char* what; size_t header_bytes;
    uint32_t *header, *list, *offsets; void* payload;      // offsets null: the raw form
    void* h_header;
};

// Delta is on, and the frame enqueued last can be delivered (wire or highlight delivery on: as such a one)
static int delta_ready(zr_ctx* c, const char* what)
{
    if (!c->delta.on) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": frame delta is off (zr_set_frame_delta)");
    return zr_deliver_ready(c, what, c->wire.delta || c->hl.delta);
}

// Packed delivery is enabled: asked before the arguments are looked at, so that a host in mode 1 hears ZR_ERR_STATE whatever it passed
static int delta_packed_enabled(zr_ctx* c, const char* what)
{
    if (c->delta.on && c->delta.b.codec.on) return ZR_OK;
    return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": packed delivery is not enabled (zr_set_frame_delta with ZR_FRAME_DELTA_PACKED)");
}

// One delivery on the render stream: the source stage (into `scaled` at a delta scale above 1), then the form's launches on what it
// left.  full and serial are the host's to know, the kernels only write them into the header.
static int delta_enqueue(zr_ctx* c, const DeltaForm& F)
{
    zr_ctx::Delta& D = c->delta;
    const ZrDeltaExtent E = zr_delta_extent(c);
    const uint32_t serial = D.serial + 1u, full = D.full ? 1u : 0u;
    const uint32_t* frame = nullptr;
    if (int rc = zr_deliver_source(c, { c->wire.delta, c->hl.delta, c->ov.delta, D.scale }, D.b.scaled, &frame)) return rc;
    if (F.offsets)
        zr_launch_frame_delta_packed(frame, D.b.delivered, D.b.flags, D.b.codec.lens, F.header, F.list, F.offsets, F.payload, E.W, E.H, E.tiles_x, E.n_tiles, full, serial,
                                     c->stream);
    else
        zr_launch_frame_delta(frame, D.b.delivered, D.b.flags, F.header, F.list, F.payload, E.W, E.H, E.tiles_x, E.n_tiles, full, serial, c->stream);
    HIPCHK(c, hipGetLastError());
    D.serial = serial; D.full = false;
    return ZR_OK;
}

// A host form: zr_finish, the delivery into the context's buffers (F), the header through pinned memory, and then only what it lists
// crosses the link.  cap_bytes: the room behind `payload`; offsets: the packed form's (offsets[0] = 0 even where nothing is listed).
static int delta_read(zr_ctx* c, const DeltaForm& F, uint32_t* tiles, uint32_t* offsets, uint8_t* payload, size_t cap_bytes, void* out)
{
    const ZrDeltaExtent E = zr_delta_extent(c);
    int rc = delta_ready(c, F.what);
    if (rc == ZR_OK) rc = zr_finish(c);
    if (rc == ZR_OK) rc = delta_enqueue(c, F);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(F.h_header, F.header, F.header_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    zr_frame_delta_packed h = {};
    memcpy(&h, F.h_header, F.header_bytes);
    const size_t bytes = offsets ? h.bytes : (size_t)h.n_tiles * kTileBytes;
    if (h.n_tiles > E.n_tiles || bytes > cap_bytes) return zr_fail(c, ZR_ERR_DEVICE, std::string(F.what) + ": more listed than the frame has");
    if (offsets) offsets[0] = 0u;
    if (h.n_tiles) {
        HIPCHK(c, hipMemcpyAsync(tiles, F.list, (size_t)h.n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
        if (offsets) HIPCHK(c, hipMemcpyAsync(offsets, F.offsets, ((size_t)h.n_tiles + 1u) * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(payload, F.payload, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    memcpy(out, &h, F.header_bytes);
    return ZR_OK;
}

extern "C" int zr_read_frame_delta(zr_ctx* c, uint32_t* tiles, uint32_t cap_tiles, uint8_t* pixels, size_t bytes, zr_frame_delta* out, size_t out_bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const ZrDeltaExtent E = zr_delta_extent(c);
        ARGCHK(c, tiles && pixels && out && out_bytes >= sizeof(zr_frame_delta));
        ARGCHK(c, cap_tiles == E.n_tiles && bytes == (size_t)E.n_tiles * kTileBytes);
        const ZrDeltaBuffers& B = c->delta.b;
        return delta_read(c, { "zr_read_frame_delta", sizeof(zr_frame_delta), B.header, B.list, nullptr, B.packed, B.h_header }, tiles, nullptr, pixels, bytes, out);
    });
}

extern "C" int zr_copy_frame_delta_async(zr_ctx* c, void* header_dev, void* tiles_dev, void* pixels_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, header_dev && tiles_dev && pixels_dev);
        ARGCHK(c, (uintptr_t)header_dev % 4 == 0 && (uintptr_t)tiles_dev % 4 == 0 && (uintptr_t)pixels_dev % 16 == 0);
        if (int rc = delta_ready(c, "zr_copy_frame_delta_async")) return rc;
        return delta_enqueue(c, { "zr_copy_frame_delta_async", sizeof(zr_frame_delta), (uint32_t*)header_dev, (uint32_t*)tiles_dev, nullptr, pixels_dev, nullptr });
    });
}

extern "C" int zr_read_frame_delta_packed(zr_ctx* c, uint32_t* tiles, uint32_t cap_tiles, uint32_t* offsets, uint32_t cap_offsets, uint8_t* stream, size_t cap_bytes,
                                          zr_frame_delta_packed* out, size_t out_bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = delta_packed_enabled(c, "zr_read_frame_delta_packed")) return rc;
        const ZrDeltaExtent E = zr_delta_extent(c);
        ARGCHK(c, tiles && offsets && stream && out && out_bytes >= sizeof(zr_frame_delta_packed));
        ARGCHK(c, cap_tiles == E.n_tiles && cap_offsets == E.n_tiles + 1u && cap_bytes == (size_t)E.n_tiles * kZrCodecRawBytes);
        const ZrDeltaBuffers::Codec& P = c->delta.b.codec;
        return delta_read(c, { "zr_read_frame_delta_packed", sizeof(zr_frame_delta_packed), P.header, c->delta.b.list, P.offsets, P.stream, P.h_header }, tiles, offsets,
                          stream, cap_bytes, out);
    });
}

extern "C" int zr_copy_frame_delta_packed_async(zr_ctx* c, void* header_dev, void* tiles_dev, void* offsets_dev, void* stream_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = delta_packed_enabled(c, "zr_copy_frame_delta_packed_async")) return rc;
        ARGCHK(c, header_dev && tiles_dev && offsets_dev && stream_dev);
        ARGCHK(c, (uintptr_t)header_dev % 4 == 0 && (uintptr_t)tiles_dev % 4 == 0 && (uintptr_t)offsets_dev % 4 == 0 && (uintptr_t)stream_dev % 16 == 0);
        if (int rc = delta_ready(c, "zr_copy_frame_delta_packed_async")) return rc;
        return delta_enqueue(c, { "zr_copy_frame_delta_packed_async", sizeof(zr_frame_delta_packed), (uint32_t*)header_dev, (uint32_t*)tiles_dev, (uint32_t*)offsets_dev,
                                  stream_dev, nullptr });
    });
}

extern "C" int zr_frame_delta_decode(const uint32_t* tiles, const uint32_t* offsets, uint32_t n, const uint8_t* stream, size_t bytes, uint32_t width, uint32_t height,
                                     uint8_t* client_rgba8)
{
    if (!offsets || !client_rgba8 || !width || !height || (n && (!tiles || !stream))) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        return zr_codec_apply(tiles, offsets, n, stream, bytes, width, height, client_rgba8) ? ZR_OK : ZR_ERR_PARSE;
    });
}
