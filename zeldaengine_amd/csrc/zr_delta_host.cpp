// zr_delta_host.cpp — delivering a frame as the tiles that changed since the last delivery, behind the C-ABI (zelda_render.h,
// "delivering changes"): the state (zr_ctx::delta), the host form and the device form.  A delivery is not a stage of the frame: it is two
// launches (zr_delta.hip) on the render stream behind the lighting pass of the frame enqueued last, where zr_copy_frame_async's copy
// goes, and the frame schedule knows nothing of it.  The packed forms (zr_set_frame_delta(ctx, ZR_FRAME_DELTA_PACKED)) deliver the same list
// with every tile as a record of the tile codec: three launches, buffers of their own beside the raw forms', the same delivered copy.
// zr_frame_delta_decode is the client's side of them and needs no context (zr_delta_codec.h).
// At a delta scale above 1 (zr_set_frame_delta_scale, zr_scale_host.cpp) all of it is made for the scaled extent (zr_delta_extent), and
// every delivery first filters the frame into `scaled` (zr_scale.hip) and then runs the same launches on that.
// With highlight delivery on (zr_set_frame_delta_highlight, zr_highlight_host.cpp) the frame is highlighted ahead of all that.
#include "zr_ctx.h"
#include "zr_delta_codec.h"

#include <cstring>

static constexpr size_t kTileBytes = (size_t)ZR_TILE * ZR_TILE * 4;
static_assert(sizeof(zr_frame_delta_packed) == 32 && kZrCodecTile == ZR_TILE, "the packed header is eight words; the codec's tile is the frame's");

// What the packed forms need beyond the raw forms' buffers, made into `mem`: the lengths (16 bits per tile, in whole 16-byte words, the
// padding 0), and the host form's header, offsets and stream with its pinned landing place
static int delta_make_packed(zr_ctx* c, const ZrDeltaExtent& E, ZrOwn& mem, zr_ctx::Delta::Codec& P)
{
    if ((uint64_t)E.n_tiles * kZrCodecRawBytes > 0xFFFFFFFFull)
        return zr_fail(c, ZR_ERR_UNSUPPORTED, "zr_set_frame_delta: the frame's packed stream would not fit 32-bit offsets");
    const size_t len_words = ((size_t)E.n_tiles + 7u) / 8u * 8u;
    HIPCHK(c, mem.alloc(&P.lens, len_words)); HIPCHK(c, mem.alloc(&P.header, 8)); HIPCHK(c, mem.alloc(&P.offsets, (size_t)E.n_tiles + 1u));
    HIPCHK(c, mem.alloc(&P.stream, (size_t)E.n_tiles * kZrCodecRawBytes)); HIPCHK(c, mem.host(&P.h_header, 1));
    HIPCHK(c, zr_fill_sync({ { P.lens, 0, len_words * 2 }, { P.header, 0, 32 } }));
    return ZR_OK;
}

// Everything is made for the delivered extent: the frame's own, or at a delta scale above 1 the scaled frame's, which every delivery
// then filters into `scaled` first (zr_scale.hip).  zr_set_frame_delta makes it for the context's extent, zr_resize for the new one.
int zr_delta_make(zr_ctx* c, uint32_t W, uint32_t H, bool codec, ZrDeltaBuffers* out)
{
    ZrDeltaBuffers& B = *out;
    const ZrDeltaExtent E = zr_delta_extent_of(W, H, c->delta.scale);
    const size_t n = (size_t)E.W * E.H, flag_bytes = ((size_t)E.n_tiles + 7u) / 8u * 8u;      // (k_delta_pack reads the flags eight at a time)
    if (c->delta.scale > 1u) HIPCHK(c, B.mem.alloc(&B.scaled, n));
    HIPCHK(c, B.mem.alloc(&B.delivered, n)); HIPCHK(c, B.mem.alloc(&B.packed, (size_t)E.n_tiles * kTileBytes)); HIPCHK(c, B.mem.alloc(&B.list, E.n_tiles));
    HIPCHK(c, B.mem.alloc(&B.header, 4)); HIPCHK(c, B.mem.alloc(&B.flags, flag_bytes)); HIPCHK(c, B.mem.host(&B.h_header, 1));
    HIPCHK(c, zr_fill_sync({ { B.delivered, 0, n * 4 }, { B.flags, 0, flag_bytes }, { B.header, 0, 16 } }));
    if (codec) { if (int rc = delta_make_packed(c, E, B.codec_mem, B.codec)) return rc; B.codec.on = true; }
    return ZR_OK;
}
void zr_delta_commit(zr_ctx* c, ZrDeltaBuffers& B)
{
    zr_ctx::Delta& D = c->delta;
    D.codec_mem = std::move(B.codec_mem); D.codec = B.codec;
    D.mem = std::move(B.mem);
    D.delivered = B.delivered; D.scaled = B.scaled; D.packed = B.packed; D.list = B.list; D.header = B.header; D.flags = B.flags; D.h_header = B.h_header;
}

extern "C" int zr_set_frame_delta(zr_ctx* c, int enable)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = zr_stage_idle(c, "zr_set_frame_delta", false)) return rc;
        zr_ctx::Delta& D = c->delta;
        const bool on = enable != 0, codec = enable == ZR_FRAME_DELTA_PACKED;
        if (on == D.on && (!on || codec == D.codec.on)) return ZR_OK;
        HIPCHK(c, hipSetDevice(c->device));
        if (!on) {
            HIPCHK(c, zr_sync_all(c));           // (deliveries in flight read and write what is released here)
            const uint32_t scale = D.scale;      // (zr_set_frame_delta_scale's: kept across the switch)
            D.mem.release();
            D = zr_ctx::Delta();
            D.scale = scale;
            return ZR_OK;
        }
        if (D.on) {                              // between the raw and the packed forms: the delivered copy, full and serial stand
            HIPCHK(c, zr_sync_all(c));
            ZrOwn pmem; zr_ctx::Delta::Codec P;
            if (codec) { if (int rc = delta_make_packed(c, zr_delta_extent(c), pmem, P)) return rc; P.on = true; }
            D.codec_mem = std::move(pmem); D.codec = P;
            return ZR_OK;
        }
        if (c->cfg.tile_world > 1 || (c->cfg.flags & ZR_FLAG_PACKED_TILES))
            return zr_fail(c, ZR_ERR_UNSUPPORTED, "zr_set_frame_delta: this context's lighting pass writes packed tiles, not the frame (tile_world > 1, ZR_FLAG_PACKED_TILES)");
        ZrDeltaBuffers B;
        if (int rc = zr_delta_make(c, c->W, c->H, codec, &B)) return rc;
        zr_delta_commit(c, B);
        D.on = true; D.full = true; D.serial = 0;
        return ZR_OK;
    });
}

// Delta is on, and the frame enqueued last is a finished one
static int delta_ready(zr_ctx* c, const char* what)
{
    if (!c->delta.on) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": frame delta is off (zr_set_frame_delta)");
    if (int rc = zr_stage_idle(c, what)) return rc;
    if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": no finished frame enqueued");
    return c->hl.delta ? zr_highlight_ready(c, what) : ZR_OK;      // (a highlighted delivery needs a captured frame)
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

// What a delivery compares and lists (*frame): the frame - with highlight delivery on, the frame highlighted into the context's buffer
// first - or at a delta scale above 1 that filtered into `scaled`, on the render stream
static int delta_frame(zr_ctx* c, const uint32_t** frame)
{
    const zr_ctx::Delta& D = c->delta;
    *frame = c->d_color;
    if (c->hl.delta)
        if (int rc = zr_highlight_enqueue(c, nullptr, frame)) return rc;
    if (D.scale <= 1u) return ZR_OK;
    zr_launch_frame_scale(*frame, D.scaled, c->W, c->H, D.scale, c->stream);
    *frame = D.scaled;
    return ZR_OK;
}

// One delivery on the render stream; full and serial are the host's to know, the kernels only write them into the header
static int delta_enqueue(zr_ctx* c, uint32_t* header_dev, uint32_t* list_dev, void* packed_dev)
{
    zr_ctx::Delta& D = c->delta;
    const ZrDeltaExtent E = zr_delta_extent(c);
    const uint32_t serial = D.serial + 1u;
    const uint32_t* frame = nullptr;
    if (int rc = delta_frame(c, &frame)) return rc;
    zr_launch_frame_delta(frame, D.delivered, D.flags, header_dev, list_dev, packed_dev, E.W, E.H, E.tiles_x, E.n_tiles, D.full ? 1u : 0u, serial,
                          c->stream);
    HIPCHK(c, hipGetLastError());
    D.serial = serial; D.full = false;
    return ZR_OK;
}

extern "C" int zr_read_frame_delta(zr_ctx* c, uint32_t* tiles, uint32_t cap_tiles, uint8_t* pixels, size_t bytes, zr_frame_delta* out, size_t out_bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const ZrDeltaExtent E = zr_delta_extent(c);
        ARGCHK(c, tiles && pixels && out && out_bytes >= sizeof(zr_frame_delta));
        ARGCHK(c, cap_tiles == E.n_tiles && bytes == (size_t)E.n_tiles * kTileBytes);
        int rc = delta_ready(c, "zr_read_frame_delta");
        if (rc == ZR_OK) rc = zr_finish(c);
        if (rc == ZR_OK) rc = delta_enqueue(c, c->delta.header, c->delta.list, c->delta.packed);
        if (rc) return rc;
        const zr_ctx::Delta& D = c->delta;
        HIPCHK(c, hipMemcpyAsync(D.h_header, D.header, sizeof(zr_frame_delta), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const zr_frame_delta h = *D.h_header;
        if (h.n_tiles > E.n_tiles) return zr_fail(c, ZR_ERR_DEVICE, "zr_read_frame_delta: more tiles listed than the frame has");
        if (h.n_tiles) {
            HIPCHK(c, hipMemcpyAsync(tiles, D.list, (size_t)h.n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(pixels, D.packed, (size_t)h.n_tiles * kTileBytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        memcpy(out, &h, sizeof h);
        return ZR_OK;
    });
}

extern "C" int zr_copy_frame_delta_async(zr_ctx* c, void* header_dev, void* tiles_dev, void* pixels_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, header_dev && tiles_dev && pixels_dev);
        ARGCHK(c, (uintptr_t)header_dev % 4 == 0 && (uintptr_t)tiles_dev % 4 == 0 && (uintptr_t)pixels_dev % 16 == 0);
        if (int rc = delta_ready(c, "zr_copy_frame_delta_async")) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        return delta_enqueue(c, (uint32_t*)header_dev, (uint32_t*)tiles_dev, pixels_dev);
    });
}

// ------------------------------------------------------------------------------------------------ the packed forms

// Packed delivery is enabled: asked before the arguments are looked at, so that a host in mode 1 hears ZR_ERR_STATE whatever it passed
static int delta_packed_enabled(zr_ctx* c, const char* what)
{
    if (c->delta.on && c->delta.codec.on) return ZR_OK;
    return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": packed delivery is not enabled (zr_set_frame_delta with ZR_FRAME_DELTA_PACKED)");
}

static int delta_enqueue_packed(zr_ctx* c, uint32_t* header_dev, uint32_t* list_dev, uint32_t* offsets_dev, void* stream_dev)
{
    zr_ctx::Delta& D = c->delta;
    const ZrDeltaExtent E = zr_delta_extent(c);
    const uint32_t serial = D.serial + 1u;
    const uint32_t* frame = nullptr;
    if (int rc = delta_frame(c, &frame)) return rc;
    zr_launch_frame_delta_packed(frame, D.delivered, D.flags, D.codec.lens, header_dev, list_dev, offsets_dev, stream_dev, E.W, E.H, E.tiles_x, E.n_tiles,
                                 D.full ? 1u : 0u, serial, c->stream);
    HIPCHK(c, hipGetLastError());
    D.serial = serial; D.full = false;
    return ZR_OK;
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
        int rc = delta_ready(c, "zr_read_frame_delta_packed");
        if (rc == ZR_OK) rc = zr_finish(c);
        const zr_ctx::Delta::Codec& P = c->delta.codec;
        if (rc == ZR_OK) rc = delta_enqueue_packed(c, P.header, c->delta.list, P.offsets, P.stream);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(P.h_header, P.header, sizeof(zr_frame_delta_packed), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const zr_frame_delta_packed h = *P.h_header;
        if (h.n_tiles > E.n_tiles || h.bytes > cap_bytes) return zr_fail(c, ZR_ERR_DEVICE, "zr_read_frame_delta_packed: more listed than the frame has");
        offsets[0] = 0u;
        if (h.n_tiles) {                         // the compressed bytes are all that cross the link
            HIPCHK(c, hipMemcpyAsync(tiles, c->delta.list, (size_t)h.n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(offsets, P.offsets, ((size_t)h.n_tiles + 1u) * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(stream, P.stream, h.bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        memcpy(out, &h, sizeof h);
        return ZR_OK;
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
        HIPCHK(c, hipSetDevice(c->device));
        return delta_enqueue_packed(c, (uint32_t*)header_dev, (uint32_t*)tiles_dev, (uint32_t*)offsets_dev, stream_dev);
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
